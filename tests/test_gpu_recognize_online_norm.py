"""The online recognizer and the command line's --online form with a normalisation spec, on the
80-dim model file of tests/test_gpu_frontend_recognizer.py.  The norm is set on OnlineRecognizer.scorer; speaker
statistics travel with open / open_features.  The yardstick is Recognizer.process under the same spec -- what
tests/test_gpu_recognize_norm.py and tests/test_gpu_online_cmvn.py pin -- field for field, floats by their bits; the
command line prints the same stdout with --online as without it."""
import os
import shutil

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import recognize

import norm_cases as NC
import refmodel_files as RF
from refmodel_text import load_text_model
from test_gpu_frontend_recognizer import CAT, DIR, HELLO, L, R, SPEC, SPEC_TEXT, STATS, TRACE, comparable, model_layers
from test_gpu_recognize_norm import binary_matrix

pytestmark = pytest.mark.gpu

FILES = [HELLO, CAT]
MODES = [("none", pk.NormSpec("none")), ("speaker", pk.NormSpec("speaker", True, True)), ("online8", pk.OnlineCmvnSpec(8, 3, 2, True)),
         ("online600", pk.OnlineCmvnSpec())]


def is_online(spec):
    return isinstance(spec, pk.OnlineCmvnSpec)


def set_norm(obj, spec, glob):
    obj.set_norm(spec, glob) if is_online(spec) else obj.set_norm(spec)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recognize_online_norm")
    layers, prior = model_layers()
    tid2pdf = load_text_model()[4]
    conf = RF.write_model(tmp, layers, prior, L, R, tid2pdf=tid2pdf, cmvn_stats=STATS)
    for name in ("wordloop.fst", "wordloop_words.bin"):
        shutil.copy(os.path.join(DIR, name), str(tmp / name))
    with open(conf, "a") as f:
        f.write("fst = wordloop.fst\nsymbol_table = wordloop_words.bin\n")
    waves = [pk.read_wav(f) for f in FILES]
    rec = pk.Recognizer(conf, max_utts=2, max_total_samples=sum(len(w) for w in waves), trace_capacity=TRACE, frontend=SPEC)
    rec.process(waves)
    rows = [rec.batch.fetch_fbank(u) for u in range(2)]
    glob = sum(NC.accumulate(r) for r in rows)
    spk = [NC.accumulate(rows[1]), NC.accumulate(rows[0]) * 2.0]
    want = {}
    for name, spec in MODES:
        set_norm(rec.batch, spec, glob)
        want[name] = rec.process(waves, speaker_stats=None if name == "none" else spk)
    rec.close()
    print("hypotheses: %r" % {k: [r.text for r in v] for k, v in want.items()})
    return conf, waves, rows, glob, spk, want


def stream(online, waves, spk, chunk=1600, feats=None):
    """Wave (or [T][D] matrix, ten frames a step) u into slot u, closed with its last chunk -> the Results."""
    data = feats if feats is not None else waves
    step = 10 if feats is not None else chunk
    pos, live, out = [0] * len(data), set(range(len(data))), {}
    for u in live:
        record = None if spk is None else spk[u]
        online.open_features(u, "raw", speaker_stats=record) if feats is not None else online.open(u, speaker_stats=record)
    while live:
        closing = []
        for u in sorted(live):
            (online.push_features if feats is not None else online.push)(u, data[u][pos[u]:pos[u] + step])
            pos[u] += step
            if pos[u] >= len(data[u]):
                online.close(u)
                closing.append(u)
        online.step()
        for u in closing:
            assert online.finished(u)
            out[u] = online.result(u)
            live.discard(u)
    return [out[u] for u in range(len(data))]


@pytest.mark.parametrize("name, spec", MODES, ids=[m[0] for m in MODES])
def test_online_recognizer_is_the_batch_recognizer(setup, name, spec):
    conf, waves, rows, glob, spk, want = setup
    records = None if name == "none" else spk
    online = pk.OnlineRecognizer(conf, max_streams=2, max_step_samples=2 * 1600, trace_capacity=TRACE, frontend=SPEC)
    set_norm(online.scorer, spec, glob)
    got = stream(online, waves, records)
    for u in range(2):
        assert comparable(got[u]) == comparable(want[name][u]), (name, u)
    got = stream(online, waves, records, feats=rows)                              # the front-end's rows as RAW frames
    for u in range(2):
        assert comparable(got[u]) == comparable(want[name][u]), (name, "raw features", u)
    if name == "online8":
        # endpointing on, with rules that cannot fire on half a second of audio: nothing is cut, each slot's one utterance
        # is the batch Result
        online.set_endpointing([10], [pk.EndpointRule(True, 5.0, np.inf, 0.0), pk.EndpointRule(False, 0.0, np.inf, 20.0)])
        online.decoder.set_commit(True)
        got = stream(online, waves, records)
        for u in range(2):
            assert comparable(got[u]) == comparable(want[name][u]), (name, "endpointing", u)
            pieces = online.utterances(u)
            assert [(p.first_frame, p.num_frames, p.rule) for p in pieces] == [(0, pk.num_frames(len(waves[u])), 0)]
            assert comparable(pieces[0].result) == comparable(want[name][u])
    online.destroy()


def test_command_line_prints_the_same_with_online(setup, tmp_path, capsys):
    conf, waves, rows, glob, spk, want = setup
    front = ["--frontend", SPEC_TEXT]
    listing = str(tmp_path / "waves.scp")
    with open(listing, "w") as f:
        f.write("\n".join(FILES) + "\n")
    ark = str(tmp_path / "feats.ark")
    with open(ark, "wb") as f:
        for k, r in zip(FILES, rows):
            f.write(k.encode() + b" " + binary_matrix(r, "FM"))
    global_file = str(tmp_path / "global.stats")
    with open(global_file, "wb") as f:
        f.write(binary_matrix(glob))
    by_utt = str(tmp_path / "by_utt.ark")
    with open(by_utt, "wb") as f:
        for k, s in zip(FILES, spk):
            f.write(k.encode() + b" " + binary_matrix(s))
    flag_sets = {"none": ["--cmvn", "mode=none"],
                 "speaker": ["--cmvn", "mode=speaker,norm_vars=true", "--cmvn-stats", "ark:" + by_utt],
                 "online8": ["--cmvn", "mode=online,cmn_window=8,speaker_frames=3,global_frames=2,norm_vars=true", "--cmvn-global", global_file,
                             "--cmvn-stats", by_utt],
                 "online600": ["--cmvn", "mode=online", "--cmvn-global", global_file, "--cmvn-stats", by_utt]}
    for name, flags in flag_sets.items():
        lines = "".join("%s\t%s\t%f\n" % (n, r.text, r.loglikelihood_per_frame) for n, r in zip(FILES, want[name]))
        for inputs in ([HELLO], [listing], ["ark:" + ark, "--features", "raw"]):
            assert recognize.main([conf] + inputs + front + flags) == 0, (name, inputs)
            batch = capsys.readouterr().out
            assert recognize.main([conf] + inputs + front + flags + ["--online"]) == 0, (name, inputs)
            assert capsys.readouterr().out == batch, (name, inputs)
            assert batch == (lines if inputs[0] != HELLO else lines.splitlines(True)[0]), (name, inputs)
