"""The recognizers with a front-end spec: pk.Recognizer(conf, frontend=spec),
pk.OnlineRecognizer(conf, frontend=spec) and python -m pocketkaldi_amd.recognize --frontend, on a model file of an 80-dim
model written into tmp_path (tests/refmodel_files.py) beside the fixture's word-loop graph and word list.  The yardstick
is pk.Decoder.decode_batch over pk.BatchScorer(frontend=spec) -- what tests/test_gpu_frontend_any.py pins -- joined
through the symbol table; every comparison is field for field, floats by their bits.

The model's weights are drawn from seed SEED: the two golden waves then decode to the words [2, 3] and [3] through the
numpy restatement of the front-end, the oracle's CMVN and layers and tests/decoder_model.py (found on a CPU before the
seed was written down), so neither hypothesis is empty."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import pocketkaldi_amd as pk

import frontend_any_cases as FA
import refmodel_files as RF
from refmodel_text import load_text_model

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
DIR = os.path.join(G, "refmodel")
HELLO, CAT = os.path.join(G, "en-us-hello.wav"), os.path.join(G, "en-us-cat.wav")
E_INVALID = -1
TRACE = 1 << 20
D, L, R, HIDDEN, PDFS, SEED = 80, 2, 1, 64, 18, 0
SPEC = FA.BATCH_SPECS[D]
SPEC_TEXT = "num_mel_bins=80,window=povey,low_freq=20,high_freq=-400"
STATS = np.concatenate([np.full(D, 12.0 * 2500.0), [2500.0]]).astype(np.float32)      # count 2500, every mean 12


def bits(x):
    return np.float32(x).tobytes()


def comparable(r):
    return (r.text, r.words, bits(r.weight), r.ok, bits(r.loglikelihood_per_frame),
            [(s.word, s.start_frame, s.num_frames, bits(s.graph_cost), bits(s.acoustic_cost)) for s in r.segments])


def model_layers():
    rng = np.random.default_rng([0xF18, SEED])
    dims = [D * (L + R + 1), HIDDEN, HIDDEN, PDFS]
    layers = []
    for i in range(3):
        W = (rng.standard_normal((dims[i + 1], dims[i])) * np.sqrt(2.0 / dims[i])).astype(np.float32)
        layers += [("linear", W, (rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32)), ("relu",) if i < 2 else ("softmax",)]
    return layers, np.full(PDFS, 1.0 / PDFS, np.float32)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The model file, the two waves, and the yardstick's Results with the batch object's fbank rows (computed once)."""
    tmp = tmp_path_factory.mktemp("frontend_recognizer")
    layers, prior = model_layers()
    tid2pdf = load_text_model()[4]
    assert len(prior) == PDFS and max(tid2pdf) < PDFS
    conf = RF.write_model(tmp, layers, prior, L, R, tid2pdf=tid2pdf, cmvn_stats=STATS)
    for name in ("wordloop.fst", "wordloop_words.bin"):
        shutil.copy(os.path.join(DIR, name), str(tmp / name))
    with open(conf, "a") as f:
        f.write("fst = wordloop.fst\nsymbol_table = wordloop_words.bin\n")
    waves = [pk.read_wav(HELLO), pk.read_wav(CAT)]
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    bs = pk.BatchScorer(am, STATS, 2, sum(len(w) for w in waves), frontend=SPEC)
    bs.set_waves(waves)
    bs.score(0.1)
    fst = pk.Fst(os.path.join(DIR, "wordloop.fst"))
    dec = pk.Decoder(fst, am, 2, trace_capacity=TRACE)
    dec.set_alignment(True)
    dec.decode_batch(bs)
    names = pk.SymbolTable(os.path.join(DIR, "wordloop_words.bin"))
    want, fbank = [], []
    for u in range(2):
        words, weight, ok = dec.result(u)
        spoken = bool(ok and words)
        text = " ".join(names[w] for w in words) if spoken else ""
        per_frame = np.float32(weight) / np.float32(bs.num_frames(u)) if spoken else np.float32(0.0)
        want.append(pk.Result(text, words, weight, ok, float(per_frame), dec.word_segments(u)))
        fbank.append(bs.fetch_fbank(u))
    assert [r.words for r in want] == [[2, 3], [3]] and all(r.text and r.ok == 1 for r in want)     # (the docstring's)
    assert all(f.shape[1] == D for f in fbank)
    names.close()
    for o in (dec, bs, am):
        o.close()
    return conf, waves, want, fbank


def test_recognizer_process_and_process_features(setup):
    conf, waves, want, fbank = setup
    rec = pk.Recognizer(conf, max_utts=2, max_total_samples=sum(len(w) for w in waves), trace_capacity=TRACE, frontend=SPEC)
    assert rec.am.feat_dim() == D and rec.batch.feat_dim() == D
    got = rec.process(waves)
    for u in range(2):
        assert comparable(got[u]) == comparable(want[u]), u
    for u in range(2):
        assert np.array_equal(rec.batch.fetch_fbank(u).view(np.uint32), fbank[u].view(np.uint32)), u
    got = rec.process_features(fbank, "raw")
    for u in range(2):
        assert comparable(got[u]) == comparable(want[u]), ("raw", u)
    got = rec.process(list(reversed(waves)))                 # and audio again on the same object
    for u in range(2):
        assert comparable(got[u]) == comparable(want[1 - u]), ("again", u)
    with pytest.raises(pk.PkCodeError) as e:                 # [T][40] matrices are not this model's
        rec.process_features([np.zeros((5, 40), np.float32)], "raw")
    assert e.value.code == E_INVALID
    rec.close()


def stream(online, waves, chunk=1600):
    """Wave u into slot u, `chunk` samples a step, closed with its last chunk -> the Results."""
    pos, live, out = [0] * len(waves), set(range(len(waves))), {}
    for u in live:
        online.open(u)
    while live:
        closing = []
        for u in sorted(live):
            online.push(u, waves[u][pos[u]:pos[u] + chunk])
            pos[u] += chunk
            if pos[u] >= len(waves[u]):
                online.close(u)
                closing.append(u)
        online.step()
        for u in closing:
            assert online.finished(u)
            out[u] = online.result(u)
            live.discard(u)
    return [out[u] for u in range(len(waves))]


def test_online_recognizer_in_100_ms_chunks(setup):
    conf, waves, want, fbank = setup
    online = pk.OnlineRecognizer(conf, max_streams=2, max_step_samples=2 * 1600, trace_capacity=TRACE, frontend=SPEC)
    assert online.scorer.feat_dim() == D
    got = stream(online, waves)
    for u in range(2):
        assert comparable(got[u]) == comparable(want[u]), u
        assert got[u].segments and all(np.isfinite(s.acoustic_cost) for s in got[u].segments)
    online.decoder.set_commit(True)                          # commit mode: the same Results
    got = stream(online, waves)
    for u in range(2):
        assert comparable(got[u]) == comparable(want[u]), ("commit", u)
    # features into the same object: the batch object's fbank rows as RAW frames, ten a step
    for u in range(2):
        online.open_features(u, "raw")
    pos, live = [0, 0], {0, 1}
    while live:
        for u in sorted(live):
            online.push_features(u, fbank[u][pos[u]:pos[u] + 10])
            pos[u] += 10
            if pos[u] >= fbank[u].shape[0]:
                online.close(u)
        online.step()
        live = {u for u in live if pos[u] < fbank[u].shape[0]}
    for u in range(2):
        assert comparable(online.result(u)) == comparable(want[u]), ("raw features", u)
    online.destroy()


def test_online_recognizer_with_endpointing_on(setup):
    """Endpointing on, with rules that cannot fire on half a second of audio (five seconds of trailing silence, or twenty
    seconds of utterance): the endpoint records are computed after every advance, nothing is cut, and each slot's one
    utterance -- rule 0, the stream's end -- is the batch Result."""
    conf, waves, want, _ = setup
    online = pk.OnlineRecognizer(conf, max_streams=2, max_step_samples=2 * 1600, trace_capacity=TRACE, frontend=SPEC)
    online.set_endpointing([10], [pk.EndpointRule(True, 5.0, np.inf, 0.0), pk.EndpointRule(False, 0.0, np.inf, 20.0)])
    online.decoder.set_commit(True)
    got = stream(online, waves)
    for u in range(2):
        assert comparable(got[u]) == comparable(want[u]), u
        pieces = online.utterances(u)
        assert [(p.first_frame, p.num_frames, p.rule) for p in pieces] == [(0, pk.num_frames(len(waves[u])), 0)]
        assert comparable(pieces[0].result) == comparable(want[u])
    online.destroy()


def test_command_line_in_a_child_process(setup, tmp_path):
    conf, waves, want, fbank = setup
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    listing = str(tmp_path / "waves.scp")
    with open(listing, "w") as f:
        f.write(HELLO + "\n" + CAT + "\n")
    lines = "".join("%s\t%s\t%f\n" % (name, r.text, r.loglikelihood_per_frame) for name, r in zip((HELLO, CAT), want))
    tool = [sys.executable, "-m", "pocketkaldi_amd.recognize", conf, listing, "--frontend", SPEC_TEXT]
    for extra in ([], ["--online"]):
        run = subprocess.run(tool + extra, capture_output=True, text=True, env=env)
        assert run.returncode == 0, run.stdout + run.stderr
        assert run.stdout == lines, extra


def test_command_line_flags_in_this_process(setup, tmp_path, capsys):
    """--frontend beside the flags that exist, through recognize.main (the child-process test above pins the entry)."""
    from pocketkaldi_amd import recognize
    conf, waves, want, fbank = setup
    front = ["--frontend", SPEC_TEXT]
    plain = "%s\t%s\t%f\n" % (HELLO, want[0].text, want[0].loglikelihood_per_frame)
    ctm = "".join("%s 1 %.2f %.2f %s\n" % (HELLO, s.start_frame * 0.01, s.num_frames * 0.01, want[0].text.split(" ")[i])
                  for i, s in enumerate(s for s in want[0].segments if s.word != 0))
    assert recognize.main([conf, HELLO] + front) == 0
    assert capsys.readouterr().out == plain
    assert recognize.main([conf, HELLO, "--ctm", "--channel", "0"] + front) == 0
    assert capsys.readouterr().out == ctm
    assert recognize.main([conf, HELLO, "--online", "--ctm", "--partials", "--commit", "--chunk-ms", "130"] + front) == 0
    out = capsys.readouterr()
    assert out.out == ctm
    assert recognize.main([conf, HELLO, "--online", "--endpoint-silence", "10", "--endpoint-rule", "1,5.0,inf,0"] + front) == 0
    frames = pk.num_frames(len(waves[0]))
    assert capsys.readouterr().out == "%s[0.00-%.2f]\t%s\t%f\n" % (HELLO, frames * 0.01, want[0].text, want[0].loglikelihood_per_frame)
    feats = str(tmp_path / "hello.npy")
    np.save(feats, fbank[0])
    for extra in ([], ["--online"]):
        assert recognize.main([conf, feats, "--features", "raw"] + extra + front) == 0
        assert capsys.readouterr().out == plain.replace(HELLO, feats)
    assert recognize.main([conf, HELLO]) == 1                # without --frontend: the reference's model file is expected
    assert "41 expected" in capsys.readouterr().out


def test_a_wrong_spec_dimension_is_refused_with_both_numbers(setup):
    conf = setup[0]
    for cls in (pk.Recognizer, pk.OnlineRecognizer):
        with pytest.raises(pk.PkCodeError) as e:
            cls(conf, frontend=FA.BATCH_SPECS[13])
        assert e.value.code == E_INVALID and "13" in str(e.value) and "80" in str(e.value), str(e.value)
        with pytest.raises(pk.PkCodeError) as e:             # 40 features of 40 bins: still not this model's 80
            cls(conf, frontend=FA.BATCH_SPECS[40])
        assert e.value.code == E_INVALID and "40-dim" in str(e.value) and "80" in str(e.value), str(e.value)
