"""The batch recognizer and the command line with a normalisation spec, on the 80-dim model file of
tests/test_gpu_frontend_recognizer.py.  The norm is set on Recognizer.batch; speaker statistics travel with process /
process_features and are split with a list that does not fit max_utts.  The yardstick is pk.Decoder.decode_batch over
pk.BatchScorer(frontend=spec) with the same spec set -- what tests/test_gpu_norm.py pins -- field for field, floats by
their bits; the command line's lines are those Results'."""
import os
import shutil
import struct

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import recognize

import norm_cases as NC
import refmodel_files as RF
from refmodel_text import load_text_model
from test_gpu_frontend_recognizer import CAT, D, DIR, HELLO, L, R, SPEC, SPEC_TEXT, STATS, TRACE, comparable, model_layers

pytestmark = pytest.mark.gpu

E_STATE = -4
FILES = [HELLO, CAT, HELLO, CAT, HELLO]
SPEAKERS = ["ann", "bob", "ann", "cy", "bob"]


def binary_matrix(m, token="DM"):
    m = np.ascontiguousarray(m, {"DM": "<f8", "FM": "<f4"}[token])
    return b"\0B" + token.encode() + b" " + struct.pack("<bi", 4, m.shape[0]) + struct.pack("<bi", 4, m.shape[1]) + m.tobytes()


def yardstick(am, waves, spec, speaker_stats=None):
    """Results of one unsplit call through BatchScorer + Decoder, and the front-end's rows."""
    bs = pk.BatchScorer(am, STATS, len(waves), sum(len(w) for w in waves), frontend=SPEC)
    bs.set_norm(spec)
    if speaker_stats is not None:
        bs.set_speaker_stats(speaker_stats)
    bs.set_waves(waves)
    bs.score(0.1)
    fst = pk.Fst(os.path.join(DIR, "wordloop.fst"))
    dec = pk.Decoder(fst, am, len(waves), trace_capacity=TRACE)
    dec.set_alignment(True)
    dec.decode_batch(bs)
    names = pk.SymbolTable(os.path.join(DIR, "wordloop_words.bin"))
    out, rows = [], []
    for u in range(len(waves)):
        words, weight, ok = dec.result(u)
        spoken = bool(ok and words)
        text = " ".join(names[w] for w in words) if spoken else ""
        per_frame = np.float32(weight) / np.float32(bs.num_frames(u)) if spoken else np.float32(0.0)
        out.append(pk.Result(text, words, weight, ok, float(per_frame), dec.word_segments(u)))
        rows.append(bs.fetch_fbank(u))
    names.close()
    for o in (dec, bs):
        o.close()
    return out, rows


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recognize_norm")
    layers, prior = model_layers()
    tid2pdf = load_text_model()[4]
    conf = RF.write_model(tmp, layers, prior, L, R, tid2pdf=tid2pdf, cmvn_stats=STATS)
    for name in ("wordloop.fst", "wordloop_words.bin"):
        shutil.copy(os.path.join(DIR, name), str(tmp / name))
    with open(conf, "a") as f:
        f.write("fst = wordloop.fst\nsymbol_table = wordloop_words.bin\n")
    by_file = {HELLO: pk.read_wav(HELLO), CAT: pk.read_wav(CAT)}
    waves = [by_file[f] for f in FILES]
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    utt = pk.NormSpec("utterance", True, True)
    want_utt, rows = yardstick(am, waves, utt)
    rec = [NC.accumulate(r) for r in rows]
    by_speaker = {s: sum(rec[u] * (1 + u) for u in range(len(FILES)) if SPEAKERS[u] == s) for s in set(SPEAKERS)}     # (distinct records)
    spk = [by_speaker[s] for s in SPEAKERS]
    want_spk, _ = yardstick(am, waves, pk.NormSpec("speaker", True, True), spk)
    am.close()
    print("hypotheses: utterance %r, speaker %r" % ([r.text for r in want_utt], [r.text for r in want_spk]))
    return conf, waves, rows, want_utt, want_spk, spk, by_speaker


def test_speaker_statistics_are_split_with_the_list(setup):
    conf, waves, rows, want_utt, want_spk, spk, _ = setup
    total = sum(len(w) for w in waves)
    for max_utts in (5, 2):                                                       # one call; three calls of 2, 2 and 1
        rec = pk.Recognizer(conf, max_utts=max_utts, max_total_samples=total, trace_capacity=TRACE, frontend=SPEC)
        rec.batch.set_norm(pk.NormSpec("speaker", True, True))
        got = rec.process(waves, speaker_stats=spk)
        assert [comparable(r) for r in got] == [comparable(r) for r in want_spk], max_utts
        got = rec.process_features(rows, "raw", speaker_stats=spk)
        assert [comparable(r) for r in got] == [comparable(r) for r in want_spk], ("features", max_utts)
        with pytest.raises(pk.PkCodeError) as e:                                  # mode speaker without records
            rec.process(waves)
        assert e.value.code == E_STATE
        with pytest.raises(pk.PkCodeError):                                       # four records for five waves
            rec.process(waves, speaker_stats=spk[:4])
        rec.batch.set_norm(pk.NormSpec("utterance", True, True))
        got = rec.process(waves)
        assert [comparable(r) for r in got] == [comparable(r) for r in want_utt], ("utterance", max_utts)
        rec.close()


def lines_of(names, results):
    return "".join("%s\t%s\t%f\n" % (n, r.text, r.loglikelihood_per_frame) for n, r in zip(names, results))


def test_command_line(setup, tmp_path, capsys):
    conf, waves, rows, want_utt, want_spk, spk, by_speaker = setup
    front = ["--frontend", SPEC_TEXT]
    listing = str(tmp_path / "waves.scp")
    with open(listing, "w") as f:
        f.write("\n".join(FILES[:2]) + "\n")
    # per utterance, with variance: wave files, a list, an .npz and an archive of the front-end's rows
    cmvn = ["--cmvn", "mode=utterance,norm_vars=true"]
    assert recognize.main([conf, HELLO] + front + cmvn) == 0
    assert capsys.readouterr().out == lines_of([HELLO], want_utt[:1])
    assert recognize.main([conf, listing] + front + cmvn) == 0
    assert capsys.readouterr().out == lines_of(FILES[:2], want_utt[:2])
    npz = str(tmp_path / "feats.npz")
    np.savez(npz, hello=rows[0], cat=rows[1])
    assert recognize.main([conf, npz, "--features", "raw"] + front + cmvn) == 0
    assert capsys.readouterr().out == lines_of(["hello", "cat"], want_utt[:2])
    ark = str(tmp_path / "feats.ark")
    keys = ["utt%d" % u for u in range(len(FILES))]
    with open(ark, "wb") as f:
        for k, r in zip(keys, rows):
            f.write(k.encode() + b" " + binary_matrix(r, "FM"))
    assert recognize.main([conf, "ark:" + ark, "--features", "raw"] + front + cmvn) == 0
    assert capsys.readouterr().out == lines_of(keys, want_utt)
    # per speaker: statistics by utterance key, and by speaker through --utt2spk
    by_utt = str(tmp_path / "by_utt.ark")
    with open(by_utt, "wb") as f:
        for k, s in zip(keys, spk):
            f.write(k.encode() + b" " + binary_matrix(s))
    speaker = ["--cmvn", "mode=speaker,norm_vars=true"]
    assert recognize.main([conf, "ark:" + ark, "--features", "raw", "--cmvn-stats", "ark:" + by_utt] + front + speaker) == 0
    assert capsys.readouterr().out == lines_of(keys, want_spk)
    by_spk = str(tmp_path / "by_spk.ark")
    with open(by_spk, "wb") as f:
        for s in sorted(by_speaker):
            f.write(s.encode() + b" " + binary_matrix(by_speaker[s]))
    utt2spk = str(tmp_path / "utt2spk")
    with open(utt2spk, "w") as f:
        f.write("".join("%s %s\n" % (k, s) for k, s in zip(keys, SPEAKERS)))
    assert recognize.main([conf, ark, "--features", "raw", "--cmvn-stats", by_spk, "--utt2spk", utt2spk] + front + speaker) == 0
    assert capsys.readouterr().out == lines_of(keys, want_spk)
    wav2spk = str(tmp_path / "wav2spk")                                           # wave files: the printed key is the file's name
    with open(wav2spk, "w") as f:
        f.write("%s ann\n%s bob\n" % (HELLO, CAT))
    assert recognize.main([conf, listing, "--cmvn-stats", by_spk, "--utt2spk", wav2spk] + front + speaker) == 0
    assert capsys.readouterr().out == lines_of(FILES[:2], want_spk[:2])
    # a missing key is a usage error that names it
    assert recognize.main([conf, listing, "--cmvn-stats", by_spk] + front + speaker) == 1
    out = capsys.readouterr().out
    assert "Usage:" in out and "'%s'" % HELLO in out and "utterance" in out
    with open(wav2spk, "w") as f:
        f.write("%s ann\n%s dora\n" % (HELLO, CAT))
    assert recognize.main([conf, listing, "--cmvn-stats", by_spk, "--utt2spk", wav2spk] + front + speaker) == 1
    out = capsys.readouterr().out
    assert "Usage:" in out and "speaker 'dora'" in out
    # mode none and the sliding rule by name
    assert recognize.main([conf, HELLO, "--cmvn", "mode=sliding"] + front) == 0
    sliding = capsys.readouterr().out
    assert recognize.main([conf, HELLO] + front) == 0
    assert capsys.readouterr().out == sliding
