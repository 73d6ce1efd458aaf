"""The batch recognizer and the command line with a feature transform, on a model file written
into tmp_path (tests/refmodel_files.py) beside the fixture's word-loop graph and word list: a 40-dim model behind a
13-of-23 MFCC, +-3 frames and a 91 -> 40 affine matrix.  The model file's cmvn_stats are at the front-end's dimension.
The yardstick is pk.Decoder.decode_batch over pk.BatchScorer(frontend=, transform=) -- what tests/test_gpu_transforms.py
pins -- field for field, floats by their bits; the command line's lines are those Results'.  The Kaldi matrix files the
command line reads are written here with struct.  Also tests/cpp/transforms_example.cc against Python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import recognize

import norm_cases as NC
import refmodel_files as RF
import transform_cases as XC
from refmodel_text import load_text_model
from test_cpp_ark_features import fnv, weight
from test_cpp_stream import build
from test_gpu_frontend_recognizer import CAT, DIR, HELLO, TRACE, comparable
from test_gpu_recognize_deltas import model_layers
from test_gpu_recognize_norm import lines_of

pytestmark = pytest.mark.gpu

E_INVALID, E_IO = -1, -3
L, R = 2, 1
CTX, Db, D = 3, 13, 40
FILES = [HELLO, CAT, HELLO, CAT, HELLO]
FRONT_TEXT = "kind=mfcc,num_mel_bins=23,num_ceps=13,window=povey,low_freq=20,high_freq=-400,cepstral_lifter=22"
NORM = pk.NormSpec("utterance", True, True)
CMVN = ["--cmvn", "mode=utterance,norm_vars=true"]


def kaldi_matrix(m):
    m = np.ascontiguousarray(m, "<f4")
    return b"\0BFM " + struct.pack("<bi", 4, m.shape[0]) + struct.pack("<bi", 4, m.shape[1]) + m.tobytes()


def yardstick(am, fe, stats, waves, spec, mats=None):
    """Results of one unsplit call through BatchScorer + Decoder, the front-end's rows and the first layer's."""
    bs = pk.BatchScorer(am, stats, len(waves), sum(len(w) for w in waves), frontend=fe, transform=spec)
    bs.set_norm(NORM)
    bs.set_waves(waves)
    if mats is not None:
        bs.set_utt_transforms(mats)
    bs.score(0.1)
    fst = pk.Fst(os.path.join(DIR, "wordloop.fst"))
    dec = pk.Decoder(fst, am, len(waves), trace_capacity=TRACE)
    dec.set_alignment(True)
    dec.decode_batch(bs)
    names = pk.SymbolTable(os.path.join(DIR, "wordloop_words.bin"))
    out, rows, ready = [], [], []
    for u in range(len(waves)):
        words, weight_, ok = dec.result(u)
        spoken = bool(ok and words)
        text = " ".join(names[w] for w in words) if spoken else ""
        per_frame = np.float32(weight_) / np.float32(bs.num_frames(u)) if spoken else np.float32(0.0)
        out.append(pk.Result(text, words, weight_, ok, float(per_frame), dec.word_segments(u)))
        rows.append(bs.fetch_fbank(u))
        ready.append(bs.fetch_cmvn(u))
    names.close()
    for o in (dec, bs):
        o.close()
    return out, rows, ready


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recognize_transforms")
    fe = pk.parse_frontend(FRONT_TEXT)
    assert fe.dim == Db
    stats = np.concatenate([np.full(Db, 0.5 * 2500.0), [2500.0]]).astype(np.float32)
    layers, prior = model_layers(D, 25)
    tid2pdf = load_text_model()[4]
    conf = RF.write_model(tmp, layers, prior, L, R, tid2pdf=tid2pdf, cmvn_stats=stats)
    for f in ("wordloop.fst", "wordloop_words.bin"):
        shutil.copy(os.path.join(DIR, f), str(tmp / f))
    with open(conf, "a") as f:
        f.write("fst = wordloop.fst\nsymbol_table = wordloop_words.bin\n")
    m = XC.matrix(Db, CTX, CTX, D, True)
    final_mat = str(tmp / "final.mat")
    with open(final_mat, "wb") as f:
        f.write(kaldi_matrix(m))
    spec = pk.TransformSpec(m, CTX, CTX)
    by_speaker = {"hello": np.eye(D, D + 1, dtype=np.float32) + 0.2 * XC.matrix(D, 0, 0, D, True, seed=61),
                  "cat": np.eye(D, D + 1, dtype=np.float32) + 0.2 * XC.matrix(D, 0, 0, D, True, seed=62)}
    speakers = ["hello" if f == HELLO else "cat" for f in FILES]
    mats = [by_speaker[s] for s in speakers]
    by_file = {HELLO: pk.read_wav(HELLO), CAT: pk.read_wav(CAT)}
    waves = [by_file[f] for f in FILES]
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    want, rows, ready = yardstick(am, fe, stats, waves, spec)
    want_utt, _, ready_utt = yardstick(am, fe, stats, waves, spec, mats)
    am.close()
    for u in range(len(FILES)):                                                   # the rows are the restatement's
        base = XC.transform(NC.normalize(rows[u], "utterance", True, True)[0], m, CTX, CTX)
        assert NC.bits_equal(ready[u], base) and NC.bits_equal(ready_utt[u], XC.transform(base, mats[u], 0, 0)), u
    print("hypotheses: %s / with per-utterance matrices: %s" % ([r.text for r in want], [r.text for r in want_utt]))
    return dict(conf=conf, fe=fe, spec=spec, final_mat=final_mat, waves=waves, rows=rows, ready=ready, want=want, want_utt=want_utt, mats=mats,
                by_speaker=by_speaker, speakers=speakers, tmp=tmp)


def test_recognizer_split_over_two_utterances_equals_one_call(setup):
    s = setup
    total = sum(len(w) for w in s["waves"])
    for max_utts in (5, 2):                                                       # one call; three calls of 2, 2 and 1
        rec = pk.Recognizer(s["conf"], max_utts=max_utts, max_total_samples=total, trace_capacity=TRACE, frontend=s["fe"], transform=s["spec"])
        rec.batch.set_norm(NORM)
        assert (rec.batch.in_dim(), rec.batch.base_dim(), rec.batch.feat_dim()) == (Db, Db, D)
        got = rec.process(s["waves"])
        assert [comparable(r) for r in got] == [comparable(r) for r in s["want"]], max_utts
        got = rec.process(s["waves"], utt_transforms=s["mats"])                   # split with the list
        assert [comparable(r) for r in got] == [comparable(r) for r in s["want_utt"]], ("utt", max_utts)
        got = rec.process(s["waves"])                                             # consumed: the stage does not run again
        assert [comparable(r) for r in got] == [comparable(r) for r in s["want"]], ("after", max_utts)
        got = rec.process_features(s["rows"], "raw", utt_transforms=s["mats"])
        assert [comparable(r) for r in got] == [comparable(r) for r in s["want_utt"]], ("raw", max_utts)
        got = rec.process_features(s["ready"], "normalized")                      # [T][D]: ready for the splice
        assert [comparable(r) for r in got] == [comparable(r) for r in s["want"]], ("normalized", max_utts)
        with pytest.raises(pk.PkCodeError):                                       # raw rows at the model's dimension
            rec.process_features(s["ready"], "raw")
        with pytest.raises(pk.PkCodeError, match="4 per-utterance transforms for 5"):
            rec.process(s["waves"], utt_transforms=s["mats"][:4])
        rec.close()


def test_load_refusals(setup):
    s = setup
    with pytest.raises(pk.PkCodeError) as e:                                      # the model file's statistics are at Db, not at D
        pk.Recognizer(s["conf"], frontend=s["fe"])
    assert e.value.code in (E_INVALID, E_IO) and str(Db + 1) in str(e.value) and str(D + 1) in str(e.value)
    with pytest.raises(pk.PkCodeError) as e:
        pk.Recognizer(s["conf"], frontend=s["fe"], transform=pk.TransformSpec(s["spec"].matrix, CTX, CTX + 1, in_dim=Db))
    assert e.value.code == E_INVALID and "cols 92" in str(e.value)
    with pytest.raises(pk.PkCodeError) as e:                                      # a transform of another output dimension
        pk.Recognizer(s["conf"], frontend=s["fe"], transform=pk.TransformSpec(XC.matrix(Db, CTX, CTX, 39, True), CTX, CTX))
    assert e.value.code == E_INVALID and "39" in str(e.value) and "40" in str(e.value)
    with pytest.raises(pk.PkCodeError) as e:                                      # the reference's 40-bin front-end in front of 13
        pk.Recognizer(s["conf"], transform=s["spec"])
    assert e.value.code == E_INVALID and "40" in str(e.value) and "13" in str(e.value)
    for cls in (pk.OnlineScorer, pk.OnlineFeatureScorer, pk.OnlineRecognizer):    # the live objects take no transform
        with pytest.raises(TypeError):
            cls(None, None, 1, 1, transform=s["spec"])


def test_command_line(setup, capsys):
    s = setup
    conf, tmp, want, want_utt = s["conf"], s["tmp"], s["want"], s["want_utt"]
    flags = ["--frontend", FRONT_TEXT, "--transform", "matrix=%s,left_context=%d,right_context=%d" % (s["final_mat"], CTX, CTX)] + CMVN
    listing = str(tmp / "waves.scp")
    with open(listing, "w") as f:
        f.write("\n".join(FILES[:2]) + "\n")
    # a wave file and a list
    assert recognize.main([conf, HELLO] + flags) == 0
    assert capsys.readouterr().out == lines_of([HELLO], want[:1])
    assert recognize.main([conf, listing] + flags) == 0
    assert capsys.readouterr().out == lines_of(FILES[:2], want[:2])
    # per-utterance matrices keyed by utterance, and by speaker with --utt2spk
    by_utt = str(tmp / "trans_utt.ark")
    with open(by_utt, "wb") as f:
        for k, m in zip(FILES[:2], s["mats"][:2]):
            f.write(k.encode() + b" " + kaldi_matrix(m))
    assert recognize.main([conf, listing] + flags + ["--utt-transforms", "ark:" + by_utt]) == 0
    assert capsys.readouterr().out == lines_of(FILES[:2], want_utt[:2])
    by_spk = str(tmp / "trans_spk.ark")
    with open(by_spk, "wb") as f:
        for k, m in s["by_speaker"].items():
            f.write(k.encode() + b" " + kaldi_matrix(m))
    keys = ["utt%d" % u for u in range(len(FILES))]
    utt2spk = str(tmp / "utt2spk")
    with open(utt2spk, "w") as f:
        f.write("".join("%s %s\n" % (k, sp) for k, sp in zip(keys + FILES[:2], s["speakers"] + s["speakers"][:2])))
    assert recognize.main([conf, listing] + flags + ["--utt-transforms", "ark:" + by_spk, "--utt2spk", utt2spk]) == 0
    assert capsys.readouterr().out == lines_of(FILES[:2], want_utt[:2])
    # an .npz and an archive of the front-end's rows; an .npz of rows that are ready for the splice
    npz = str(tmp / "feats.npz")
    np.savez(npz, hello=s["rows"][0], cat=s["rows"][1])
    assert recognize.main([conf, npz, "--features", "raw"] + flags) == 0
    assert capsys.readouterr().out == lines_of(["hello", "cat"], want[:2])
    assert recognize.main([conf, npz, "--features", "raw"] + flags + ["--utt-transforms", "ark:" + by_spk]) == 0      # the arrays' names are the speakers'
    assert capsys.readouterr().out == lines_of(["hello", "cat"], want_utt[:2])
    ark = str(tmp / "feats.ark")
    with open(ark, "wb") as f:
        for k, r in zip(keys, s["rows"]):
            f.write(k.encode() + b" " + kaldi_matrix(r))
    assert recognize.main([conf, "ark:" + ark, "--features", "raw"] + flags + ["--utt-transforms", "ark:" + by_spk, "--utt2spk", utt2spk]) == 0
    assert capsys.readouterr().out == lines_of(keys, want_utt)
    ready = str(tmp / "ready.npz")
    np.savez(ready, hello=s["ready"][0], cat=s["ready"][1])
    assert recognize.main([conf, ready, "--features", "normalized"] + flags) == 0
    assert capsys.readouterr().out == lines_of(["hello", "cat"], want[:2])
    # a missing key is a usage error that names it; so are the live objects
    assert recognize.main([conf, "ark:" + ark, "--features", "raw"] + flags + ["--utt-transforms", "ark:" + by_spk]) == 1
    out = capsys.readouterr().out
    assert "--utt-transforms: no transform for utterance 'utt0'" in out and "Usage:" in out
    short = str(tmp / "utt2spk_short")
    with open(short, "w") as f:
        f.write("utt0 hello\nutt1 nobody\n")
    assert recognize.main([conf, "ark:" + ark, "--features", "raw"] + flags + ["--utt-transforms", "ark:" + by_spk, "--utt2spk", short]) == 1
    out = capsys.readouterr().out
    assert "--utt-transforms: no transform for speaker 'nobody'" in out and "Usage:" in out
    for extra in (["--utt-transforms", "ark:" + by_utt], []):
        assert recognize.main([conf, HELLO, "--online"] + flags[:4] + extra) == 1
        out = capsys.readouterr().out
        assert "the live objects do not have transforms yet" in out and "Usage:" in out
    # without --transform the model file does not fit its front-end
    assert recognize.main([conf, HELLO, "--frontend", FRONT_TEXT]) == 1
    out = capsys.readouterr().out
    assert "pocketkaldi:" in out and "Usage:" not in out


def test_transforms_example_equals_python():
    N = 16
    got = subprocess.run([build("transforms_example"), HELLO], capture_output=True, text=True)
    assert got.returncode == 0 and "transforms_example ok" in got.stdout, got.stdout + got.stderr
    fe = pk.FrontendSpec("mfcc", 23, 13, "povey", 20.0, 0.0, 22.0)
    K = (2 * CTX + 1) * Db
    m = (np.float32(20.0) * weight(5000011 + np.arange(D * (K + 1)))).reshape(D, K + 1)
    mu = (np.float32(20.0) * weight(7000003 + np.arange(D * (D + 1)))).reshape(D, D + 1) + np.eye(D, D + 1, dtype=np.float32)
    W = weight(np.arange(N * D * (L + R + 1))).reshape(N, D * (L + R + 1))
    b = weight(1000003 + np.arange(N))
    am = pk.AcousticModel([("linear", W, b), ("softmax",)], np.full(N, 1.0 / N, np.float32), L, R)
    g = np.zeros(Db + 1, np.float32)
    g[Db] = 1.0
    wave = pk.read_wav(HELLO)
    bs = pk.BatchScorer(am, g, 1, wave.shape[0] + 1, frontend=fe, transform=pk.TransformSpec(m, CTX, CTX))
    bs.set_norm(NORM)
    bs.set_waves([wave])
    bs.set_utt_transforms([mu])
    bs.score(0.1)
    rows = bs.fetch_fbank(0)
    want = XC.transform(XC.transform(NC.normalize(rows, "utterance", True, True)[0], m, CTX, CTX), mu, 0, 0)
    assert NC.bits_equal(bs.fetch_cmvn(0), want)
    lines = ["frames %d base %d dim %d" % (rows.shape[0], Db, D), "features %s" % fnv(rows.tobytes()), "transformed %s" % fnv(want.tobytes()),
             "loglik %s" % fnv(bs.fetch(0).log_prob().tobytes())]
    assert got.stdout.splitlines()[:4] == lines
    bs.close()
    am.close()
