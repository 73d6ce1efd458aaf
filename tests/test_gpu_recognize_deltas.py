"""The batch recognizer and the command line with deltas, on two model files written into tmp_path
(tests/refmodel_files.py) beside the fixture's word-loop graph and word list: a 39-dim model behind a 13-of-23 MFCC with
deltas and double deltas, and a 120-dim one behind the reference's 40-bin fbank.  The model file's cmvn_stats are at the
front-end's dimension.  The yardstick is pk.Decoder.decode_batch over pk.BatchScorer(frontend=, deltas=) -- what
tests/test_gpu_deltas.py pins -- field for field, floats by their bits; the command line's lines are those Results'."""
import os
import shutil

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import recognize

import norm_cases as NC
import refmodel_files as RF
from refmodel_text import load_text_model
from test_gpu_frontend_recognizer import CAT, DIR, HELLO, TRACE, comparable
from test_gpu_recognize_norm import binary_matrix, lines_of

pytestmark = pytest.mark.gpu

E_INVALID, E_IO = -1, -3
L, R, HIDDEN, PDFS = 2, 1, 64, 18
FILES = [HELLO, CAT, HELLO, CAT, HELLO]
DELTAS_TEXT = "order=2,window=2"
MODELS = {
    "mfcc39": "kind=mfcc,num_mel_bins=23,num_ceps=13,window=povey,low_freq=20,high_freq=-400,cepstral_lifter=22",
    "fbank120": None,                                    # the reference's front-end: no --frontend
}


def model_layers(D, seed):
    rng = np.random.default_rng([0xDE17A, seed])
    dims = [D * (L + R + 1), HIDDEN, HIDDEN, PDFS]
    layers = []
    for i in range(3):
        W = (rng.standard_normal((dims[i + 1], dims[i])) * np.sqrt(2.0 / dims[i])).astype(np.float32)
        layers += [("linear", W, (rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32)), ("relu",) if i < 2 else ("softmax",)]
    return layers, np.full(PDFS, 1.0 / PDFS, np.float32)


def yardstick(am, fe, stats, waves, norm=None, speaker_stats=None):
    """Results of one unsplit call through BatchScorer + Decoder, and the front-end's rows."""
    bs = pk.BatchScorer(am, stats, len(waves), sum(len(w) for w in waves), frontend=fe, deltas=pk.DeltaSpec())
    if norm is not None:
        bs.set_norm(norm)
    if speaker_stats is not None:
        bs.set_speaker_stats(speaker_stats)
    bs.set_waves(waves)
    bs.score(0.1)
    fst = pk.Fst(os.path.join(DIR, "wordloop.fst"))
    dec = pk.Decoder(fst, am, len(waves), trace_capacity=TRACE)
    dec.set_alignment(True)
    dec.decode_batch(bs)
    names = pk.SymbolTable(os.path.join(DIR, "wordloop_words.bin"))
    out, rows, deltas = [], [], []
    for u in range(len(waves)):
        words, weight, ok = dec.result(u)
        spoken = bool(ok and words)
        text = " ".join(names[w] for w in words) if spoken else ""
        per_frame = np.float32(weight) / np.float32(bs.num_frames(u)) if spoken else np.float32(0.0)
        out.append(pk.Result(text, words, weight, ok, float(per_frame), dec.word_segments(u)))
        rows.append(bs.fetch_fbank(u))
        deltas.append(bs.fetch_cmvn(u))
    names.close()
    for o in (dec, bs):
        o.close()
    return out, rows, deltas


@pytest.fixture(scope="module", params=sorted(MODELS))
def setup(request, tmp_path_factory):
    name = request.param
    tmp = tmp_path_factory.mktemp("recognize_deltas_" + name)
    fe = pk.FrontendSpec() if MODELS[name] is None else pk.parse_frontend(MODELS[name])
    Db = fe.dim
    D = pk.DeltaSpec().dim(Db)
    stats = np.concatenate([np.full(Db, (12.0 if MODELS[name] is None else 0.5) * 2500.0), [2500.0]]).astype(np.float32)
    layers, prior = model_layers(D, len(name))
    tid2pdf = load_text_model()[4]
    conf = RF.write_model(tmp, layers, prior, L, R, tid2pdf=tid2pdf, cmvn_stats=stats)
    for f in ("wordloop.fst", "wordloop_words.bin"):
        shutil.copy(os.path.join(DIR, f), str(tmp / f))
    with open(conf, "a") as f:
        f.write("fst = wordloop.fst\nsymbol_table = wordloop_words.bin\n")
    by_file = {HELLO: pk.read_wav(HELLO), CAT: pk.read_wav(CAT)}
    waves = [by_file[f] for f in FILES]
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    want = {}
    want["sliding"], rows, deltas = yardstick(am, fe, stats, waves)
    want["none"], _, _ = yardstick(am, fe, stats, waves, pk.NormSpec("none"))
    want["utterance"], _, _ = yardstick(am, fe, stats, waves, pk.NormSpec("utterance", True, True))
    rec = [NC.accumulate(r) for r in rows]
    spk = [r + rec[1] for r in rec]
    want["speaker"], _, _ = yardstick(am, fe, stats, waves, pk.NormSpec("speaker", True, True), spk)
    want["online"], _, _ = yardstick(am, fe, stats, waves, pk.OnlineCmvnSpec(8, 600, 0, True))
    am.close()
    assert all(r.shape[1] == Db for r in rows) and all(d.shape[1] == D for d in deltas)
    print("%s hypotheses: %s" % (name, {k: [r.text for r in v] for k, v in want.items()}))
    front = [] if MODELS[name] is None else ["--frontend", MODELS[name]]
    return dict(name=name, conf=conf, fe=fe, front=front, waves=waves, rows=rows, deltas=deltas, want=want, spk=spk, Db=Db, D=D, tmp=tmp)


def test_recognizer_split_over_two_utterances_equals_one_call(setup):
    s = setup
    total = sum(len(w) for w in s["waves"])
    for max_utts in (5, 2):                                                       # one call; three calls of 2, 2 and 1
        rec = pk.Recognizer(s["conf"], max_utts=max_utts, max_total_samples=total, trace_capacity=TRACE,
                            frontend=None if s["name"] == "fbank120" else s["fe"], deltas=pk.DeltaSpec())
        assert (rec.batch.base_dim(), rec.batch.feat_dim()) == (s["Db"], s["D"])
        got = rec.process(s["waves"])
        assert [comparable(r) for r in got] == [comparable(r) for r in s["want"]["sliding"]], max_utts
        got = rec.process_features(s["rows"], "raw")                              # [T][Db]: the deltas are added behind the norm
        assert [comparable(r) for r in got] == [comparable(r) for r in s["want"]["sliding"]], ("raw", max_utts)
        got = rec.process_features(s["deltas"], "normalized")                     # [T][D]: ready for the splice
        assert [comparable(r) for r in got] == [comparable(r) for r in s["want"]["sliding"]], ("normalized", max_utts)
        rec.batch.set_norm(pk.NormSpec("speaker", True, True))
        got = rec.process(s["waves"], speaker_stats=s["spk"])
        assert [comparable(r) for r in got] == [comparable(r) for r in s["want"]["speaker"]], ("speaker", max_utts)
        with pytest.raises(pk.PkCodeError):                                       # raw rows at the model's dimension
            rec.process_features(s["deltas"], "raw")
        rec.close()


def test_load_refusals(setup, tmp_path):
    s = setup
    with pytest.raises(pk.PkCodeError) as e:                                      # the model file's statistics are at Db, not at D
        pk.Recognizer(s["conf"], frontend=s["fe"])
    assert e.value.code in (E_INVALID, E_IO) and str(s["Db"] + 1) in str(e.value) and str(s["D"] + 1) in str(e.value)
    with pytest.raises(pk.PkCodeError) as e:                                      # order 1: statistics for D / 2 (or D odd)
        pk.Recognizer(s["conf"], frontend=s["fe"], deltas=pk.DeltaSpec(1, 2))
    assert e.value.code in (E_INVALID, E_IO)
    with pytest.raises(pk.PkCodeError) as e:
        pk.Recognizer(s["conf"], frontend=s["fe"], deltas=pk.DeltaSpec(2, 9))
    assert e.value.code == E_INVALID and "window" in str(e.value)


def test_command_line(setup, capsys):
    s = setup
    conf, want, tmp = s["conf"], s["want"], s["tmp"]
    flags = s["front"] + ["--deltas", DELTAS_TEXT]
    listing = str(tmp / "waves.scp")
    with open(listing, "w") as f:
        f.write("\n".join(FILES[:2]) + "\n")
    keys = ["utt%d" % u for u in range(len(FILES))]
    by_utt = str(tmp / "by_utt.ark")
    with open(by_utt, "wb") as f:
        for k, r in zip(FILES[:2], s["spk"][:2]):
            f.write(k.encode() + b" " + binary_matrix(r))
    # a wave file and a list under every CMVN mode
    modes = {"sliding": [], "none": ["--cmvn", "mode=none"], "utterance": ["--cmvn", "mode=utterance,norm_vars=true"],
             "online": ["--cmvn", "mode=online,cmn_window=8,speaker_frames=600,global_frames=0,norm_vars=true"],
             "speaker": ["--cmvn", "mode=speaker,norm_vars=true", "--cmvn-stats", "ark:" + by_utt]}
    for mode, cmvn in modes.items():
        assert recognize.main([conf, HELLO] + flags + cmvn) == 0, mode
        assert capsys.readouterr().out == lines_of([HELLO], want[mode][:1]), mode
        assert recognize.main([conf, listing] + flags + cmvn) == 0, mode
        assert capsys.readouterr().out == lines_of(FILES[:2], want[mode][:2]), mode
    # an .npz and an archive of the front-end's rows; an .npz of rows that are ready for the splice
    cmvn = modes["utterance"]
    npz = str(tmp / "feats.npz")
    np.savez(npz, hello=s["rows"][0], cat=s["rows"][1])
    assert recognize.main([conf, npz, "--features", "raw"] + flags + cmvn) == 0
    assert capsys.readouterr().out == lines_of(["hello", "cat"], want["utterance"][:2])
    ark = str(tmp / "feats.ark")
    with open(ark, "wb") as f:
        for k, r in zip(keys, s["rows"]):
            f.write(k.encode() + b" " + binary_matrix(r, "FM"))
    assert recognize.main([conf, "ark:" + ark, "--features", "raw"] + flags + cmvn) == 0
    assert capsys.readouterr().out == lines_of(keys, want["utterance"])
    ready = str(tmp / "ready.npz")
    np.savez(ready, hello=s["deltas"][0], cat=s["deltas"][1])
    assert recognize.main([conf, ready, "--features", "normalized"] + flags) == 0
    assert capsys.readouterr().out == lines_of(["hello", "cat"], want["sliding"][:2])
    # without --deltas the model file does not fit its front-end
    assert recognize.main([conf, HELLO] + s["front"]) == 1
    out = capsys.readouterr().out
    assert "pocketkaldi:" in out and "Usage:" not in out and str(s["D"]) in out
