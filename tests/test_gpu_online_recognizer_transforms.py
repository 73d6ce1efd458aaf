"""The online recognizer and the online decoder behind a feature transform, on the model file of
tests/test_gpu_recognize_transforms.py: a 40-dim model behind a 13-of-23 MFCC, +-3 frames and a 91 -> 40 affine matrix,
cmvn_stats at the front-end's dimension, under the sliding-window CMVN.  The yardstick is pk.Recognizer(..., transform=)
on the whole waves -- text, weight bits, segments and their costs -- without and with per-utterance matrices
(utt_transforms= there, set_slot_transform here), and for the decoder alone Decoder.decode_batch over
BatchScorer(frontend=, transform=).  Also tests/cpp/online_transforms_example.cc against Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import refmodel_files as RF
import transform_cases as TC
from refmodel_text import load_text_model
from test_cpp_ark_features import fnv, weight
from test_cpp_stream import build
from test_gpu_frontend_recognizer import CAT, DIR, HELLO, TRACE, comparable
from test_gpu_recognize_deltas import model_layers

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, R = 2, 1
CTX, Db, D = 3, 13, 40
FRONT_TEXT = "kind=mfcc,num_mel_bins=23,num_ceps=13,window=povey,low_freq=20,high_freq=-400,cepstral_lifter=22"


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The model file, the waves, the front-end's rows of each and the batch recognizer's Results (computed once)."""
    tmp = tmp_path_factory.mktemp("online_recognizer_transforms")
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
    spec = pk.TransformSpec(TC.matrix(Db, CTX, CTX, D, True), CTX, CTX)
    mats = [np.eye(D, D + 1, dtype=np.float32) + 0.2 * TC.matrix(D, 0, 0, D, True, seed=61 + u) for u in range(2)]
    waves = [pk.read_wav(HELLO), pk.read_wav(CAT)]
    rec = pk.Recognizer(conf, max_utts=2, max_total_samples=sum(len(w) for w in waves), trace_capacity=TRACE, frontend=fe, transform=spec)
    want = rec.process(waves)
    rows = [rec.batch.fetch_fbank(u) for u in range(2)]
    want_utt = rec.process(waves, utt_transforms=mats)
    rec.close()
    assert [comparable(r) for r in want] != [comparable(r) for r in want_utt]      # the matrices matter
    return dict(conf=conf, fe=fe, spec=spec, stats=stats, waves=waves, rows=rows, want=want, want_utt=want_utt, mats=mats,
                model=(layers, prior, tid2pdf))


def online_of(s):
    return pk.OnlineRecognizer.with_transform(s["conf"], s["spec"], max_streams=2, max_step_samples=2 * 1600, trace_capacity=TRACE, frontend=s["fe"])


def stream(online, waves, chunk=1600, close_later=False, mats=None):
    """Wave u into slot u, `chunk` samples a step, closed with its last chunk or in a step of its own -> the Results."""
    pos, live, out = [0] * len(waves), set(range(len(waves))), {}
    for u in live:
        online.open(u)
        if mats is not None:
            online.scorer.set_slot_transform(u, mats[u])
    while live:
        closing = []
        for u in sorted(live):
            if pos[u] < len(waves[u]):
                online.push(u, waves[u][pos[u]:pos[u] + chunk])
                pos[u] += chunk
                if close_later:
                    continue
            if pos[u] >= len(waves[u]):
                online.close(u)
                closing.append(u)
        online.step()
        for u in closing:
            assert online.finished(u)
            out[u] = online.result(u)
            live.discard(u)
    return [out[u] for u in range(len(waves))]


def test_online_recognizer_is_the_batch_recognizer(setup):
    s = setup
    online = online_of(s)
    assert (online.scorer.in_dim(), online.scorer.base_dim(), online.scorer.feat_dim()) == (Db, Db, D)
    for chunk, later, mats, want in ((1600, False, None, s["want"]), (1237, True, s["mats"], s["want_utt"]), (1600, False, None, s["want"])):
        got = stream(online, s["waves"], chunk, later, mats)
        for u in range(2):
            assert comparable(got[u]) == comparable(want[u]), (chunk, mats is not None, u)
            assert got[u].segments and all(np.isfinite(g.acoustic_cost) for g in got[u].segments)
    online.decoder.set_commit(True)                          # commit mode: the same Results
    got = stream(online, s["waves"], mats=s["mats"])
    for u in range(2):
        assert comparable(got[u]) == comparable(s["want_utt"][u]), ("commit", u)
    # the front-end's rows as RAW frames [n][Db], ten a step, into the same object; slot 1 with its own matrix
    for u in range(2):
        online.open_features(u, "raw")
    online.scorer.set_slot_transform(1, s["mats"][1])
    with pytest.raises(pk.PkCodeError) as e:                 # [n][feat_dim] frames are not a RAW slot's
        online.push_features(0, np.zeros((3, D), np.float32))
    assert e.value.code == E_INVALID
    pos, live = [0, 0], {0, 1}
    while live:
        for u in sorted(live):
            online.push_features(u, s["rows"][u][pos[u]:pos[u] + 10])
            pos[u] += 10
            if pos[u] >= s["rows"][u].shape[0]:
                online.close(u)
        online.step()
        live = {u for u in live if pos[u] < s["rows"][u].shape[0]}
    assert comparable(online.result(0)) == comparable(s["want"][0]), "raw features"
    assert comparable(online.result(1)) == comparable(s["want_utt"][1]), "raw features, the slot's matrix"
    online.destroy()


def test_with_commit_and_endpointing_the_matrix_belongs_to_the_opening(setup):
    """A rule that fires on every utterance 30 frames long: slot 0 takes the wave 100 ms a step, slot 1 the front-end's rows
    of the same wave, as many a step as slot 0's audio completed, both with the same matrix of their own -- the same
    utterances, cut at the same frames; without the matrix the pieces' costs differ."""
    s = setup
    online = online_of(s)
    online.set_endpointing([10], [pk.EndpointRule(False, 0.0, np.inf, 0.30)])
    online.decoder.set_commit(True)
    costs = {}
    for with_matrix in (True, False):
        wave, rows = s["waves"][0], s["rows"][0]
        online.open(0)
        online.open_features(1, "raw")
        if with_matrix:
            online.scorer.set_slot_transform(0, s["mats"][0])
            online.scorer.set_slot_transform(1, s["mats"][0])
        pos = fed = 0
        while pos < len(wave):
            online.push(0, wave[pos:pos + 1600])
            pos = min(pos + 1600, len(wave))
            n = pk.num_frames(pos)
            online.push_features(1, rows[fed:n])
            fed = n
            if pos == len(wave):
                online.close(0)
                online.close(1)
            online.step()
            if pos < len(wave):
                assert online.decoder.num_frames(0) == online.decoder.num_frames(1)
                assert online.partial(0) == online.partial(1) and online.stable(0) == online.stable(1)
        assert fed == rows.shape[0] and online.finished(0) and online.finished(1)
        a, b = online.utterances(0), online.utterances(1)
        assert [(p.first_frame, p.num_frames, p.rule) for p in a] == [(p.first_frame, p.num_frames, p.rule) for p in b]
        assert len(a) >= 2 and a[-1].rule == 0 and all(p.rule == 1 for p in a[:-1])
        assert sum(p.num_frames for p in a) == rows.shape[0]
        assert [comparable(p.result) for p in a] == [comparable(p.result) for p in b], with_matrix
        costs[with_matrix] = [comparable(p.result) for p in a]
    assert costs[True] != costs[False]                      # every piece of the opening went through the matrix, the first too
    assert costs[True][0] != costs[False][0] and costs[True][-1] != costs[False][-1]
    online.destroy()


def test_online_decoder_advance_over_a_transform_scorer(setup):
    s = setup
    layers, prior, tid2pdf = s["model"]
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    fst = pk.Fst(os.path.join(DIR, "wordloop.fst"))
    waves = s["waves"]
    bs = pk.BatchScorer(am, s["stats"], 2, sum(len(w) for w in waves), frontend=s["fe"], transform=s["spec"])
    bs.set_waves(waves)
    bs.set_utt_transforms(s["mats"])
    bs.score(0.1)
    dec = pk.Decoder(fst, am, 2)
    dec.decode_batch(bs)
    want = [dec.result(u) for u in range(2)]
    sc = pk.OnlineScorer.with_transform(am, s["stats"], 2, 2 * 1600, s["spec"], frontend=s["fe"])
    od = pk.OnlineDecoder(fst, am, 2)
    pos, live = [0, 0], {0, 1}
    for u in live:
        sc.open(u)
        sc.set_slot_transform(u, s["mats"][u])
        od.open(u)
    while live:
        for u in sorted(live):
            sc.push(u, waves[u][pos[u]:pos[u] + 1600])
            pos[u] += 1600
            if pos[u] >= len(waves[u]):
                sc.close(u)
                live.discard(u)
        sc.step(0.1, sync=False)
        od.advance(sc)
    for u in range(2):
        words, weight_, ok = od.result(u)
        assert (words, ok) == (want[u][0], want[u][2]) and np.float32(weight_).tobytes() == np.float32(want[u][1]).tobytes(), u
        assert od.num_frames(u) == bs.num_frames(u)
    for o in (od, sc):
        o.destroy()
    for o in (dec, bs, fst, am):
        o.close()


def test_refusals_are_the_stream_entry_s(setup):
    s = setup
    with pytest.raises(pk.PkCodeError) as e:                 # 13 is odd: two blocks do not divide it
        pk.OnlineRecognizer.with_transform(s["conf"], s["spec"], frontend=s["fe"], deltas=pk.DeltaSpec(1, 2))
    assert e.value.code == E_INVALID and "2 blocks" in str(e.value) and "13" in str(e.value)
    with pytest.raises(pk.PkCodeError) as e:
        pk.OnlineRecognizer.with_transform(s["conf"], s["spec"], frontend=s["fe"], deltas=pk.DeltaSpec(4, 2))
    assert e.value.code == E_INVALID and "order" in str(e.value)
    with pytest.raises(pk.PkCodeError) as e:                 # a front-end of another dimension than Db
        pk.OnlineRecognizer.with_transform(s["conf"], s["spec"], frontend=pk.FrontendSpec(num_mel_bins=80))
    assert e.value.code == E_INVALID and "80" in str(e.value)
    to39 = pk.TransformSpec(TC.matrix(Db, CTX, CTX, 39, True), CTX, CTX)
    with pytest.raises(pk.PkCodeError) as e:                 # a transform of another output dimension than the model's
        pk.OnlineRecognizer.with_transform(s["conf"], to39, frontend=s["fe"])
    assert e.value.code == E_INVALID and "39" in str(e.value)


def test_online_transforms_example_equals_python():
    Lm, Rm, N, Lt, Rt = 2, 1, 16, 3, 3
    wav = os.path.join(REPO, "tests", "golden", "en-us-hello.wav")
    got = subprocess.run([build("online_transforms_example"), wav], capture_output=True, text=True)
    assert got.returncode == 0 and "online_transforms_example ok" in got.stdout, got.stdout + got.stderr
    fe = pk.FrontendSpec("mfcc", 23, 13, "povey", 20.0, 0.0, 22.0)
    K = (Lt + Rt + 1) * fe.dim
    lda = (weight(2000003 + np.arange(D * (K + 1))) * np.float32(4.0)).reshape(D, K + 1)
    k = np.arange(D * (D + 1))
    fmllr = (weight(3000017 + k) + (k // (D + 1) == k % (D + 1)).astype(np.float32)).reshape(D, D + 1)
    W = weight(np.arange(N * D * (Lm + Rm + 1))).reshape(N, D * (Lm + Rm + 1))
    b = weight(1000003 + np.arange(N))
    am = pk.AcousticModel([("linear", W, b), ("softmax",)], np.full(N, 1.0 / N, np.float32), Lm, Rm)
    g = np.zeros(fe.dim + 1, np.float32)
    g[fe.dim] = 1.0
    wave = pk.read_wav(wav)
    bs = pk.BatchScorer(am, g, 1, wave.shape[0] + 1, frontend=fe, transform=pk.TransformSpec(lda, Lt, Rt))
    bs.set_waves([wave])
    bs.set_utt_transforms([fmllr])
    bs.score(0.1)
    rows = bs.fetch(0).log_prob()
    assert got.stdout.splitlines()[:2] == ["frames %d base %d dim %d" % (rows.shape[0], fe.dim, D), "loglik %s" % fnv(rows.tobytes())]
    bs.close()
    am.close()
