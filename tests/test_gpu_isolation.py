"""Isolation and reuse of the scorers (include/pk_mi355.h, "Isolation and reuse"; the designed waves and layouts are
tests/isolation_cases.py, their predictions are checked against the oracle and the live reference in
test_isolation_cases.py):
  1. f32 batch: a neighbour full of NaN, Inf or loud non-integer samples changes no bit of an utterance's results;
  2. batch reuse (f32 and f16x3): what an earlier call left in any buffer of the scorer changes no bit of a call's;
  3. the single-utterance workspace behind pk_decodable_init / pk_mi355_nnet_propagate, likewise;
  4. the online scorer: a poisoned neighbour slot, a slot reopened after a NaN stream, one step of more than 600 new
     frames on top of history, and a 600-frame ring that wraps twice.
Every comparison is bitwise (NaN where NaN is owed), or the 1e-4 contract of the stable tail against the oracle
(test_gpu_parity.assert_loglik_close).  No utterance, row or slot is left out."""
import functools

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth
from oracle import oracle as O

import isolation_cases as C
from test_gpu_parity import assert_loglik_close
from test_gpu_stream import batch_rows, chunks_of, model_s, refmodel, run_jobs

pytestmark = pytest.mark.gpu

SOFTMAX = ["stable", "reference"]
SETTINGS = {"default": {}, "chunk128_lanes2": {"PK_MI355_CHUNK": "128", "PK_MI355_LANES": "2"}}


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def model(which):
    """-> (layers, prior, L, R, tid2pdf, cmvn global stats)."""
    if which == "refmodel":
        return refmodel()
    if which == "S":
        return model_s()
    return synth.model(which) + (None, synth.global_cmvn_stats())


def new_am(which, softmax="stable", precision="f32"):
    layers, prior, L, R, tid2pdf, _ = model(which)
    return pk.AcousticModel(layers, prior, L, R, tid2pdf, precision=precision).set_softmax(softmax)


_oracle = {}


def oracle_stages(which, key, wave):
    """(fbank, cmvn, log-likelihoods) of one wave by the oracle: made once, shared, left unchanged."""
    if (which, key) not in _oracle:
        layers, prior, L, R, _, g = model(which)
        raw = O.Fbank().compute(wave)
        y = O.cmvn(g, raw)
        with np.errstate(invalid="ignore"):
            _oracle[(which, key)] = (raw, y, O.Nnet(layers).am_compute(y, prior, L, R, 0.1))
    return _oracle[(which, key)]


def assert_held_to_oracle(which, softmax, key, wave, pred, fb, cm, ll, what):
    """fbank and CMVN bit for bit, log-likelihoods bit for bit (reference softmax) or within the 1e-4 contract (stable
    tail) on every row that is not NaN; the NaN rows are the oracle's and the predicted ones, stage by stage."""
    T, R = pred.T, model(which)[3]
    if T == 0:
        assert fb.shape[0] == cm.shape[0] == ll.shape[0] == 0, what
        return
    raw, y, ref = oracle_stages(which, key, wave)
    assert fb.shape == raw.shape and cm.shape == y.shape and ll.shape == ref.shape, (what, fb.shape, cm.shape, ll.shape)
    C.assert_nan_rows(fb, pred.fbank, what + " fbank")
    C.assert_nan_rows(cm, pred.cmvn, what + " cmvn")
    C.assert_nan_rows(ll, pred.loglik(R), what + " loglik")
    assert C.same_bits(fb, raw), what + ": fbank differs from the oracle's"
    assert C.same_bits(cm, y), what + ": CMVN differs from the oracle's"
    if softmax == "reference":
        assert C.same_bits(ll, ref), what + ": log-likelihoods differ from the oracle's"
    else:
        C.assert_nan_rows(ref, pred.loglik(R), what + " oracle loglik")
        keep = ~pred.loglik(R)
        assert_loglik_close(ll[keep], ref[keep])


# ---------------------------------------------------------------- 1. batch neighbours

_alone = {}


def scored_alone(which, softmax, am, e):
    """Utterance e scored alone in a fresh one-utterance BatchScorer (default settings): made once per model, softmax
    mode and wave, shared by the cases below and left unchanged."""
    key = (which, softmax, e["kind"], e["seed"], e["T"])
    if key not in _alone:
        _alone[key] = batch_rows(am, model(which)[5], [e["wave"]])[0]
    return _alone[key]


def check_layout(name, rotation, softmax, settings, monkeypatch, oracle):
    which = C.LAYOUTS[name][0]
    g, R = model(which)[5], model(which)[3]
    am = new_am(which, softmax)
    utts = C.layout_utterances(name, rotation)
    alone = [scored_alone(which, softmax, am, e) for e in utts]           # (before the settings below take hold)
    for k, v in SETTINGS[settings].items():
        monkeypatch.setenv(k, v)
    bs = pk.BatchScorer(am, g, len(utts), sum(len(e["wave"]) for e in utts))
    bs.set_waves([e["wave"] for e in utts])
    bs.score(0.1)
    assert bs.total_frames() == sum(e["T"] for e in utts)
    for u, e in enumerate(utts):
        what = "layout %s rotation %d %s utterance %d (%d frames, %s)" % (name, rotation, softmax, u, e["T"], e["kind"] or "healthy")
        ll = bs.fetch(u).log_prob()
        assert ll.shape == (e["T"], am.num_pdfs() if e["T"] else 0), (what, ll.shape)
        C.assert_nan_rows(ll, e["pred"].loglik(R), what)
        if e["kind"] is None:
            assert bits_equal(ll, alone[u]), what + ": differs from the utterance scored alone"
        else:                                                             # a poisoned utterance is its own samples' function too
            assert C.same_bits(ll, alone[u]), what + ": differs from the utterance scored alone"
        if e["kind"] == "loud":
            assert np.isfinite(ll).all(), what
        if oracle:
            assert_held_to_oracle(which, softmax, (e["kind"], e["seed"], e["T"]), e["wave"], e["pred"], bs.fetch_fbank(u),
                                  bs.fetch_cmvn(u), ll, what)
    bs.close()


@pytest.mark.parametrize("settings", list(SETTINGS))
@pytest.mark.parametrize("softmax", SOFTMAX)
@pytest.mark.parametrize("rotation", list(C.ROTATIONS))
def test_batch_neighbours_small_tiles(rotation, softmax, settings, monkeypatch):
    """Layout A, model tiny: every stage of every utterance against the oracle, and against the utterance alone."""
    check_layout("A", rotation, softmax, settings, monkeypatch, oracle=True)


@pytest.mark.parametrize("softmax", SOFTMAX)
@pytest.mark.parametrize("rotation", list(C.ROTATIONS))
@pytest.mark.parametrize("name", ["B", "C"])
def test_batch_neighbours_fused_tail_and_big_tiles(name, rotation, softmax, monkeypatch):
    """Layouts B (fused tail plus strip launch, NaN and healthy rows in one 128-row tile) and C (big tiles in every
    layer), model S: every utterance bit for bit the utterance scored alone."""
    check_layout(name, rotation, softmax, "default", monkeypatch, oracle=False)


# ---------------------------------------------------------------- 2. batch reuse

def is_range_error(e):
    return "range" in str(e)


def score_layout(bs, waves, i16):
    """Set, score and read everything back: per-utterance fetches of all three stages and one fetch_all."""
    if i16 and waves:
        bs.set_waves_i16([w.astype(np.int16) for w in waves])
    else:
        bs.set_waves(waves)
    bs.score(0.1)
    n = len(waves)
    assert bs.num_utts() == n
    out = {"ll": [bs.fetch(u).log_prob() for u in range(n)], "fb": [bs.fetch_fbank(u) for u in range(n)],
           "cm": [bs.fetch_cmvn(u) for u in range(n)]}
    views = bs.fetch_all()
    out["all"] = [v.log_prob() for v in views]
    for v in views:
        v.destroy()
    return out


@pytest.mark.parametrize("ingest", ["f32_then_i16", "i16_then_f32"])
@pytest.mark.parametrize("settings", list(SETTINGS))
@pytest.mark.parametrize("prec,kind,softmax", [("f32", "nan_all", "stable"), ("f32", "nan_all", "reference"), ("f32", "loud", "stable"),
                                               ("f32", "loud", "reference"), ("f16x3", "loud", "stable")])
def test_batch_reuse_after_poisoned_calls(prec, kind, softmax, settings, ingest, monkeypatch):
    """One BatchScorer(am, g, 8, cap).  A poison call fills it to both capacities; then, in turn, fewer and shorter
    utterances, the same count each 1 to 3 frames shorter (context pads where features were), frameless utterances in
    between, a single one-frame utterance, an empty batch and straight after it a healthy batch at full capacity -- the
    scorer poisoned again after each but the empty one.  f32_then_i16: poison by float, healthy by int16 (each path has
    a PCM buffer of its own); i16_then_f32: full-scale int16 noise on top of the float poison, healthy by float.  Every
    result equals a fresh scorer's bit for bit; f32 is held to the oracle as well.  f16x3: the poison call may fail its
    range check (PK_MI355_E_RANGE) -- that is its contract, and no later call's business; the fresh and the reused
    scorer share one model, calibrated once on the healthy full batch."""
    for k, v in SETTINGS[settings].items():
        monkeypatch.setenv(k, v)
    g, N = model("tiny")[5], len(model("tiny")[1])
    am = new_am("tiny", softmax, prec)
    full = [i for i, (name, _) in enumerate(C.REUSE_LAYOUTS) if name == "full"][0]
    if prec != "f32":
        cal = pk.BatchScorer(am, g, C.REUSE_MAX_UTTS, C.REUSE_CAP)
        cal.set_waves(C.reuse_healthy_waves(full))
        cal.calibrate()
        cal.close()
    bs = pk.BatchScorer(am, g, C.REUSE_MAX_UTTS, C.REUSE_CAP)
    assert sum(len(w) for w in C.reuse_poison_waves(kind)) == C.REUSE_CAP and len(C.REUSE_POISON_FRAMES) == C.REUSE_MAX_UTTS

    def poison_call(set_waves, waves, want_nan):
        set_waves(waves)
        try:
            bs.score(0.1)
            views = bs.fetch_all()
        except pk.PkError as e:
            assert prec != "f32" and is_range_error(e), e
            return
        assert [v.log_prob().shape for v in views] == [(T, N) for T in C.REUSE_POISON_FRAMES]
        if prec == "f32":
            assert all(np.isnan(v.log_prob()).all() if want_nan else np.isfinite(v.log_prob()).all() for v in views)
        for v in views:
            v.destroy()

    def poison():
        poison_call(bs.set_waves, C.reuse_poison_waves(kind), kind == "nan_all")
        if ingest == "i16_then_f32":
            poison_call(bs.set_waves_i16, C.reuse_poison_waves_i16(), False)

    def healthy(i):
        name, frames = C.REUSE_LAYOUTS[i]
        waves = C.reuse_healthy_waves(i)
        got = score_layout(bs, waves, ingest == "f32_then_i16")
        fresh_bs = pk.BatchScorer(am, g, C.REUSE_MAX_UTTS, C.REUSE_CAP)
        want = score_layout(fresh_bs, waves, ingest == "f32_then_i16")
        fresh_bs.close()
        assert len(got["ll"]) == len(got["all"]) == len(frames)           # fetch_all shows this call's rows, and only them
        for u, T in enumerate(frames):
            what = "%s %s %s after %s, layout %s utterance %d (%d frames)" % (prec, settings, ingest, kind, name, u, T)
            assert got["ll"][u].shape == (T, N if T else 0), (what, got["ll"][u].shape)
            assert bits_equal(got["all"][u], got["ll"][u]), what + ": fetch_all differs from fetch"
            for stage in ("fb", "cm", "ll", "all"):
                assert bits_equal(got[stage][u], want[stage][u]), what + ": %s differs from a fresh scorer's" % stage
            if prec == "f32":
                key = ("reuse", i, u)
                assert_held_to_oracle("tiny", softmax, key, waves[u], C.Prediction(T, [], None), got["fb"][u], got["cm"][u],
                                      got["ll"][u], what)

    poison()
    for i, (name, _) in enumerate(C.REUSE_LAYOUTS):
        healthy(i)
        if name not in ("empty", "full"):
            poison()
    bs.close()


# ---------------------------------------------------------------- 3. the single-utterance workspace

@pytest.mark.parametrize("stack", C.SINGLE_STACKS)
def test_single_utterance_workspace_after_nan_f32(stack):
    """pk_decodable_init and pk_mi355_nnet_propagate on one model object: 4 500 frames of NaN (two 4 096-row passes),
    then healthy features of 1, 127, 129 and 4 097 frames -- the oracle's bits (reference softmax)."""
    layers, prior, L, R = C.single_stack(stack)
    am = pk.AcousticModel(layers, prior, L, R).set_softmax("reference")
    nn = O.Nnet(layers)
    nan_feats = np.full((C.SINGLE_POISON_T, 40), np.nan, np.float32)
    nan_x = np.full((C.SINGLE_POISON_T, 40 * (L + R + 1)), np.nan, np.float32)
    for T in C.SINGLE_T:
        assert np.isnan(pk.Decodable(am, 0.1, nan_feats).log_prob()).all()
        feats = C.single_features(T)
        got = pk.Decodable(am, 0.1, feats).log_prob()
        assert bits_equal(got, nn.am_compute(feats, prior, L, R, 0.1)), (stack, T, "decodable")
        assert np.isnan(am.propagate(nan_x)).all()
        x = O.splice(feats, L, R)
        assert bits_equal(am.propagate(x), nn.propagate(x)), (stack, T, "propagate")


@pytest.mark.parametrize("stack", C.SINGLE_STACKS)
def test_single_utterance_workspace_after_loud_f16x3(stack):
    """The same on an f16x3 model, calibrated on healthy features: 4 500 loud finite frames, past the fp16 clamp at the
    calibrated exponent (the call may fail its range check: its contract), then the healthy calls -- the bits of a fresh
    model object with the same exponents, and no verdict inherited from the loud call's leftovers."""
    layers, prior, L, R = C.single_stack(stack)
    am = pk.AcousticModel(layers, prior, L, R, precision="f16x3").calibrate(C.single_features(600, seed=2))
    x_exp = am.exponents()[1]
    # loud enough that the first operand passes the fp16 clamp (|x| 2^x_exp >= 65504) wherever it is counted
    loud = C.single_features(C.SINGLE_POISON_T, seed=1)
    loud *= np.float32(2.0 ** np.ceil(np.log2(4 * 65504.0 / (np.abs(loud).max() * 2.0 ** int(x_exp[0])))))
    assert np.isfinite(loud).all() and np.abs(loud).max() * 2.0 ** int(x_exp[0]) >= 4 * 65504.0
    loud_x = O.splice(loud, L, R)

    def fresh():
        m = pk.AcousticModel(layers, prior, L, R, precision="f16x3")
        m.set_input_exponents(x_exp)
        return m

    def poisoned(call):
        try:
            assert np.isfinite(call()).all()
        except pk.PkError as e:
            assert is_range_error(e), e

    for T in C.SINGLE_T:
        feats = C.single_features(T)
        poisoned(lambda: pk.Decodable(am, 0.1, loud).log_prob())
        got = pk.Decodable(am, 0.1, feats).log_prob()
        assert got.shape == (T, len(prior))
        assert bits_equal(got, pk.Decodable(fresh(), 0.1, feats).log_prob()), (stack, T, "decodable")
        poisoned(lambda: am.propagate(loud_x))
        x = O.splice(feats, L, R)
        assert bits_equal(am.propagate(x), fresh().propagate(x)), (stack, T, "propagate")


# ---------------------------------------------------------------- 4. the online scorer

WHICH = ["refmodel", "S"]


@pytest.mark.parametrize("kind", ["nan_from", "loud"])
@pytest.mark.parametrize("softmax", SOFTMAX)
@pytest.mark.parametrize("which", WHICH)
def test_online_neighbour_slot(which, softmax, kind):
    """Four slots; slot 1 streams a poisoned wave, the others healthy ones, 5, 7 and 3 rows a step (padding rows in
    every group of four that meets the next slot's columns).  Every slot equals the batch scorer on its whole wave; the
    poisoned slot's NaN rows are the predicted ones."""
    g, R = model(which)[5], model(which)[3]
    am = new_am(which, softmax)
    waves, pred = C.online_neighbour_waves(kind)
    assert all((C.ONLINE_CHUNK[s] // 160) % 4 for s in range(C.ONLINE_SLOTS) if s != C.ONLINE_POISONED_SLOT)
    want = [batch_rows(am, g, [w])[0] for w in waves]
    sc = pk.OnlineScorer(am, g, C.ONLINE_SLOTS, sum(C.ONLINE_CHUNK.values()))
    got = run_jobs(sc, [{"slot": s, "wave": w, "chunks": chunks_of(len(w), C.ONLINE_CHUNK[s], None), "start": s % 2}
                        for s, w in enumerate(waves)])
    for s in range(C.ONLINE_SLOTS):
        what = "%s %s slot %d beside %s" % (which, softmax, s, kind)
        assert got[s].shape == want[s].shape == (C.ONLINE_T[s], am.num_pdfs()), what
        if s == C.ONLINE_POISONED_SLOT:
            C.assert_nan_rows(got[s], pred.loglik(R), what)
            assert C.same_bits(got[s], want[s]), what
        else:
            assert np.isfinite(got[s]).all(), what
            assert bits_equal(got[s], want[s]), what
    sc.destroy()


@pytest.mark.parametrize("softmax", SOFTMAX)
@pytest.mark.parametrize("which", WHICH)
def test_online_slot_reopened_after_a_nan_stream(which, softmax):
    """705 frames of NaN through slot 0 (the sample tails, the window sums, all 600 frames of the raw ring and the
    context history are NaN afterwards), closed and flushed; the slot reopened with a healthy wave whose window slides
    over that ring: the batch scorer's bits."""
    g = model(which)[5]
    am = new_am(which, softmax)
    bad, good = C.online_reuse_waves()
    sc = pk.OnlineScorer(am, g, 2, 16000)
    rows = run_jobs(sc, [{"slot": 0, "wave": bad, "chunks": chunks_of(len(bad), 16000, None), "start": 0}])[0]
    assert rows.shape == (C.ONLINE_REUSE_T, am.num_pdfs()) and np.isnan(rows).all()
    got = run_jobs(sc, [{"slot": 0, "wave": good, "chunks": chunks_of(len(good), 8000, None), "start": 0}])[0]
    assert C.frames_of(len(good)) >= 700 and bits_equal(got, batch_rows(am, g, [good])[0])
    sc.destroy()


@pytest.mark.parametrize("softmax", SOFTMAX)
@pytest.mark.parametrize("which", WHICH)
def test_online_one_step_of_more_than_600_frames_on_history(which, softmax):
    """50 frames in a first step, then 625 new frames in ONE step: the raw ring is read and overwritten within the
    step, the frames leaving the window come from the step's own rows."""
    g = model(which)[5]
    am = new_am(which, softmax)
    w = C.online_big_step_wave()
    first, big = C.samples_for(C.ONLINE_BIG_STEP[0]), 160 * C.ONLINE_BIG_STEP[1]
    chunks = [first, big, len(w) - first - big]
    assert C.ONLINE_BIG_STEP[1] > 600 and chunks[2] > 0
    sc = pk.OnlineScorer(am, g, 1, big)
    got = run_jobs(sc, [{"slot": 0, "wave": w, "chunks": chunks, "start": 0}])[0]
    assert bits_equal(got, batch_rows(am, g, [w])[0])
    sc.destroy()


_long = {}


@pytest.mark.parametrize("how", ["whole", 1600])
@pytest.mark.parametrize("softmax", SOFTMAX)
@pytest.mark.parametrize("which", WHICH)
def test_online_ring_wraps_twice(which, softmax, how):
    """1 307 frames, pushed whole and in 100 ms chunks."""
    g = model(which)[5]
    am = new_am(which, softmax)
    w = C.online_long_wave()
    if (which, softmax) not in _long:
        _long[(which, softmax)] = batch_rows(am, g, [w])[0]
    sc = pk.OnlineScorer(am, g, 1, len(w) if how == "whole" else how)
    got = run_jobs(sc, [{"slot": 0, "wave": w, "chunks": chunks_of(len(w), how, None), "start": 0}])[0]
    assert got.shape == (C.ONLINE_LONG_T, am.num_pdfs()) and bits_equal(got, _long[(which, softmax)])
    sc.destroy()
