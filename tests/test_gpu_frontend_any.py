"""The front-end at a specification on the GPU: FbankAnyKernel through pk.Frontend and through
pk.BatchScorer(..., frontend=spec).
  * Single utterance: pk.Frontend(spec).compute equals the numpy restatement (tests/frontend_any_cases.py) bit for bit at
    every spec -- bin counts around the lane wrap, single-tap triangles, a 3-bin spec with 200-tap triangles, MFCC with
    and without lifter -- on the frame-count edges, both DC paths, silence, a wave every wavefront walks twice, and
    with a NaN and an inf sample (exactly the frames that hold them change).
  * Batch: fetch_fbank is the restatement, fetch_cmvn the CMVN rule of the dimension, the log-likelihoods those of
    pk.FeatureScorer on the same rows as RAW features, bit for bit in both softmax modes; every wave entry, other sample
    rates, switching sources, a failed call, a poisoned neighbour, the decoder, f16x3.
  * Failure codes."""
import ctypes as C

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth
from pocketkaldi_amd import synth_graph as SG
from oracle import oracle as O

import cmvn_any_cases as CA
import frontend_any_cases as FA
from test_gpu_parity import assert_loglik_close

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
GRID = 3072                                        # LaunchFbankAny: workgroups of four frames over one utterance, at most


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


_tables = {}


def tables(spec):
    key = FA.spec_id(spec)
    if key not in _tables:
        _tables[key] = pk.frontend_tables(spec)
    return _tables[key]


def restated(wave, spec):
    return FA.frontend_any(wave, spec, tables(spec))


def tiny(D, L=2, R=1, softmax="stable", precision="f32"):
    layers, prior, _, _ = synth.model("tiny", feat_dim=D, left=L, right=R)
    return pk.AcousticModel(layers, prior, L, R, precision=precision).set_softmax(softmax)


def stats_for(D):
    """Count 2500, every mean 10."""
    return np.concatenate([np.full(D, 10.0 * 2500.0), [2500.0]]).astype(np.float32)


def stats_of(rows):
    """Count 2500 and the rows' own means: what a model's statistics are to its features.  (With far-off means the first
    frames of an utterance, which lean on the global statistics, reach the layers unnormalised, and the reference
    softmax overflows on them.)"""
    mean = np.concatenate([r for r in rows if r.shape[0]]).astype(np.float64).mean(axis=0)
    return np.concatenate([mean * 2500.0, [2500.0]]).astype(np.float32)


def cmvn_rule(g, rows):
    return O.cmvn(g, rows) if rows.shape[1] == 40 else CA.cmvn_any(g, rows)


def fetch_rows(bs):
    return [bs.fetch(u).log_prob() for u in range(bs.num_utts())]


# ---------------------------------------------------------------- single utterance

@pytest.mark.parametrize("spec", FA.SPECS, ids=[FA.spec_id(s) for s in FA.SPECS])
def test_compute_equals_the_restatement_bit_for_bit(spec):
    fe = pk.Frontend(spec)
    for name, w in FA.waves().items():
        got, want = fe.compute(w), restated(w, spec)
        if pk.num_frames(w.size) == 0:             # an empty matrix, as pk.Fbank gives (fbank.cc:272-273)
            assert got.size == 0 and want.shape[0] == 0, name
            continue
        assert got.shape == (pk.num_frames(w.size), spec.dim), name
        assert bits_equal(got, want), "%s on %s: %d values differ" % (
            FA.spec_id(spec), name, int(np.sum(got.view(np.uint32) != want.view(np.uint32))) if got.shape == want.shape else -1)
        if name.startswith("zero"):
            assert np.isfinite(got).all()          # silence: every energy at the floor


@pytest.mark.parametrize("spec", [FA.SPECS[1], FA.SPECS[9]], ids=["fbank80", "mfcc13of23"])
def test_every_wavefront_walks_a_second_frame(spec):
    T = 4 * GRID + 1
    w = FA.wave_float(400 + 160 * (T - 1), 21)
    got = pk.Frontend(spec).compute(w)
    assert got.shape == (T, spec.dim)
    assert bits_equal(got, restated(w, spec))


@pytest.mark.parametrize("spec", [FA.SPECS[0], FA.SPECS[1], FA.SPECS[8], FA.SPECS[9], FA.SPECS[12]],
                         ids=["default", "fbank80", "fbank128", "mfcc13of23", "mfcc65of65"])
def test_a_nan_and_an_inf_sample_change_exactly_their_frames(spec):
    clean = FA.wave_float(2000, 31)                # 11 frames; sample 450 lies in frames 1, 2 and sample 1700 in frames 9, 10
    bad = clean.copy()
    bad[450], bad[1700] = np.nan, np.inf
    hit = np.array([any(160 * t <= i < 160 * t + 400 for i in (450, 1700)) for t in range(11)])
    assert hit.tolist() == [t in (1, 2, 9, 10) for t in range(11)]
    fe = pk.Frontend(spec)
    got, ref = fe.compute(bad), fe.compute(clean)
    assert np.isfinite(ref).all()
    assert bits_equal(got[~hit], ref[~hit])
    want = restated(bad, spec)
    assert np.isnan(want[hit]).all() or spec.kind == 1
    assert FA.same_bits(got, want)
    assert np.isnan(got[hit]).any(axis=1).all()


# ---------------------------------------------------------------- batch

LENGTHS = (399, 1237, 0, 4321, 159)                # frameless first, in the middle and last; odd offsets between them


def batch_waves(seed):
    return [FA.wave_i16(n, seed + u) for u, n in enumerate(LENGTHS)]


class DeviceWaves:
    """The waves one after the other in HBM, one float into the allocation (4-byte aligned and no better)."""

    def __init__(self, waves):
        cat = np.ascontiguousarray(np.concatenate(waves), np.float32)
        self.base = pk.lib().pk_mi355_device_malloc(cat.nbytes + 4)
        assert self.base
        self.ptr = self.base + 4
        assert pk.lib().pk_mi355_memcpy(C.c_void_p(self.ptr), cat.ctypes.data_as(C.c_void_p), cat.nbytes, 1) == 0

    def free(self):
        pk.lib().pk_mi355_device_free(C.c_void_p(self.base))


def feature_scorer_rows(am, g, rows):
    fs = pk.FeatureScorer(am, len(rows), max(sum(r.shape[0] for r in rows), 1), global_stats=g)
    fs.set_features(rows, "raw")
    fs.score(0.1)
    out = fetch_rows(fs)
    fs.close()
    return out


@pytest.mark.parametrize("D", sorted(FA.BATCH_SPECS))
def test_batch_scorer_with_a_frontend(D):
    spec = FA.BATCH_SPECS[D]
    assert spec.dim == D
    waves = batch_waves(100 * D)
    rows = [restated(w, spec) for w in waves]
    g = stats_of(rows)
    frames = [r.shape[0] for r in rows]
    assert frames == [0, 6, 0, 25, 0]
    norm = [cmvn_rule(g, r) if r.shape[0] else r for r in rows]
    cap = sum(LENGTHS) + 4000
    dev = DeviceWaves(waves)
    try:
        for softmax in ("stable", "reference"):
            am = tiny(D, softmax=softmax)
            want = feature_scorer_rows(am, g, rows)
            assert all(np.isfinite(w).all() for w in want)
            bs = pk.BatchScorer(am, g, len(waves), cap, frontend=spec)
            assert bs.feat_dim() == D

            def check(what):
                bs.score(0.1)
                for u in range(len(waves)):
                    assert bs.num_frames(u) == frames[u], (what, u)
                    assert bits_equal(bs.fetch_fbank(u), rows[u]), "%s D=%d utterance %d: the front-end's rows differ" % (what, D, u)
                    assert bits_equal(bs.fetch_cmvn(u), norm[u]), "%s D=%d utterance %d: CMVN differs" % (what, D, u)
                    assert bits_equal(bs.fetch(u).log_prob(), want[u]) or frames[u] == 0, "%s D=%d utterance %d: rows differ" % (what, D, u)

            bs.enable_timing(True)
            bs.set_waves(waves)
            check("set_waves")
            t = bs.timing()
            assert t["fbank"][1] == 1 and t["cmvn"][1] == 1, t
            bs.enable_timing(False)
            bs.set_waves_i16([w.astype(np.int16) for w in waves])
            check("set_waves_i16")
            bs.set_waves_device(dev.ptr, list(LENGTHS))
            check("set_waves_device")
            # waves -> features -> waves on one object
            bs.set_features(norm, "normalized")
            bs.score(0.1)
            for u, r in enumerate(fetch_rows(bs)):
                assert bits_equal(r, want[u]) or frames[u] == 0, ("normalized", u)
            bs.set_features(rows, "raw")
            bs.score(0.1)
            for u, r in enumerate(fetch_rows(bs)):
                assert bits_equal(bs.fetch_cmvn(u), norm[u]) and (bits_equal(r, want[u]) or frames[u] == 0), ("raw", u)
            bs.set_waves(waves)
            check("waves after features")
            # a failed call changes nothing that a later call sees
            with pytest.raises(pk.PkError):
                bs.set_waves([FA.wave_i16(cap + 1, 1)])
            with pytest.raises(pk.PkError):
                bs.set_waves(waves + waves)
            bs.set_waves_i16([w.astype(np.int16) for w in waves])
            check("after failed calls")
            # a poisoned neighbour: NaN and 1e30 utterances between the healthy ones
            mixed = [waves[1], np.full(1600, np.nan, np.float32), waves[3], np.full(900, 1e30, np.float32), waves[0]]
            bs.set_waves(mixed)
            bs.score(0.1)
            for at, u in ((0, 1), (2, 3)):
                assert bits_equal(bs.fetch_fbank(at), rows[u]) and bits_equal(bs.fetch_cmvn(at), norm[u]), (at, u)
                assert bits_equal(bs.fetch(at).log_prob(), want[u]), (at, u)
            assert np.isnan(bs.fetch(1).log_prob()).all() and bs.num_frames(4) == 0
            bs.set_waves(waves)
            check("after the poisoned batch")
            bs.close()
            am.close()
    finally:
        dev.free()


@pytest.mark.parametrize("D", [13, 80])
def test_other_sample_rates_equal_resampling_first(D):
    spec = FA.BATCH_SPECS[D]
    am = tiny(D)
    rates = [8000, 16000, 44100, 22050, 48000]
    native = [FA.wave_i16(int(n), 7 + u) for u, n in enumerate((2500, 1237, 9000, 0, 700))]
    at16 = [w if r == 16000 else pk.resample(w, r) for w, r in zip(native, rates)]
    cap = sum(w.size for w in at16)                # capacity counts 16 kHz samples
    g = stats_of([restated(w, spec) for w in at16])
    bs = pk.BatchScorer(am, g, len(native), cap, frontend=spec)
    bs.set_waves(at16)
    bs.score(0.1)
    want_fb, want = [bs.fetch_fbank(u) for u in range(len(native))], fetch_rows(bs)
    assert sum(w.shape[0] for w in want_fb) > 20
    for u, w in enumerate(at16):
        assert bits_equal(want_fb[u], restated(w, spec)), u
    bs.set_waves(native, rates=rates)
    bs.score(0.1)
    for u in range(len(native)):
        assert bits_equal(bs.fetch_fbank(u), want_fb[u]) and bits_equal(bs.fetch(u).log_prob(), want[u]), u
    bs.close()
    am.close()


def test_decode_batch_gives_the_feature_scorers_results(tmp_path):
    D = 65
    spec = FA.BATCH_SPECS[D]
    am = tiny(D)
    graph = SG.word_loop(30, 8, seed=3)
    assert graph["num_tids"] <= am.num_pdfs()
    path = str(tmp_path / "loop.fst")
    SG.write_fst(path, graph["start"], graph["final"], graph["arcs"])
    fst = pk.Fst(path)
    waves = [FA.wave_float(n, 40 + u) for u, n in enumerate((8000, 399, 16000, 560))]
    rows = [restated(w, spec) for w in waves]
    g = stats_of(rows)
    fs = pk.FeatureScorer(am, len(rows), sum(r.shape[0] for r in rows), global_stats=g)
    fs.set_features(rows, "raw")
    fs.score(0.1)
    bs = pk.BatchScorer(am, g, len(waves), sum(w.size for w in waves), frontend=spec)
    bs.set_waves(waves)
    bs.score(0.1)
    dec = pk.Decoder(fst, am, len(waves))
    dec.decode_batch(fs)
    want = [dec.result(u) for u in range(len(waves))]
    dec.decode_batch(bs)
    got = [dec.result(u) for u in range(len(waves))]
    for u in range(len(waves)):
        assert got[u][0] == want[u][0] and np.float32(got[u][1]).tobytes() == np.float32(want[u][1]).tobytes() and got[u][2] == want[u][2], u
    assert any(w[0] for w in want)
    for o in (dec, bs, fs):
        o.close()
    am.close()


def test_f16x3_at_80_against_the_f32_result():
    D = 80
    spec = FA.BATCH_SPECS[D]
    waves = batch_waves(900)
    g = stats_of([restated(w, spec) for w in waves])
    am32, am16 = tiny(D), tiny(D, precision="f16x3")
    cap = sum(LENGTHS)
    ref = pk.BatchScorer(am32, g, len(waves), cap, frontend=spec)
    ref.set_waves(waves)
    ref.score(0.1)
    bs = pk.BatchScorer(am16, g, len(waves), cap, frontend=spec)
    bs.set_waves(waves)
    bs.calibrate()
    bs.score(0.1)
    worst = 0.0
    for u in range(len(waves)):
        got, want = bs.fetch(u).log_prob(), ref.fetch(u).log_prob()
        assert bits_equal(bs.fetch_fbank(u), ref.fetch_fbank(u)) and bits_equal(bs.fetch_cmvn(u), ref.fetch_cmvn(u)), u
        if want.shape[0] == 0:
            assert got.shape[0] == 0
            continue
        worst = max(worst, float((np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)).max()))
        assert_loglik_close(got, want.astype(np.float64))
    print("FRONTEND_ANY_F16X3_MAX_ERR %.3e (contract 1e-4)" % worst)
    for o in (bs, ref, am16, am32):
        o.close()


# ---------------------------------------------------------------- failure codes

def code_of(call, *args, **kw):
    with pytest.raises(pk.PkCodeError) as e:
        call(*args, **kw)
    return e.value.code, str(e.value)


def test_failure_codes():
    am80, am13, am13h = tiny(80), tiny(13), tiny(13, precision="f16x3")
    spec80, spec13 = FA.BATCH_SPECS[80], FA.BATCH_SPECS[13]
    g80, g13 = stats_for(80), stats_for(13)
    code, msg = code_of(pk.BatchScorer, am80, g80, 2, 16000, frontend=spec13)            # spec dimension against the model's
    assert code == E_INVALID and "13" in msg and "80" in msg, msg
    code, msg = code_of(pk.BatchScorer, am80, g13, 2, 16000, frontend=spec80)            # statistics length
    assert code == E_INVALID and "14" in msg and "81" in msg, msg
    code, msg = code_of(pk.BatchScorer, am80, stats_for(40), 2, 16000, frontend=spec80)
    assert code == E_INVALID and "41" in msg and "81" in msg, msg
    code, msg = code_of(pk.BatchScorer, am13h, g13, 2, 16000, frontend=spec13)           # f16: a multiple of 8
    assert code == E_INVALID and "multiple of 8" in msg, msg
    code, msg = code_of(pk.BatchScorer, am80, g80, 2, 16000, frontend=FA.S(bins=127))    # a refused spec, by name
    assert code == E_INVALID and "empty triangle" in msg, msg
    for units, samples in ((0, 16000), (2, 0), (-1, 16000)):
        assert code_of(pk.BatchScorer, am80, g80, units, samples, frontend=spec80)[0] == E_INVALID
    with pytest.raises(pk.PkError, match="41 entries"):                                  # without frontend=: the old constructor
        pk.BatchScorer(am80, g80, 2, 16000)
    bs = pk.BatchScorer(am13, g13, 2, 4000, frontend=spec13)
    w = FA.wave_float(1500, 3)
    bs.set_waves([w])
    with pytest.raises(pk.PkError, match="samples"):                                     # over capacity: samples, utterances
        bs.set_waves([FA.wave_float(4001, 4)])
    with pytest.raises(pk.PkError, match="utterances"):
        bs.set_waves([w[:500], w[:500], w[:500]])
    assert code_of(bs.set_waves, [FA.wave_float(9000, 5)], rates=[8000])[0] == E_INVALID     # 18000 samples at 16 kHz
    assert code_of(bs.set_features, [np.zeros((3, 40), np.float32)], "raw")[0] == E_INVALID
    bs.set_waves([w])                                                                    # a call after the failed calls
    bs.score(0.1)
    assert bits_equal(bs.fetch_fbank(0), restated(w, spec13))
    bs.close()
    for am in (am80, am13, am13h):
        am.close()
