"""Features instead of audio: pk.FeatureScorer, BatchScorer.set_features / set_features_device,
Recognizer.process_features and the command line's --features.
  * FeatureLayoutKernel is a copy: fetch_cmvn returns the input's bits (random bit patterns, NaN payloads, -0.0,
    subnormals), at every feature dimension and context the kernel takes another path for; the pads are held through
    the scores.
  * On finite features every utterance's f32 log-likelihoods are pk.Decodable's on the same model, bit for bit (that
    entry is pinned to the oracle and the reference); f16x3 is held to the oracle at 1e-4 max(|ref|, 1).
  * RAW features are the wave call's fbank: CMVN and log-likelihoods equal the wave call's bit for bit.
  * The device entry, reuse of one scorer across sources, poisoned neighbours, every failure code, and the decoder,
    the recognizer and the command line downstream."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth
from oracle import oracle as O

import isolation_cases as IC
from test_gpu_align import TRACE, check_alignment, got_segments
from test_gpu_decode import flat_arcs
from test_gpu_decode_edges import outcome
from test_gpu_parity import assert_loglik_close

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
# zero-length utterances first, in the middle and last
FRAMES = (0, 1, 2, 3, 0, 4, 5, 63, 64, 65, 0, 127, 128, 129, 200, 0)
DIMS = [1, 3, 39, 40, 63, 64, 65, 130]
CONTEXTS = [(0, 0), (1, 1), (2, 1), (5, 5), (0, 7), (70, 3)]
SPECIALS = np.array([0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF,
                     0x00400000], np.uint32)           # NaN payloads, +-Inf, -0.0, subnormals


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def bit_patterns(T, D, seed):
    rng = np.random.default_rng([0xB175, seed, T, D])
    x = rng.integers(0, 2 ** 32, size=(T, D), dtype=np.uint64).astype(np.uint32)
    flat = x.reshape(-1)
    if flat.size:
        at = rng.integers(0, flat.size, size=max(flat.size // 7, 1))
        flat[at] = SPECIALS[np.arange(len(at)) % len(SPECIALS)]
        flat[0], flat[-1] = SPECIALS[2], SPECIALS[6]                # the frames the pads replicate carry specials too
    return x.view(np.float32)


def finite(T, D, seed, sigma=1.0):
    return (np.random.default_rng([0xF1A7, seed, T, D]).standard_normal((T, D)) * sigma).astype(np.float32)


def tiny(D, L, R, softmax="stable", precision="f32"):
    layers, prior, _, _ = synth.model("tiny", feat_dim=D, left=L, right=R)
    return pk.AcousticModel(layers, prior, L, R, precision=precision).set_softmax(softmax), layers, prior


def decodable_rows(am, feats):
    d = pk.Decodable(am, 0.1, feats)
    out = d.log_prob()
    d.destroy()
    return out


def fetch_rows(bs):
    return [bs.fetch(u).log_prob() for u in range(bs.num_utts())]


def assert_rows_are_decodables(am, bs, feats, what):
    got = fetch_rows(bs)
    assert len(got) == len(feats)
    for u, f in enumerate(feats):
        if f.shape[0] == 0:
            assert got[u].shape[0] == 0, (what, u)
            continue
        want = decodable_rows(am, f)
        assert got[u].shape == want.shape == (f.shape[0], am.num_pdfs()), (what, u, got[u].shape)
        assert np.isfinite(want).all(), (what, u)
        assert bits_equal(got[u], want), "%s utterance %d (%d frames): differs from pk.Decodable" % (what, u, f.shape[0])


# ---------------------------------------------------------------- layout, bit for bit; the pads through the scores

@pytest.mark.parametrize("D", DIMS)
def test_layout_is_a_copy_and_the_pads_hold_through_the_scores(D):
    for k, (L, R) in enumerate(CONTEXTS):
        am, _, _ = tiny(D, L, R, softmax=("stable", "reference")[k % 2])
        fs = pk.FeatureScorer(am, len(FRAMES), sum(FRAMES))
        assert fs.feat_dim() == D
        what = "D=%d L=%d R=%d" % (D, L, R)
        raw = [bit_patterns(T, D, u) for u, T in enumerate(FRAMES)]
        fs.set_features(raw)
        fs.score(0.1)
        assert fs.num_utts() == len(FRAMES) and fs.total_frames() == sum(FRAMES)
        for u, x in enumerate(raw):
            assert fs.num_frames(u) == x.shape[0]
            got = fs.fetch_cmvn(u)
            assert got.shape == x.shape and np.array_equal(got.view(np.uint32), x.view(np.uint32)), "%s utterance %d" % (what, u)
        with pytest.raises(pk.PkCodeError) as e:
            fs.fetch_fbank(1)
        assert e.value.code == E_STATE
        # the same scorer, finite features: first and last frame replicated into pads of any width, T below the context
        feats = [finite(T, D, 100 + u) for u, T in enumerate(FRAMES)]
        fs.set_features(feats)
        fs.score(0.1)
        assert_rows_are_decodables(am, fs, feats, what)
        fs.close()
        am.close()


# ---------------------------------------------------------------- scores: both GEMM routes, both softmax modes

@pytest.mark.parametrize("softmax", ["stable", "reference"])
@pytest.mark.parametrize("layout", ["B", "C"])
def test_scores_equal_decodable_big_tiles_compact_rows_fused_tail(layout, softmax, monkeypatch):
    """Model S, isolation_cases' layouts B (2 116 compact rows: the fused tail with its strip launch) and C (6 292: big
    tiles in every layer), with a frameless utterance in between; the knob puts the fused route's threshold at 64 tiles
    for B so that it does not hang on the default."""
    if layout == "B":
        monkeypatch.setenv("PK_MI355_FUSED_TAIL_MIN_TILES", "64")
    layers, prior, L, R = synth.model("S")
    am = pk.AcousticModel(layers, prior, L, R).set_softmax(softmax)
    frames = [T for T, _ in IC.LAYOUTS[layout][1]]
    frames.insert(2, 0)
    feats = [finite(T, 40, 200 + u) for u, T in enumerate(frames)]
    fs = pk.FeatureScorer(am, len(feats), sum(frames))
    fs.set_features(feats)
    fs.enable_timing(True)
    fs.score(0.1)
    t = fs.timing()
    assert t["fbank"][1] == 0 and t["cmvn"][1] == 1 and t["gemm"][1] >= 1, t          # the layout launch sits in the CMVN slot
    assert_rows_are_decodables(am, fs, feats, "model S layout %s %s" % (layout, softmax))
    views = fs.fetch_all()
    for u, v in enumerate(views):
        assert bits_equal(v.log_prob(), fs.fetch(u).log_prob()) or frames[u] == 0
        v.destroy()
    fs.close()


def test_f16x3_within_the_contract_of_the_oracle():
    layers, prior, L, R = synth.model("S")
    am = pk.AcousticModel(layers, prior, L, R, precision="f16x3")
    feats = [finite(T, 40, 300 + u, sigma=2.0) for u, T in enumerate((211, 0, 130, 5))]
    fs = pk.FeatureScorer(am, len(feats), sum(f.shape[0] for f in feats))
    fs.set_features(feats)
    fs.calibrate()                                           # pk_mi355_batch_calibrate on a features batch
    fs.score(0.1)
    nn = O.Nnet(layers)
    worst = 0.0
    for u, f in enumerate(feats):
        got = fs.fetch(u).log_prob()
        if f.shape[0] == 0:
            assert got.shape[0] == 0
            continue
        ref = nn.am_compute(f, prior, L, R, 0.1)
        worst = max(worst, float((np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)).max()))
        print("FEATURES_F16X3_MAX_ERR utterance %d: %.3e" % (u, worst))
        assert_loglik_close(got, ref)
    print("FEATURES_F16X3_MAX_ERR %.3e (contract 1e-4)" % worst)
    fs.close()


# ---------------------------------------------------------------- RAW

_wave_stages = {}


def wave_stages(which, prec="f32"):
    """(am, stats, waves, fbank, cmvn, log-likelihoods) of a fixed set of waves through a fresh wave scorer: 705 frames
    (the CMVN window slides), 1 frame, 300 samples (no frame), 130 frames.  Made once, shared, left unchanged."""
    if (which, prec) not in _wave_stages:
        layers, prior, L, R = synth.model(which)
        am = pk.AcousticModel(layers, prior, L, R, precision=prec)
        g = synth.global_cmvn_stats()
        waves = [IC.healthy(7001, 705), IC.healthy(7002, 1), IC.healthy(7003, 3)[:300], IC.healthy(7004, 130)]
        bs = pk.BatchScorer(am, g, len(waves), sum(len(w) for w in waves))
        bs.set_waves(waves)
        if prec != "f32":
            bs.calibrate()
        bs.score(0.1)
        n = len(waves)
        assert [bs.num_frames(u) for u in range(n)] == [705, 1, 0, 130]
        _wave_stages[(which, prec)] = (am, g, waves, [bs.fetch_fbank(u) for u in range(n)], [bs.fetch_cmvn(u) for u in range(n)],
                                       fetch_rows(bs), bs)
    return _wave_stages[(which, prec)]


def assert_stages(bs, fb, cm, ll, what, fbank=True):
    assert bs.num_utts() == len(ll)
    for u in range(len(ll)):
        assert bits_equal(bs.fetch_cmvn(u), cm[u]), "%s utterance %d: CMVN differs" % (what, u)
        assert bits_equal(bs.fetch(u).log_prob(), ll[u]), "%s utterance %d: log-likelihoods differ" % (what, u)
        if fbank:
            assert bits_equal(bs.fetch_fbank(u), fb[u]), "%s utterance %d: fbank differs" % (what, u)


def test_raw_features_are_the_wave_calls_fbank():
    am, g, waves, fb, cm, ll, same = wave_stages("tiny")
    total = sum(f.shape[0] for f in fb)
    second = pk.BatchScorer(am, g, len(waves), sum(len(w) for w in waves))
    featured = pk.FeatureScorer(am, len(waves), total, global_stats=g)
    for name, bs in (("the same scorer", same), ("a second wave scorer", second), ("a FeatureScorer with stats", featured)):
        bs.set_features(fb, kind="raw")
        bs.enable_timing(True)
        bs.score(0.1)
        t = bs.timing()
        assert t["fbank"][1] == 0 and t["cmvn"][1] == 1, (name, t)
        assert_stages(bs, fb, cm, ll, name)
        # ... and NORMALIZED features that are the wave call's CMVN give the wave call's rows
        bs.set_features(cm, kind="normalized")
        bs.score(0.1)
        assert_stages(bs, fb, cm, ll, name + ", normalized", fbank=False)
    same.set_waves(waves)                                    # a later set_waves switches a wave batch back
    same.enable_timing(True)
    same.score(0.1)
    assert same.timing()["fbank"][1] == 1
    assert_stages(same, fb, cm, ll, "back to waves")
    second.close()
    featured.close()


# ---------------------------------------------------------------- the device entry

@pytest.mark.parametrize("D,kind", [(39, "normalized"), (40, "normalized"), (40, "raw")])
def test_device_entry_equals_the_host_entry(D, kind):
    L = pk.lib()
    if kind == "raw":
        am, g, _, feats, _, _, _ = wave_stages("tiny")
    else:
        am, g = tiny(D, 2, 1)[0], None
        feats = [finite(T, D, 400 + u) for u, T in enumerate((65, 0, 7, 129))]
    frames = [f.shape[0] for f in feats]
    host = pk.FeatureScorer(am, len(feats), sum(frames), global_stats=g)
    host.set_features(feats, kind=kind)
    host.score(0.1)
    want = fetch_rows(host)
    cat = np.ascontiguousarray(np.concatenate(feats))
    # one row into the allocation: for D = 39 the first row is 4-byte aligned and no better
    ptr = L.pk_mi355_device_malloc(cat.nbytes + 4 * D)
    assert ptr
    try:
        assert L.pk_mi355_memcpy(C.c_void_p(ptr + 4 * D), cat.ctypes.data_as(C.c_void_p), cat.nbytes, 1) == 0
        assert (ptr + 4 * D) % 8 != 0 or D != 39
        dev = pk.FeatureScorer(am, len(feats), sum(frames), global_stats=g)
        dev.set_features_device(ptr + 4 * D, frames, kind=kind)
        dev.score(0.1)
        got = fetch_rows(dev)
        for u in range(len(feats)):
            assert bits_equal(got[u], want[u]), (D, kind, u)
            assert bits_equal(dev.fetch_cmvn(u), host.fetch_cmvn(u)), (D, kind, u)
        assert any(w.size for w in want)
        dev.close()
    finally:
        L.pk_mi355_device_free(C.c_void_p(ptr))
    host.close()


# ---------------------------------------------------------------- reuse and isolation

@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_one_scorer_alternating_waves_and_features(prec):
    """One wave scorer takes waves, raw and normalised features in turn, large layouts before small ones, with a
    NaN-filled call (and in f16x3 a loud one, sigma = 3e4) in between: every healthy call is the fresh scorer's, bit
    for bit, and the healthy f16x3 call after the loud one does not fail its range check."""
    am, g, waves, fb, cm, ll, _ = wave_stages("tiny", prec)
    order = {"large": [0, 1, 2, 3], "small": [3, 2, 1], "one": [1], "none": []}
    bs = pk.BatchScorer(am, g, 4, sum(len(w) for w in waves))
    frames = [f.shape[0] for f in fb]

    def poison(how):
        if how == "nan_features":
            bs.set_features([np.full((T, 40), np.nan, np.float32) for T in frames], kind="normalized")
        elif how == "nan_waves":
            bs.set_waves([np.full(len(w), np.nan, np.float32) for w in waves])
        else:
            bs.set_features([finite(T, 40, 500 + u, sigma=IC.LOUD_SIGMA) for u, T in enumerate(frames)], kind="normalized")
        try:
            bs.score(0.1)
            rows = fetch_rows(bs)
        except pk.PkError as e:
            assert prec != "f32" and "range" in str(e), e
            return
        if prec == "f32" and how != "loud":
            assert all(np.isnan(r).all() for r in rows)

    def healthy(source, which):
        pick = order[which]
        if source == "waves":
            bs.set_waves([waves[u] for u in pick])
        else:
            bs.set_features([(fb if source == "raw" else cm)[u] for u in pick], kind=source)
        bs.score(0.1)                                        # (f16x3: PK_MI355_E_RANGE would raise here)
        assert_stages(bs, [fb[u] for u in pick], [cm[u] for u in pick], [ll[u] for u in pick],
                      "%s %s %s" % (prec, source, which), fbank=source != "normalized")

    poisons = ["nan_features", "nan_waves"] + (["loud"] if prec != "f32" else [])
    k = 0
    for which in ("large", "small", "one", "none", "large"):
        for source in ("normalized", "waves", "raw"):
            poison(poisons[k % len(poisons)])
            k += 1
            healthy(source, which)
    bs.close()


def test_a_poisoned_neighbour_changes_no_bit():
    am, _, _ = tiny(40, 5, 5)
    layout = IC.LAYOUTS["A"][1]
    feats = [np.full((T, 40), np.nan, np.float32) if bad else finite(T, 40, 600 + u) for u, (T, bad) in enumerate(layout)]
    fs = pk.FeatureScorer(am, len(feats), sum(T for T, _ in layout))
    fs.set_features(feats)
    fs.score(0.1)
    healthy = [np.zeros((0, 40), np.float32) if bad else f for f, (_, bad) in zip(feats, layout)]
    got = fetch_rows(fs)
    for u, (T, bad) in enumerate(layout):
        if bad:
            assert got[u].shape == (T, am.num_pdfs()) and np.isnan(got[u]).all(), u
        elif T:
            assert bits_equal(got[u], decodable_rows(am, healthy[u])), u
    fs.close()


# ---------------------------------------------------------------- errors

def matrix(a, nrow=None, ncol=None):
    m = pk.pk_matrix_t()
    m.ncol, m.nrow = a.shape
    m.data = a.ctypes.data_as(C.POINTER(C.c_float))
    if nrow is not None:
        m.nrow = nrow
    if ncol is not None:
        m.ncol = ncol
    return m


def test_every_failure_code_and_the_scorer_stays_usable():
    L = pk.lib()
    am, g, waves, fb, cm, ll, _ = wave_stages("tiny")
    x = finite(6, 40, 700)
    n6 = (C.c_int * 2)(6, 6)
    wave_bs = pk.BatchScorer(am, g, 2, 16000)                # 102 frames of capacity
    plain = pk.FeatureScorer(am, 2, 100)                     # no statistics
    with_stats = pk.FeatureScorer(am, 2, 100, global_stats=g)

    def code(rc, want):
        assert rc == want and L.pk_mi355_last_error_code() == want, (rc, L.pk_mi355_last_error())
        return L.pk_mi355_last_error().decode()

    assert wave_bs.feat_dim() == plain.feat_dim() == 40
    with pytest.raises(pk.PkError):                          # nothing set yet
        plain.score(0.1)
    assert L.pk_mi355_last_error_code() == E_STATE
    plain.set_features([x, x[:3]])
    plain.score(0.1)
    before = fetch_rows(plain)
    for bs in (wave_bs, plain, with_stats):
        h = bs._h
        code(L.pk_mi355_features_set(h, None, 1, 0), E_INVALID)
        msg = code(L.pk_mi355_features_set(h, C.byref(matrix(x, nrow=39)), 1, 0), E_INVALID)
        assert "39" in msg and "40" in msg, msg              # both are named, as pk_decodable_init names them
        code(L.pk_mi355_features_set(h, C.byref(matrix(x, ncol=-1)), 1, 0), E_INVALID)
        for kind in (2, -1):
            code(L.pk_mi355_features_set(h, C.byref(matrix(x)), 1, kind), E_INVALID)
            code(L.pk_mi355_features_set_device(h, C.c_void_p(16), n6, 1, kind), E_INVALID)
        three = (pk.pk_matrix_t * 3)(matrix(x), matrix(x), matrix(x))
        code(L.pk_mi355_features_set(h, three, 3, 0), E_INVALID)                       # utterances
        big = finite(103, 40, 701)
        code(L.pk_mi355_features_set(h, C.byref(matrix(big)), 1, 0), E_INVALID)       # frames
        code(L.pk_mi355_features_set_device(h, None, n6, 2, 0), E_INVALID)
        code(L.pk_mi355_features_set_device(h, C.c_void_p(16), None, 2, 0), E_INVALID)
        code(L.pk_mi355_features_set_device(h, C.c_void_p(16), (C.c_int * 2)(6, -1), 2, 0), E_INVALID)
        code(L.pk_mi355_features_set_device(h, C.c_void_p(16), (C.c_int * 2)(60, 60), 2, 0), E_INVALID)
    assert plain.num_utts() == 2 and all(bits_equal(a, b) for a, b in zip(fetch_rows(plain), before))   # nothing was touched
    # RAW needs the statistics and 40 dimensions
    code(L.pk_mi355_features_set(plain._h, C.byref(matrix(x)), 1, 1), E_INVALID)
    code(L.pk_mi355_features_set_device(plain._h, C.c_void_p(16), n6, 1, 1), E_INVALID)
    am39, _, _ = tiny(39, 1, 1)
    with pytest.raises(pk.PkCodeError) as e:
        pk.FeatureScorer(am39, 2, 100, global_stats=g)
    assert e.value.code == E_INVALID
    with pytest.raises(pk.PkCodeError) as e:
        pk.FeatureScorer(am, 0, 100)
    assert e.value.code == E_INVALID
    am39h, _, _ = tiny(39, 1, 1, precision="f16x3")
    with pytest.raises(pk.PkCodeError) as e:                 # the f16 modes' spliced view needs a multiple of 8
        pk.FeatureScorer(am39h, 2, 100)
    assert e.value.code == E_INVALID
    with pytest.raises(pk.PkError):                          # the wave scorer still refuses such a model
        pk.BatchScorer(am39, g, 2, 16000)
    # wave entries on a features-only batch
    wave = pk.pk_vector_t(len(waves[1]), waves[1].ctypes.data_as(C.POINTER(C.c_float)))
    n1 = (C.c_int * 1)(len(waves[1]))
    i16 = waves[1].astype(np.int16)
    for bs in (plain, with_stats):
        code(L.pk_mi355_batch_set_waves(bs._h, C.byref(wave), 1), E_STATE)
        code(L.pk_mi355_resample_set_waves(bs._h, C.byref(wave), (C.c_int * 1)(8000), 1), E_STATE)
        code(L.pk_mi355_batch_set_waves_i16(bs._h, i16.ctypes.data_as(C.POINTER(C.c_int16)), n1, 1), E_STATE)
        code(L.pk_mi355_batch_set_waves_device(bs._h, C.c_void_p(16), n1, 1), E_STATE)
    # no fbank after NORMALIZED; the input after RAW
    out = np.zeros((6, 40), np.float32)
    code(L.pk_mi355_batch_fetch_fbank(plain._h, 0, out.ctypes.data_as(C.POINTER(C.c_float))), E_STATE)
    with_stats.set_features([x], kind="raw")
    with_stats.score(0.1)
    assert bits_equal(with_stats.fetch_fbank(0), x)
    with_stats.set_features([x], kind="normalized")
    with_stats.score(0.1)
    code(L.pk_mi355_batch_fetch_fbank(with_stats._h, 0, out.ctypes.data_as(C.POINTER(C.c_float))), E_STATE)
    # after all these failures: usable
    plain.set_features([x])
    plain.score(0.1)
    assert bits_equal(plain.fetch(0).log_prob(), decodable_rows(am, x))
    wave_bs.set_features([fb[3][:100]], kind="raw")
    wave_bs.score(0.1)
    assert wave_bs.num_frames(0) == 100 and np.isfinite(wave_bs.fetch(0).log_prob()).all()
    # nothing but frameless utterances
    plain.set_features([np.zeros((0, 40), np.float32)] * 2)
    plain.score(0.1)
    assert plain.num_utts() == 2 and plain.total_frames() == 0
    assert [plain.fetch(u).log_prob().shape[0] for u in range(2)] == [0, 0]
    views = plain.fetch_all()
    assert [v.log_prob().shape[0] for v in views] == [0, 0]
    for v in views:
        v.destroy()
    for bs in (wave_bs, plain, with_stats):
        bs.close()


# ---------------------------------------------------------------- downstream: decoder, recognizer, command line

def test_decode_batch_of_a_feature_batch_equals_decode_of_its_fetch_all():
    from refmodel_text import DIR, load_text_model
    from test_gpu_decoder import G
    layers, prior, Lc, Rc, tid2pdf, cmvn41 = load_text_model()
    am = pk.AcousticModel(layers, prior, Lc, Rc, tid2pdf)
    hello, cat = (pk.read_wav(os.path.join(G, w)) for w in ("en-us-hello.wav", "en-us-cat.wav"))
    waves = [hello, cat, np.ascontiguousarray(hello[:300]), np.ascontiguousarray(cat[2000:9000]), np.ascontiguousarray(hello[500:4321])]
    wb = pk.BatchScorer(am, cmvn41, len(waves), sum(len(w) for w in waves))
    wb.set_waves(waves)
    wb.score(0.1)
    feats = [wb.fetch_cmvn(u) for u in range(len(waves))]
    assert feats[2].shape[0] == 0
    fs = pk.FeatureScorer(am, len(feats), sum(f.shape[0] for f in feats))
    fs.set_features(feats)
    fs.score(0.1)
    fst_path = os.path.join(DIR, "wordloop.fst")
    fst = pk.Fst(fst_path)
    dec = pk.Decoder(fst, am, 16, trace_capacity=TRACE)
    dec.set_alignment(True)
    dec.decode_batch(fs)
    lls = [v.log_prob() for v in fs.fetch_all()]
    host = pk.Decoder(fst, am, len(feats), trace_capacity=TRACE)
    host.set_alignment(True)
    host.decode(lls)
    arcs = flat_arcs(fst_path)
    for u, ll in enumerate(lls):
        assert bits_equal(ll, wb.fetch(u).log_prob()) or ll.shape[0] == 0
        assert outcome(dec, u) == outcome(host, u), u
        assert check_alignment(dec, u, arcs, ll, lambda t: int(tid2pdf[t])) == check_alignment(host, u, arcs, ll, lambda t: int(tid2pdf[t]))
        for a, b in zip(dec.alignment(u), host.alignment(u)):
            assert a.tobytes() == b.tobytes()
        assert got_segments(dec, u) == got_segments(host, u)
    assert len(dec.alignment(0)[0]) == lls[0].shape[0] > 0 and dec.result(0)[0]


def fields(r):
    f32 = lambda v: np.float32(v).tobytes()
    return (r.text, r.words, f32(r.weight), r.ok, f32(r.loglikelihood_per_frame),
            [tuple(s[:3]) + (f32(s[3]), f32(s[4])) for s in r.segments])


def test_recognizer_from_features_equals_the_recognizer_from_waves():
    from test_gpu_recognizer import CAT, CONF, HELLO
    hello, cat = pk.read_wav(HELLO), pk.read_wav(CAT)
    waves = [hello, cat, np.ascontiguousarray(hello[:300]), np.ascontiguousarray(cat[:6000]), np.ascontiguousarray(hello[1000:])]
    rec = pk.Recognizer(CONF, max_utts=2, max_total_samples=len(hello) + len(cat), trace_capacity=TRACE)
    want, fb = [], []
    for w in waves:                                          # one at a time: the batch holds the wave's fbank afterwards
        want += rec.process([w])
        fb.append(rec.batch.fetch_fbank(0))
    assert want[0].text and want[1].text and want[2].text == "" and fb[2].shape == (0, 40)
    got = rec.process_features(fb, "raw")                    # five utterances, two per call: three calls
    assert len(got) == len(want)
    for u, (a, b) in enumerate(zip(got, want)):
        assert fields(a) == fields(b), u
    assert [fields(r) for r in rec.process_features(fb[:2])] == [fields(r) for r in want[:2]]     # (kind defaults to raw)
    with pytest.raises(pk.PkError, match="frames"):          # a single matrix that cannot fit is refused, nothing is cut
        rec.process_features([np.zeros((rec.max_total_samples // 160 + 3, 40), np.float32)])
    with pytest.raises(pk.PkError):
        rec.process_features([np.zeros((5, 39), np.float32)])
    assert [fields(r) for r in rec.process_features(fb[:1])] == [fields(want[0])]                   # still usable
    rec.close()


def test_command_line_on_an_npz_prints_the_wave_files_lines(tmp_path):
    from test_gpu_recognizer import CAT, CONF, HELLO
    rec = pk.Recognizer(CONF, max_utts=1, max_total_samples=200000)
    fb = {}
    for name, path in (("hello", HELLO), ("cat", CAT)):
        rec.process([pk.read_wav(path)])
        fb[name] = rec.batch.fetch_fbank(0)
    rec.close()
    npz, npy, scp = str(tmp_path / "feats.npz"), str(tmp_path / "hello.npy"), str(tmp_path / "waves.scp")
    np.savez(npz, **fb)
    np.save(npy, fb["hello"])
    with open(scp, "w") as f:
        f.write(HELLO + "\n" + CAT + "\n")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(*args):
        p = subprocess.run([sys.executable, "-m", "pocketkaldi_amd.recognize", CONF] + list(args), capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stdout + p.stderr
        return p.stdout

    def renamed(text, sep):
        return [l.replace(HELLO + sep, "hello" + sep, 1).replace(CAT + sep, "cat" + sep, 1) for l in text.splitlines()]

    plain = None
    for flags, sep in (([], "\t"), (["--ctm"], " ")):
        from_waves = run(scp, *flags)
        from_feats = run(npz, "--features", "raw", *flags)
        assert from_feats.splitlines() == renamed(from_waves, sep) and len(from_feats.splitlines()) >= 2
        plain = plain or from_feats.splitlines()
    assert run(npy, "--features", "raw").splitlines() == [plain[0].replace("hello\t", npy + "\t", 1)]
