"""The log-likelihood tail kernels on designed logits (tests/tail_cases.py): a row maximum in every edge column of every
TailWaveRows instantiation, flat rows whose sum is an exact integer, rows that straddle the floor, wide and shifted
spreads with distinct priors, infinite and out-of-range logits, 1 to 8 195 rows per call -- against exact bit predictions
where the arithmetic cannot round and against a float64 reference under a bound derived from the kernels' operations
(tests/tail_model.py) everywhere else.  test_tail_cases.py shows on a model of the kernel that this assertion catches a
dropped or doubled column, a wave half left out, an unwritten last column, a missing floor and a misplaced prior.

Routes.  The environment switches are read when the model object is made, so each test sets them first.  The
single-utterance entry cannot say which kernel ran; the route is derived from the documented rules
(tail_cases.fused_route, tail_model.wave_shape / kernel_cache) and named in every failure message.

Not reached from here, and why:
  * TailWaveKernel<..., LDS_PRIOR = true> needs more than 8 * 8192 * per_wg rows in one launch (262 144, pair form
    131 072); the fused route runs the same TailWaveLdsPrior.
  * iters >= 2 of the stand-alone wave tail (more than 8192 * per_wg rows in ONE launch, the prefetch into nv[]):
    pk_decodable_init takes any number of frames but walks them in passes of 4 096, so a launch never holds more.  The
    many-row test below therefore runs two full passes and a 3-row one; only the batch scorer (audio in, no designed
    logits) makes longer launches (test_gpu_parity.py: the full-size batch tests).
  * The fused form at 1 000 and 1 024 columns (C = 4): 8 column tiles need 48 row tiles = 6 144 rows in one launch.
    test_gpu_parity.py::test_fp32_fused_tail_equals_the_stand_alone_wave_tail reaches it through the batch scorer.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pocketkaldi_amd as pk
from oracle import oracle as O

import tail_cases as C
import tail_model as M

ENV = {"wave": {"PK_MI355_FUSED_TAIL32": "1", "PK_MI355_FUSED_TAIL_MIN_TILES": "100000000"},
       "fused": {"PK_MI355_FUSED_TAIL32": "1", "PK_MI355_FUSED_TAIL_MIN_TILES": "384"},
       "kernel": {"PK_MI355_FUSED_TAIL32": "0"}}
FUSED_WIDTHS = [n for n in C.FUSED_WIDTHS if C.fused_row_counts(n)]


def make_model(monkeypatch, route, case, prior_kind, precision="f32", softmax=True, relu=False):
    for k, v in ENV[route].items():
        monkeypatch.setenv(k, v)
    pad = 8 if precision != "f32" else 1
    layers = C.layers(case, identity_first=(route == "fused"), softmax=softmax, pad_k=pad) + ([("relu",)] if relu else [])
    return pk.AcousticModel(layers, C.prior(case["n"], prior_kind), 0, 0, precision=precision), layers, pad


def score(am, case, scale, rows, pad=1):
    d = pk.Decodable(am, scale, C.features(case, rows, pad))
    out = d.log_prob().copy()
    d.destroy()
    return out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def report(name, worst):
    print("TAIL_EDGES_RATIO %s %.4f" % (name, worst))
    assert worst <= 1.0, "%s: largest err / bound %.3f" % (name, worst)


def wave_name(n):
    return "TailWaveRows<C=%d, PAIR=%d, EXACT=%d>" % M.wave_shape(n)


# ------------------------------------------------------------------ the stand-alone wave tail

@pytest.mark.parametrize("n", C.STANDALONE_WIDTHS)
def test_stand_alone_wave_tail(n, monkeypatch):
    case = C.main_case(n)
    P = case["X"].shape[0]
    where = "stand-alone " + wave_name(n)
    worst = 0.0
    for prior_kind in ("ones", "varied"):
        am, _, _ = make_model(monkeypatch, "wave", case, prior_kind)
        for scale in C.SCALES:
            worst = max(worst, C.check(case, score(am, case, scale, P), scale, prior_kind, "wave", where))
        if n in (700, 4097) and prior_kind == "varied":                   # launches of fewer rows than a workgroup holds, and a few more
            for rows in (1, 2, 3, 5, 7):
                worst = max(worst, C.check(case, score(am, case, 0.1, rows), 0.1, prior_kind, "wave", "%s, %d rows" % (where, rows)))
        am.close()
    for name, inf in C.infinite_cases(n):
        am, _, _ = make_model(monkeypatch, "wave", inf, "varied")
        worst = max(worst, C.check(inf, score(am, inf, 0.1, 5), 0.1, "varied", "wave", "%s, bias %s" % (where, name)))
        am.close()
    report(where, worst)


@pytest.mark.parametrize("n", [700, 4097])
def test_stand_alone_wave_tail_over_several_passes(n, monkeypatch):
    """pk_decodable_init takes any number of frames and walks them in passes of 4 096 (see the module docstring): two full
    passes -- 1 024 (2 048 in the pair form) workgroups each -- and one of three rows, every row compared with the
    predicted bits of its pattern, tile by tile."""
    case = C.peaks_case(n)
    am, _, _ = make_model(monkeypatch, "wave", case, "varied")
    got = score(am, case, 0.1, 2 * C.SINGLE_PASS_ROWS + 3)
    am.close()
    assert got.shape[0] == 2 * C.SINGLE_PASS_ROWS + 3
    C.check(case, got, 0.1, "varied", "wave", "stand-alone %s, 8 195 rows" % wave_name(n))


# ------------------------------------------------------------------ the tail inside the last GEMM launch

@pytest.mark.parametrize("n", FUSED_WIDTHS)
def test_fused_tail(n, monkeypatch):
    """Behind an identity layer the last affine layer writes frame-major rows and, from 384 tiles on, finishes them
    itself.  The fewest row tiles that fuse, the last one holding a single row and full; where the 64 x 64 strip launch
    writes the last columns ahead of the fused launch, the same again with the fewest row tiles at which it joins in.
    The stand-alone wave tail must return the same bits for the same model."""
    case = C.main_case(n)
    worst = 0.0
    for i, rows in enumerate(C.fused_row_counts(n)):
        route = C.fused_route(rows, n)
        assert route != "wave" and C.fused_route(rows, n, 100000000) == "wave"
        where = "%s %s, %d rows" % (route, wave_name(n), rows)
        for prior_kind, scale in (("ones", 0.125), ("varied", 0.1)):
            am, _, _ = make_model(monkeypatch, "fused", case, prior_kind)
            got = score(am, case, scale, rows)
            am.close()
            worst = max(worst, C.check(case, got, scale, prior_kind, "wave", where))
        monkeypatch.setenv("PK_MI355_FUSED_TAIL_MIN_TILES", "100000000")      # (make_model sets the others)
        layers = C.layers(case, identity_first=True)
        am = pk.AcousticModel(layers, C.prior(n, "varied"), 0, 0)
        alone = score(am, case, 0.1, rows)
        am.close()
        assert bits_equal(got, alone), where + ": differs from the stand-alone wave tail"
        if i == 0:
            for name, inf in C.infinite_cases(n):
                am, _, _ = make_model(monkeypatch, "fused", inf, "varied")
                worst = max(worst, C.check(inf, score(am, inf, 0.1, rows), 0.1, "varied", "wave", "%s, bias %s" % (where, name)))
                am.close()
    report("fused " + wave_name(n), worst)


# ------------------------------------------------------------------ TailKernel / TailWideKernel

def kernel_name(n):
    k = M.kernel_cache(n)
    return "TailWideKernel" if k == "wide" else "TailKernel<%d>" % k


@pytest.mark.parametrize("n", C.KERNEL_WIDTHS)
def test_workgroup_per_row_tail(n, monkeypatch):
    case = C.main_case(n)
    P = case["X"].shape[0]
    where = kernel_name(n)
    worst = 0.0
    for prior_kind in ("ones", "varied"):
        am, _, _ = make_model(monkeypatch, "kernel", case, prior_kind)
        for scale in C.SCALES:
            worst = max(worst, C.check(case, score(am, case, scale, P), scale, prior_kind, "kernel", where))
        am.close()
    for name, inf in C.infinite_cases(n):
        am, _, _ = make_model(monkeypatch, "kernel", inf, "varied")
        worst = max(worst, C.check(inf, score(am, inf, 0.1, 5), 0.1, "varied", "kernel", "%s, bias %s" % (where, name)))
        am.close()
    report(where, worst)


@pytest.mark.parametrize("n", C.PLAIN_WIDTHS)
def test_plain_tail_without_a_softmax_layer(n, monkeypatch):
    """kTailLoglik: a ReLU net's non-negative outputs, floored at 1e-20; the device logf is the C library's restated, so
    the oracle's bits are owed."""
    case = C.plain_case(n)
    P = case["X"].shape[0]
    am, layers, _ = make_model(monkeypatch, "kernel", case, "varied", softmax=False, relu=True)
    got = score(am, case, 0.1, P)
    am.close()
    want = O.Nnet(layers).am_compute(C.features(case, P), C.prior(n, "varied"), 0, 0, 0.1)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s, plain tail, n=%d: %d values differ, first at %s: got %r, want %r" % (
        kernel_name(n), n, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def test_f16x3_peaks_through_the_workgroup_tail(monkeypatch):
    """The f16 modes take TailKernel; 0, -32 and -64 are exact in the (hi, lo) split, so the predicted bits are owed."""
    n = 3000
    case = C.f16_case(n)
    P = case["X"].shape[0]
    for prior_kind in ("ones", "varied"):
        am, _, pad = make_model(monkeypatch, "wave", case, prior_kind, precision="f16x3")
        for scale in C.SCALES:
            C.check(case, score(am, case, scale, P, pad), scale, prior_kind, "kernel", "f16x3 " + kernel_name(n))
        am.close()


# ------------------------------------------------------------------ the reference-exact kernels

@pytest.mark.parametrize("n", C.REFERENCE_WIDTHS)
def test_reference_mode_returns_the_oracles_bits(n, monkeypatch):
    case = C.reference_case(n)
    P = case["X"].shape[0]
    rows = 2 * P + 3
    for prior_kind in ("ones", "varied"):
        am, layers, _ = make_model(monkeypatch, "wave", case, prior_kind)
        am.set_softmax("reference")
        for scale in C.SCALES:
            got = score(am, case, scale, rows)
            want = O.Nnet(layers).am_compute(C.features(case, rows), C.prior(n, prior_kind), 0, 0, scale)
            bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, "%s, n=%d, prior %s, scale %g: %d values differ, first at %s: got %r, want %r" % (
                "TailExactRegKernel" if n <= 3008 else "TailExactKernel", n, prior_kind, scale, len(bad), tuple(bad[0]),
                got[tuple(bad[0])], want[tuple(bad[0])])
        am.close()


# ------------------------------------------------------------------ past the stable tail's domain

@pytest.mark.parametrize("route,n", [("wave", 700), ("wave", 1024), ("wave", 4097), ("wave", 8192), ("fused", 3072), ("fused", 8000),
                                     ("kernel", 1025), ("kernel", 8193)])
def test_documented_limit_row_maxima_past_flt_max_over_log2e(route, n, monkeypatch):
    """RECORDS A DOCUMENTED LIMIT (pk_tail_wave.h), it does not state what should be: the wave form's domain
    is |x| < FLT_MAX / log2 e = 2.36e38, because -m * log2 e is a float product.  A row whose maximum is 2.5e38 comes out
    all +inf (every exponent argument is -inf: s = 0).  A row whose maximum is -2.5e38 comes out all floor (arguments
    +inf: lse = +inf) where every column a wave holds is real, and all NaN where one is selected to -inf (-inf + inf).
    TailKernel computes expf(v - m) and is right.  An ordinary row between them is untouched."""
    case = C.range_case(n)
    am, _, _ = make_model(monkeypatch, route, case, "ones")
    rows = C.fused_row_counts(n)[0] if route == "fused" else 3
    got = score(am, case, 0.125, rows)
    am.close()
    floor = np.full(n, M.FLOOR32 * np.float32(0.125), np.float32)
    ordinary = np.full(n, np.float32(-np.log(np.float64(n)) * 0.125), np.float32)
    for r in range(rows):
        g, p = got[r], r % 3
        if p == 2:
            assert np.all(np.abs(g - ordinary) <= 4 * M.ulp32(ordinary)), (route, n, r)
        elif route == "kernel" and p == 0:                             # right: the peak's t is 0, the rest is floored
            assert g[0] == 0.0 and bits_equal(g[1:], floor[1:]), (route, n, r)
        elif route == "kernel":                                        # right: -2.5e38 + log(n - 1) is -2.5e38 in float and in double
            assert np.all(g[:n - 1] == 0.0) and g[n - 1] == floor[0], (route, n, r)
        elif p == 0:
            assert np.all(g == np.inf), (route, n, r, "all +inf")
        elif n % 1024 == 0:
            assert bits_equal(g, floor), (route, n, r, "all floor")
        else:
            assert np.isnan(g).all(), (route, n, r, "all NaN")
