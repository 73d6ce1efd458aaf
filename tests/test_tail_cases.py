"""The designed tail cases (tests/tail_cases.py) and the model of the wave tail (tests/tail_model.py), without a GPU:
the logits reach the tail bit for bit, the fault-free model passes the very assertion test_gpu_tail_edges.py applies to
the GPU, every named fault fails it, and the exact bit predictions lie inside the bound around the float64 reference.
That the suite would notice a subtly wrong kernel is shown here, on the model, and never by running such a kernel.
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O

import tail_cases as C
import tail_model as M

WAVE_WIDTHS = sorted(set(C.STANDALONE_WIDTHS + C.FUSED_WIDTHS))
ALL_WIDTHS = sorted(set(WAVE_WIDTHS + C.KERNEL_WIDTHS + C.REFERENCE_WIDTHS + C.PLAIN_WIDTHS))
# one width per instantiation family: scalar stores, C = 4 ragged and exact, 12 ragged, pair ragged and exact
FAULT_WIDTHS = [5, 700, 1023, 1024, 3001, 4097, 6100, 6144, 8000]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_shapes_at_the_switch_over_points():
    want = {1: (4, False, False), 768: (4, False, False), 769: (4, False, True), 1024: (4, False, True), 1025: (8, False, False),
            1792: (8, False, False), 1793: (8, False, True), 2048: (8, False, True), 2049: (12, False, False),
            2817: (12, False, True), 3072: (12, False, True), 3073: (16, False, False), 3841: (16, False, True),
            4096: (16, False, True), 4097: (12, True, False), 5888: (12, True, False), 5889: (12, True, True),
            6144: (12, True, True), 6145: (16, True, False), 7936: (16, True, False), 7937: (16, True, True),
            8192: (16, True, True)}
    for n, shape in want.items():
        assert M.wave_shape(n) == shape, n
    assert [M.kernel_cache(n) for n in (1, 1024, 1025, 3072, 3073, 8192, 8193)] == [1, 1, 3, 3, 8, 8, "wide"]
    assert C.fused_route(2049, 3000) == "fused+strip" and C.fused_route(1921, 3000) == "fused" and C.fused_route(1920, 3000) == "wave"
    assert C.fused_route(4096, 1024) == "wave" and C.fused_row_counts(1024) == [] and C.fused_row_counts(3072) == [1921, 2048]
    assert C.fused_row_counts(3000) == [1921, 2048, 2049, 2176] and C.fused_row_counts(8000) == [769, 896]


def test_round_f32_is_round_to_nearest_even():
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.standard_normal(300) * 10.0 ** rng.integers(-44, 39, 300),
                         [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 2.0 ** -149 * 0.5, 2.0 ** -149 * 1.5, 3.4028235677973366e38, 0.0]])
    with np.errstate(over="ignore"):
        for x in xs:
            assert bits_equal(M.round_f32(Fraction(float(x))), np.float32(x)), x
    a, b, c = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -60)
    want = M.round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))
    assert bits_equal(M._fma32(np.array([a]), np.array([b]), np.array([c]))[0], want)


@pytest.mark.parametrize("n", ALL_WIDTHS)
def test_logits_reach_the_tail_bit_for_bit(n):
    """O.Nnet(layers).propagate without the softmax returns the patterns' bits -- one layer, behind an identity layer,
    with an infinite bias, and the ReLU net of the plain tail."""
    case = C.main_case(n)
    P = case["X"].shape[0]
    rows = 2 * P + 1
    want = C.logits(case)[np.arange(rows) % P]
    for ident in (False, True):
        got = O.Nnet(C.layers(case, identity_first=ident, softmax=False)).propagate(C.features(case, rows))
        assert bits_equal(got, want), (n, ident)
    got = O.Nnet(C.layers(case, softmax=False, pad_k=8)).propagate(C.features(case, rows, pad_k=8))
    assert bits_equal(got, want)
    for name, inf in C.infinite_cases(n):
        got = O.Nnet(C.layers(inf, softmax=False)).propagate(C.features(inf, 5))
        assert bits_equal(got, C.logits(inf)), (n, name)
        assert np.isinf(got).any() and not np.isnan(got).any()
    plain = C.plain_case(n)
    got = O.Nnet(C.layers(plain, softmax=False) + [("relu",)]).propagate(C.features(plain, plain["X"].shape[0]))
    assert bits_equal(got, plain["X"]) and (plain["X"] >= 0).all()
    rng = C.range_case(n)
    assert bits_equal(O.Nnet(C.layers(rng, softmax=False)).propagate(C.features(rng, 3)), rng["X"])


def run_model(case, prior_kind, scale, fault=None, rows=None):
    n = case["n"]
    p = C.prior(n, prior_kind)
    x = C.logits(case)
    if rows is not None:
        x = x[np.arange(rows) % x.shape[0]]
    return M.wave_model(x, n, scale, p, fault=fault, log_prior32=C.log_prior32(p))


@pytest.mark.parametrize("n", WAVE_WIDTHS)
def test_the_model_without_a_fault_passes_every_case(n):
    case = C.main_case(n)
    worst = 0.0
    for prior_kind, scale in (("ones", 0.125), ("ones", 0.1), ("varied", 0.1)):
        worst = max(worst, C.check(case, run_model(case, prior_kind, scale), scale, prior_kind, "wave", "model"))
    for name, inf in C.infinite_cases(n):
        worst = max(worst, C.check(inf, run_model(inf, "varied", 0.1), 0.1, "varied", "wave", "model, " + name))
    assert worst <= 1.0
    P = case["X"].shape[0]
    if n in (700, 4097):                                            # fewer rows than patterns, and more
        for rows in (1, 2, 3, 5, 7, 2 * P + 3):
            C.check(case, run_model(case, "varied", 0.1, rows=rows), 0.1, "varied", "wave", "model, %d rows" % rows)


def caught(case, prior_kind, scale, fault):
    try:
        C.check(case, run_model(case, prior_kind, scale, fault=fault), scale, prior_kind, "wave", "model with " + fault)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("fault", M.FAULTS)
def test_every_fault_is_caught(fault):
    """Each named fault fails the GPU test's assertion at every width where it changes what the kernel does."""
    seen = 0
    for n in FAULT_WIDTHS:
        C_, pair, exact = M.wave_shape(n)
        n4 = (n + 3) >> 2
        applies = {"no_select_last": n != 256 * C_ * (2 if pair else 1),
                   "no_select_clamped": n4 < 64 * C_ * (2 if pair else 1),
                   "half1_not_in_max": pair, "half1_not_in_sum": pair,
                   "last_col_unwritten": n % 4 != 0, "no_floor": True, "prior_neighbour": True}[fault]
        prior_kind = "varied" if fault == "prior_neighbour" else "ones"
        hit = caught(C.main_case(n), prior_kind, 0.125, fault)
        assert hit == applies, "fault %s at n = %d: caught %s, changes the kernel %s" % (fault, n, hit, applies)
        seen += hit
    assert seen >= 1


def test_a_prior_from_the_wrong_chunk_needs_distinct_priors():
    """Why the spread family carries distinct priors: with prior = 1 everywhere the fault cannot show."""
    assert not caught(C.main_case(700), "ones", 0.125, "prior_neighbour")
    assert caught(C.main_case(700), "varied", 0.125, "prior_neighbour")


@pytest.mark.parametrize("form", ["wave", "kernel"])
def test_bit_predictions_agree_with_the_reference_inside_the_bound(form):
    for n in (C.STANDALONE_WIDTHS if form == "wave" else C.KERNEL_WIDTHS):
        case = C.peaks_case(n)
        for prior_kind in ("ones", "varied"):
            for scale in C.SCALES:
                p = C.prior(n, prior_kind)
                bits = M.predict_bits(case["t"], C.log_prior32(p), scale, form)
                ref, tol = M.reference(case["X"], p, scale), M.error_bound(case["X"], p, scale, form)
                assert np.all(np.abs(bits.astype(np.float64) - ref) <= tol), (n, prior_kind, scale)
                if prior_kind == "ones" and scale == 0.125:           # a power of two and log prior 0: one answer for both forms
                    assert bits_equal(bits, M.predict_bits(case["t"], C.log_prior32(p), scale, "kernel" if form == "wave" else "wave"))
    p = C.prior(700, "varied")                                       # elsewhere each form has its own
    t = C.peaks_case(700)["t"]
    assert not bits_equal(M.predict_bits(t, C.log_prior32(p), 0.1, "wave"), M.predict_bits(t, C.log_prior32(p), 0.1, "kernel"))


def test_the_model_past_the_domain_does_what_the_header_says():
    """|m| > FLT_MAX / log2 e: -m * log2 e overflows.  m > 0: every exponent argument is -inf, s = 0, the row comes out all
    +inf.  m < 0: the arguments are +inf, s = inf, lse = +inf and the row comes out all floor -- unless the wave holds a
    column selected to -inf (any width that is not 256 C columns per wave), whose argument is -inf + inf: the row is NaN."""
    for n in (700, 1024, 4097, 8192):
        case = C.range_case(n)
        got = run_model(case, "ones", 0.125)
        assert np.all(got[0] == np.inf)
        if n % 1024 == 0:
            assert bits_equal(got[1], np.full(n, M.FLOOR32 * np.float32(0.125), np.float32))
        else:
            assert np.isnan(got[1]).all()
        ref = M.reference(case["X"], C.prior(n, "ones"), 0.125)
        assert ref[0, 0] == 0.0 and np.all(ref[0, 1:] == 0.125 * M.FLOOR) and np.isfinite(ref[1]).all()


def test_what_the_reference_does_with_a_positive_infinite_logit():
    """vector.cc:265-277 + am.cc:106-112: exp(inf) / inf is NaN for that element, 0 / inf is floored for the rest.  The
    stable tail makes the whole row NaN on purpose (pk_tail_wave.h); this is the other side of that choice."""
    name, case = C.infinite_cases(700)[2]
    assert name == "one +inf"
    got = O.Nnet(C.layers(case)).am_compute(C.features(case, 5), C.prior(700, "ones"), 0, 0, 0.125)
    assert np.isnan(got[:, 699]).all() and bits_equal(got[:, :699], np.full((5, 699), M.FLOOR32 * np.float32(0.125), np.float32))
    assert np.isnan(M.reference(C.logits(case), C.prior(700, "ones"), 0.125)).all()
