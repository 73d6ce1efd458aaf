"""The constructions of tests/f16_cases.py, checked on the CPU before test_gpu_f16_exact.py holds the kernels to them:
the exactness guard holds, the split returns the intended halves, the model (tests/f16_model.py) equals the float64
product exactly and equals the fp32 oracle (nnet.cc restated, oracle/pk_oracle.c) bit for bit -- which ties the helper
to the reference -- and a case meant to engage a cross term really does (its hi-only result differs).
"""
import numpy as np
import pytest

import f16_cases as C
import f16_model as M
from oracle import oracle as O


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def exact64(case):
    """The network in float64 on the unscaled inputs (ReLU layers only)."""
    h = case["x"].astype(np.float64)
    for l in case["layers"]:
        if l[0] == "linear":
            h = h @ l[1].astype(np.float64).T + l[2].astype(np.float64)
        elif l[0] == "relu":
            h = np.maximum(h, 0.0)
    return h


def oracle(case):
    return O.Nnet([l for l in case["layers"] if l[0] != "softmax"]).propagate(case["x"])


def check_exact(case, cap=M.SPAN_CAP_LOG2):
    spans, ops = [], []
    got = C.model(case, 3, guard=spans, operands=ops)
    assert len(spans) == C.num_linear(case["layers"]) and max(spans) <= cap
    assert M.operands_in_range(ops)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), exact64(case))
    assert bits_equal(got, oracle(case))
    return got, spans, ops


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", C.AFFINE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_integer_affine_cases(shape, relu):
    case = C.integer_affine(*shape, relu)
    got, spans, ops = check_exact(case)
    assert not ops[0][1].any() and not M.split(case["layers"][0][1] * np.float32(2.0 ** C.w_exps(case["layers"])[0]))[1].any()
    assert bits_equal(C.model(case, 1, guard=[]), got)          # lo = 0 everywhere: plain f16 has the same exact answer
    if relu and got.size > 100:
        assert (got == 0).any() and (got > 0).any()
    for e in (3, -4):                                            # the input exponent moves no bit
        assert bits_equal(C.model(case, 3, guard=[], x_exp=[e]), got)


def test_the_integer_span_at_k_2560_is_what_the_construction_says():
    _, spans, _ = check_exact(C.integer_affine(5, 2560, 257, False))
    assert 16.0 < spans[0] < 18.4


@pytest.mark.parametrize("shape", C.LO_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_w_lo_cases(shape):
    case = C.w_lo_affine(*shape)
    got, spans, ops = check_exact(case)
    W = case["layers"][0][1]
    e_w = M.finalize_exponent(W)
    assert e_w == -case["log2_scale"]
    hi, lo = M.split(W * np.float32(2.0 ** e_w))
    assert np.array_equal(hi, case["w_halves"][0]) and np.array_equal(lo, case["w_halves"][1]) and lo.any()
    assert not ops[0][1].any()
    hi_only = C.model(case, 1, guard=[])
    assert not bits_equal(hi_only, got)                          # the hi x lo term carries part of the answer
    for s in (-20, 6):                                           # the weight scale moves e_w and nothing else
        moved = dict(case, layers=[("linear", W * np.float32(2.0 ** s), case["layers"][0][2] * np.float32(2.0 ** s))])
        assert C.w_exps(moved["layers"])[0] == e_w - s
        assert bits_equal(C.model(moved, 3, guard=[]) * np.float32(2.0 ** -s), got)


@pytest.mark.parametrize("shape", C.LO_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_x_lo_cases(shape):
    case = C.x_lo_affine(*shape)
    got, spans, ops = check_exact(case)
    assert np.array_equal(ops[0][0], case["x_halves"][0]) and np.array_equal(ops[0][1], case["x_halves"][1])
    assert ops[0][1].any()
    assert not M.split(case["layers"][0][1] * np.float32(2.0 ** C.w_exps(case["layers"])[0]))[1].any()
    assert not bits_equal(C.model(case, 1, guard=[]), got)       # the lo x hi term carries part of the answer


def test_the_guard_refuses_what_it_should():
    rng = np.random.default_rng(3)
    hi, lo = C.w_lo_halves(rng, 8, 16)
    xh = C.X_HI[rng.integers(0, 4, size=(4, 16))]
    xl = np.full((4, 16), 1.0 / 16, np.float32)
    with pytest.raises(M.NotExact, match="lo x lo"):
        M.exactness_guard(M.split(xh + xl), M.split(hi + lo), 3)
    M.exactness_guard(M.split(xh + xl), M.split(hi + lo), 1)     # hi only: no lo half takes part
    dense = C.x_lo_affine(33, 520, 130)
    dense["layers"] = [("linear", np.full((130, 520), 2.0, np.float32), np.zeros(130, np.float32))]
    with pytest.raises(M.NotExact, match="cap"):
        C.model(dense, 3, guard=[])
    assert M.lowest_bit(np.array([12.0, 0.0, -0.375, 65504.0])).tolist() == [4.0, np.inf, 0.125, 32.0]


@pytest.mark.parametrize("depth", [2, 3])
def test_small_integer_stacks(depth):
    case = C.small_int_stack(depth)
    got, spans, ops = check_exact(case)
    assert all(e != 0 for e in case["x_exp"][1:])
    assert not any(lo.any() for _, lo in ops)
    assert bits_equal(C.model(case, 1, guard=[]), got)
    assert bits_equal(C.model(case, 3, guard=[], x_exp=[0] * depth), got)
    hidden = ops[1][0]
    assert (hidden == 0).mean() > 0.2 and hidden.max() > 0 and hidden.min() == 0      # the ReLU zeroed the negative ones


@pytest.mark.parametrize("depth", [2, 3])
def test_big_hidden_stacks(depth):
    case = C.big_hidden_stack(depth)
    got, spans, ops = check_exact(case)
    assert not ops[0][1].any()
    for hi, lo in ops[1:]:
        assert lo.any() and hi.min() == 0 and (hi == 0).mean() > 0.2
    assert (ops[1][0] + ops[1][1]).max() * 2.0 ** 5 > 2.0 ** 19                       # hidden integers near 2^20
    assert not bits_equal(C.model(case, 1, guard=[]), got)


@pytest.mark.parametrize("n", [12, 516, 1028])
def test_normalize_cases(n):
    case = C.normalize_case(n)
    spans, ops = [], []
    got = C.model(case, 3, guard=spans, operands=ops)
    assert M.operands_in_range(ops)
    hidden = ops[1][0]
    z = case["zero_row"]
    assert not ops[1][1].any() and set(np.unique(np.abs(hidden))) == {0.0, 4.0}       # +-2, times 2^x_exp
    assert ((hidden != 0).sum(axis=1) == np.where(np.arange(hidden.shape[0]) == z, 0, n // 4)).all()
    assert hidden[0, n - 1] != 0
    assert bits_equal(got[z], case["layers"][2][2])                                   # the zero row: the bias
    ref = oracle(case)                                           # (the reference makes NaN of the zero row: 0 * inf)
    keep = np.arange(got.shape[0]) != z
    assert np.isnan(ref[z]).all() and bits_equal(got[keep], ref[keep])
    assert bits_equal(C.model(case, 1, guard=[]), got)
    assert bits_equal(C.model(case, 3, guard=[], x_exp=[2, -3]), got)


@pytest.mark.parametrize("D,L,R,T", [(8, 0, 0, 1), (8, 1, 0, 257), (40, 5, 5, 1), (40, 5, 5, 257), (16, 3, 2, 257)])
def test_spliced_cases(D, L, R, T):
    case = C.spliced_case(D, L, R, T)
    got, _, _ = check_exact(case)
    assert np.abs(got).max() < 40                                # logits the reference-order softmax keeps finite
    ll = O.Nnet(case["layers"]).am_compute(case["feats"], case["prior"], L, R, 0.1)
    assert np.isfinite(ll).all()


def test_named_cases_build():
    for name, make in C.NAMED.items():
        assert C.holds(make()), name
