"""The fp16 matrix-core kernels (csrc/gemm_f16.hip: GemmF16K32Kernel for "f16x3", GemmF16Kernel for "f16", the
re-splitting epilogue, NormalizeSplitKernel, SplitKernel) held to EXACT answers.

On the dyadic grids of tests/f16_cases.py every product and every partial sum is exactly representable in fp32 in any
order (tests/f16_model.py: exactness_guard; the constructions are checked on the CPU in test_f16_exact_cases.py), so
the accumulation order does not matter and the GPU must return the mathematically exact result -- which is also the
fp32 oracle's -- bit for bit.  No tolerance anywhere in this file: indexing, swizzles, padding, k tails, tile walks,
the split, each cross term, the exponent plumbing, the epilogues and the range verdict either are right or a bit moves.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pocketkaldi_amd as pk
from oracle import oracle as O

import f16_cases as C
import f16_model as M

PRECISIONS = {"f16x3": 3, "f16": 1}


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def where_differs(got, want):
    bad = np.argwhere(np.ascontiguousarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32))
    i = tuple(bad[0])
    return "%d of %d values differ, first at %s: got %r, want %r" % (len(bad), got.size, i, got[i], want[i])


def assert_exact(case, precision, want=None, x_exp=None):
    """Run on the GPU; the result must be the model's bits (fed with the exponents the library reports)."""
    got, w_exp = C.run_gpu(case, precision, x_exp)
    assert w_exp == C.w_exps(case["layers"])
    if want is None:
        want = C.model(case, PRECISIONS[precision], guard=[], w_exp=w_exp, x_exp=x_exp)
    assert bits_equal(got, want), where_differs(got, want)
    return got


@functools.lru_cache(maxsize=None)
def affine(shape, relu):
    case = C.integer_affine(*shape, relu)
    return case, C.model(case, 3, guard=[])


@functools.lru_cache(maxsize=None)
def named(name):
    case = C.NAMED[name]()
    return case, {p: C.model(case, t, guard=[]) for p, t in PRECISIONS.items()}


# ------------------------------------------------------------------ one affine layer at every edge

@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", C.AFFINE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_one_affine_layer_is_exact(shape, relu):
    case, want = affine(shape, relu)
    assert bits_equal(want, O.Nnet(case["layers"]).propagate(case["x"]))
    for precision in PRECISIONS:                       # lo = 0 everywhere: both kernels owe the same exact bits
        assert_exact(case, precision, want)


# ------------------------------------------------------------------ each cross term on its own

@pytest.mark.parametrize("shape", C.LO_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("family", ["w_lo", "x_lo"])
def test_each_cross_term(family, shape):
    case = (C.w_lo_affine if family == "w_lo" else C.x_lo_affine)(*shape)
    full, hi_only = C.model(case, 3, guard=[]), C.model(case, 1, guard=[])
    assert bits_equal(full, O.Nnet(case["layers"]).propagate(case["x"])) and not bits_equal(full, hi_only)
    assert_exact(case, "f16x3", full)                  # hi x lo (w_lo) / lo x hi (x_lo) is all that separates the two
    assert_exact(case, "f16", hi_only)


# ------------------------------------------------------------------ exponents

@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_weight_scale_and_input_exponent_move_no_bit(precision):
    case = C.w_lo_affine(64, 48, 300)
    W, b = case["layers"][0][1], case["layers"][0][2]
    base = assert_exact(case, precision)
    e_w = C.w_exps(case["layers"])[0]
    for s in (-20, 0, 6):
        moved = dict(case, layers=[("linear", W * np.float32(2.0 ** s), b * np.float32(2.0 ** s))])
        got, w_exp = C.run_gpu(moved, precision)
        assert w_exp == [e_w - s]
        want = C.model(moved, PRECISIONS[precision], guard=[], w_exp=w_exp)
        assert bits_equal(got, want), where_differs(got, want)
        assert bits_equal(got * np.float32(2.0 ** -s), base)
    for e in (3, -4):
        assert bits_equal(assert_exact(case, precision, x_exp=[e]), base)
    ints, want = affine((64, 33, 64), True)
    for e in (3, -4):
        assert_exact(ints, precision, want, x_exp=[e])


# ------------------------------------------------------------------ stacks: the LAST = false epilogue and the re-split

@pytest.mark.parametrize("depth", [2, 3])
def test_small_integer_stacks(depth):
    case = C.small_int_stack(depth)
    want = C.model(case, 3, guard=[])
    assert bits_equal(want, O.Nnet(case["layers"]).propagate(case["x"]))
    for precision in PRECISIONS:
        assert_exact(case, precision, want)
        assert_exact(case, precision, want, x_exp=[1, -2, 3][:depth])


@pytest.mark.parametrize("depth", [2, 3])
def test_stacks_whose_hidden_values_need_both_halves(depth):
    case = C.big_hidden_stack(depth)
    ops = []
    full, hi_only = C.model(case, 3, guard=[], operands=ops), C.model(case, 1, guard=[])
    assert all(lo.any() for _, lo in ops[1:]) and not bits_equal(full, hi_only)
    assert bits_equal(full, O.Nnet(case["layers"]).propagate(case["x"]))
    assert_exact(case, "f16x3", full)
    assert_exact(case, "f16", hi_only)


@pytest.mark.parametrize("n", [12, 516, 1028])
def test_normalize_between_two_affine_layers(n):
    case = C.normalize_case(n)
    want = C.model(case, 3, guard=[])
    z = case["zero_row"]
    assert bits_equal(want[z], case["layers"][2][2])             # the all-zero row stays zero: the next layer's bias
    keep = np.arange(want.shape[0]) != z
    assert bits_equal(want[keep], O.Nnet(case["layers"]).propagate(case["x"])[keep])
    for precision in PRECISIONS:
        assert_exact(case, precision, want)
        assert_exact(case, precision, want, x_exp=[2, -3])


# ------------------------------------------------------------------ the spliced first layer and the tail

@pytest.mark.parametrize("D,L,R,T,N", [(8, 0, 0, 1, 50), (8, 0, 0, 257, 50), (8, 1, 0, 1, 50), (8, 1, 0, 257, 50),
                                       (40, 5, 5, 1, 50), (40, 5, 5, 257, 50), (16, 3, 2, 1, 50), (16, 3, 2, 257, 50),
                                       (8, 1, 0, 4100, 5)])
def test_spliced_first_layer_and_reference_tail(D, L, R, T, N):
    case = C.spliced_case(D, L, R, T, N)
    ref = O.Nnet(case["layers"]).am_compute(case["feats"], case["prior"], L, R, 0.1)
    assert np.isfinite(ref).all()
    for precision in PRECISIONS:
        am = pk.AcousticModel(case["layers"], case["prior"], L, R, precision=precision).set_softmax("reference")
        got = pk.Decodable(am, 0.1, case["feats"]).log_prob()
        assert bits_equal(got, ref), (precision, where_differs(got, ref))
        am.close()


# ------------------------------------------------------------------ forced MFMA shapes and tile walks

CHILD = """
import sys
try:
    import torch  # noqa: F401 (first, as tests/conftest.py: one HIP runtime in the process)
except ImportError:
    pass
sys.path[:0] = [%r, %r]
import numpy as np
import f16_cases as C
precision, path = sys.argv[1], sys.argv[2]
np.savez(path, **{name: C.run_gpu(C.NAMED[name](), precision)[0] for name in sys.argv[3:]})
print("child: ok")
"""
FORCED_CASES = ["edge_257_15_257", "edge_64_48_64", "tiles_5x6", "w_lo_64_48_300", "big_hidden_2"]


@pytest.mark.parametrize("walk", ["1x1", "3x5"])
@pytest.mark.parametrize("precision,shape", [("f16x3", "32"), ("f16", "16")])
def test_forced_shapes_and_walks_give_the_same_exact_bits(precision, shape, walk, tmp_path):
    """PK_MI355_F16_SHAPE / _WALK are read once per process: a fresh child runs the kernel form the mode does not
    take by default (32x32x16 for f16x3, 16x16x32 for f16) under another tile walk."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-c", CHILD % (repo, os.path.join(repo, "tests")), precision, out] + FORCED_CASES,
                       capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, PK_MI355_F16_SHAPE=shape, PK_MI355_F16_WALK=walk))
    assert r.returncode == 0 and "child: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)
    for name in FORCED_CASES:
        want = named(name)[1][precision]
        assert bits_equal(z[name], want), (name, where_differs(z[name], want))


def test_the_default_process_agrees_with_the_forced_ones():
    for name in FORCED_CASES:
        case, want = named(name)
        for precision in PRECISIONS:
            assert_exact(case, precision, want[precision])


# ------------------------------------------------------------------ the range verdict at its boundaries

def _placed(top, K=24, N=20, T=6):
    """Integer x whose largest magnitude is `top`, small integer W."""
    rng = np.random.default_rng([0xE7, top])
    x = rng.integers(-min(top, 1000), min(top, 1000) + 1, size=(T, K)).astype(np.float32)
    x[2, 5] = -float(top)
    W = rng.integers(-2, 3, size=(N, K)).astype(np.float32)
    W[0, 0] = 2.0
    return {"x": x, "layers": [("linear", W, rng.integers(-9, 10, size=N).astype(np.float32))], "x_exp": [0]}


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_range_verdict_boundaries(precision):
    top = _placed(1023)                                          # 1023 * 2^6 = 65472: the fp16 value just below the clamp
    want = C.model(top, 3, guard=[])
    assert bits_equal(want, O.Nnet(top["layers"]).propagate(top["x"]))
    ops = []
    C.model(top, 3, guard=[], operands=ops, x_exp=[6])
    assert np.abs(ops[0][0]).max() == 65472.0 and not ops[0][1].any()
    assert_exact(top, precision, want, x_exp=[6])
    with pytest.raises(pk.PkError, match="affine layer 0 saturated"):
        C.run_gpu(_placed(2047), precision, x_exp=[5])           # 2047 * 2^5 = 65504
    one = _placed(1)
    assert_exact(one, precision, C.model(one, 3, guard=[]), x_exp=[-5])        # max |hi| = 2^-5 exactly
    below = _placed(2047)                                        # 2047 * 2^-16: the fp16 value just below 2^-5
    assert np.abs(M.split(below["x"] * np.float32(2.0 ** -16))[0]).max() == float(np.nextafter(np.float16(2.0 ** -5), np.float16(0)))
    with pytest.raises(pk.PkError, match="affine layer 0 is too small"):
        C.run_gpu(below, precision, x_exp=[-16])


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_an_all_zero_hidden_operand_passes(precision):
    rng = np.random.default_rng(0xE8)
    x = rng.integers(0, 5, size=(9, 24)).astype(np.float32)
    x[0, 0] = 4.0
    W1 = (0 - rng.integers(0, 3, size=(257, 24))).astype(np.float32)
    W1[0, 0] = -2.0
    b2 = rng.integers(-9, 10, size=12).astype(np.float32)
    layers = [("linear", W1, np.zeros(257, np.float32)), ("relu",),
              ("linear", rng.integers(-2, 3, size=(12, 257)).astype(np.float32), b2)]
    case = {"x": x, "layers": layers, "x_exp": [0, 3]}
    ops = []
    want = C.model(case, 3, guard=[], operands=ops)
    assert not ops[1][0].any() and bits_equal(want, np.tile(b2, (9, 1)))
    assert_exact(case, precision, want)
