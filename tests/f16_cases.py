"""Exactly representable cases for the fp16 matrix-core modes: inputs on dyadic grids for which tests/f16_model.py
proves (exactness_guard) that no sum can round, so the model's float64 result IS the answer and a kernel must return
its bits.  Every case is a dict {x | feats, layers, x_exp, ...}; the generators thin their operands until the guard
holds and every operand sits inside the range the modes accept -- they look at the model only, never at a kernel.
test_f16_exact_cases.py checks the constructions on the CPU, test_gpu_f16_exact.py runs them on the GPU.
"""
import numpy as np

import f16_model as M

# (T, K, N) at the edges of the 256 x 256 tile, the 8-wide (hi, lo) interleave, the k16 half-slab and the k32 pair
AFFINE_SHAPES = [(1, 1, 1), (1, 7, 2), (255, 8, 255), (256, 9, 256), (257, 15, 257), (3, 16, 513), (513, 17, 3),
                 (64, 31, 64), (64, 32, 64), (64, 33, 64), (64, 48, 64), (257, 440, 520), (33, 2048, 130),
                 (5, 2560, 257), (1100, 16, 1300)]
LO_SHAPES = [(257, 40, 257), (64, 48, 300), (33, 520, 130)]


def w_exps(layers):
    return [M.finalize_exponent(l[1]) for l in layers if l[0] == "linear"]


def num_linear(layers):
    return sum(1 for l in layers if l[0] == "linear")


def model(case, terms, guard=None, operands=None, x_exp=None, w_exp=None):
    """The exact answer of a case: the fp32 output of its last affine layer."""
    x_exp = case["x_exp"] if x_exp is None else x_exp
    return M.f16_stack(case["x"], case["layers"], w_exps(case["layers"]) if w_exp is None else w_exp, x_exp, terms,
                       guard=guard, operands=operands)


def holds(case, terms=3):
    """The guard holds in every GEMM of the case and every operand is in range."""
    ops = []
    try:
        model(case, terms, guard=[], operands=ops)
    except M.NotExact:
        return False
    return M.operands_in_range(ops)


def _thin(make, densities):
    for d in densities:
        case = make(d)
        if holds(case, 3) and holds(case, 1):
            case["density"] = d
            return case
    raise M.NotExact("no density of %s makes the case exact" % (densities,))


def _ints(rng, shape, lo, hi, density=1.0):
    a = rng.integers(lo, hi + 1, size=shape).astype(np.float32)
    if density < 1.0:
        a = np.where(rng.random(shape) < density, a, np.float32(0.0))          # (no -0.0)
    return a


def integer_affine(T, K, N, relu, seed=0):
    """|x| <= 8 integers, W = j 2^-9 with |j| <= 16, bias on the 2^-6 grid: every lo half is zero, sum |terms| <=
    128 K g (2^18.3 g at K = 2560)."""
    rng = np.random.default_rng([0xE0, T, K, N, seed])
    x = _ints(rng, (T, K), -8, 8)
    W = _ints(rng, (N, K), -16, 16) * np.float32(2.0 ** -9)
    x[0, 0], W[0, 0] = 5.0, np.float32(13 * 2.0 ** -9)
    b = _ints(rng, (N,), -40, 40) * np.float32(2.0 ** -6)
    layers = [("linear", W, b)] + ([("relu",)] if relu else [])
    return {"x": x, "layers": layers, "x_exp": [0]}


W_HI = np.array([9216, -9216, 10240, 12288, -12288], np.float32)      # away from powers of two: fp16(hi + lo) = hi
X_HI = np.array([1152, -1152, -1280, 1536, 0], np.float32)


def w_lo_halves(rng, N, K):
    hi = W_HI[rng.integers(0, len(W_HI), size=(N, K))]
    lo = _ints(rng, (N, K), -3, 3)
    hi.flat[0], lo.flat[0] = 12288.0, 3.0
    return hi, lo


def w_lo_affine(T, K, N, seed=0, log2_scale=-16):
    """W carries lo halves (scaled hi in {+-9216, 10240, +-12288}: fp16 ulp 8, lo in [-3, 3]); x in {-1, 0, 1}, lo = 0."""
    def make(density):
        rng = np.random.default_rng([0xE1, T, K, N, seed])
        hi, lo = w_lo_halves(rng, N, K)
        W = (hi + lo) * np.float32(2.0 ** log2_scale)
        x = _ints(rng, (T, K), -1, 1, density)
        x[0, 0] = 1.0
        b = _ints(rng, (N,), -40, 40) * np.float32(2.0 ** log2_scale)
        return {"x": x, "layers": [("linear", W, b)], "x_exp": [0], "w_halves": (hi, lo), "log2_scale": log2_scale}
    return _thin(make, [0.25, 0.18, 0.12, 0.08, 0.05, 0.03])


def x_lo_affine(T, K, N, seed=0):
    """x carries lo halves (hi in {+-1152, -1280, 1536, 0}: fp16 ulp 1, lo in [-3, 3] / 16); W in {-2 .. 2}, lo = 0."""
    def make(density):
        rng = np.random.default_rng([0xE2, T, K, N, seed])
        hi = X_HI[rng.integers(0, len(X_HI), size=(T, K))]
        lo = np.where(hi != 0, _ints(rng, (T, K), -3, 3) * np.float32(1.0 / 16), np.float32(0.0))
        hi.flat[0], lo.flat[0] = 1536.0, np.float32(3.0 / 16)
        W = _ints(rng, (N, K), -2, 2, density)
        W[0, 0], W[-1, -1] = 2.0, 1.0
        b = _ints(rng, (N,), -40, 40)
        return {"x": hi + lo, "layers": [("linear", W, b)], "x_exp": [0], "x_halves": (hi, lo)}
    return _thin(make, [0.25, 0.18, 0.12, 0.08, 0.05, 0.03, 0.02])


def small_int_stack(depth, T=70, K=24, N=300, x_exp=None, seed=0):
    """Two or three affine layers with ReLU, hidden widths 257 (and 12), every hidden value a small integer (lo = 0);
    the hidden operands carry non-zero exponents."""
    dims = [K, 257, N] if depth == 2 else [K, 257, 12, N]
    x_exp = ([0, 2, -1] if x_exp is None else x_exp)[:depth]

    def make(density):
        rng = np.random.default_rng([0xE3, depth, T, seed])
        layers = []
        for i in range(depth):
            W = _ints(rng, (dims[i + 1], dims[i]), -2, 2, 1.0 if i == 0 else density)
            W[0, 0] = 2.0
            layers.append(("linear", W, _ints(rng, (dims[i + 1],), -6, 6)))
            if i < depth - 1:
                layers.append(("relu",))
        return {"x": _ints(rng, (T, K), -4, 4), "layers": layers, "x_exp": x_exp}
    return _thin(make, [0.1, 0.05, 0.03])


def big_hidden_stack(depth, T=40, K=40, N=300, seed=0):
    """The first layer's W carries lo halves and x reaches +-8: its ReLU'd output holds odd integers up to 2^20, which
    the LAST = false epilogue must re-split into hi AND lo halves (operand exponent -5: below the 65504 clamp).  Every
    later W has lo = 0 and a few +-1 per row, so the lo x hi term carries the low bits through."""
    dims = [K, 257, N] if depth == 2 else [K, 257, 12, N]
    x_exp = [0, -5, -6][:depth]

    def make(knob):
        density, nnz = knob
        rng = np.random.default_rng([0xE4, depth, T, seed])
        hi, lo = w_lo_halves(rng, dims[1], K)
        layers = [("linear", hi + lo, _ints(rng, (dims[1],), -40, 40)), ("relu",)]
        for i in range(1, depth):
            W = np.zeros((dims[i + 1], dims[i]), np.float32)
            for r in range(W.shape[0]):
                W[r, rng.choice(dims[i], size=nnz, replace=False)] = rng.choice([-1.0, 1.0], size=nnz)
            layers.append(("linear", W, _ints(rng, (dims[i + 1],), -40, 40)))
            if i < depth - 1:
                layers.append(("relu",))
        x = _ints(rng, (T, K), -8, 8, density)
        x[0, 0] = 8.0
        return {"x": x, "layers": layers, "x_exp": x_exp}
    return _thin(make, [(d, n) for n in (3, 2, 1) for d in (0.4, 0.25)])


def normalize_case(n, T=9, K=20, N=37, seed=0):
    """Linear, Normalize, Linear.  x rows are one-hot (+-2^j); column k of W1 holds exactly n / 4 non-zero entries
    +-c_k, c_k a power of two, and b1 = 0: a hidden row has n / 4 entries +-c, so sum x^2 = (n / 4) c^2 adds up exactly
    in any order, sqrt(n / ssq) = 2 / c exactly, and the normalized row holds +-2.  Row 3 of x is all zero: the hidden
    row stays zero (NormalizeSplitKernel) and the output is the second layer's bias."""
    assert n % 4 == 0
    rng = np.random.default_rng([0xE5, n, seed])
    W1 = np.zeros((n, K), np.float32)
    for k in range(K):
        rows = rng.choice(n - 1, size=n // 4, replace=False)
        if k == 0:
            rows[0] = n - 1                                   # the last hidden column is used (n is no multiple of 8)
        W1[rows, k] = rng.choice([-1.0, 1.0], size=n // 4) * 2.0 ** int(rng.integers(-6, -2))
    x = np.zeros((T, K), np.float32)
    for t in range(T):
        x[t, rng.integers(0, K)] = rng.choice([-1.0, 1.0]) * 2.0 ** int(rng.integers(0, 4))
    x[0, :] = 0.0
    x[0, 0] = 4.0
    x[3, :] = 0.0
    W2 = _ints(rng, (N, n), -16, 16)
    W2[0, n - 1] = 16.0
    layers = [("linear", W1, np.zeros(n, np.float32)), ("normalize",), ("linear", W2, _ints(rng, (N,), -40, 40))]
    case = {"x": x, "layers": layers, "x_exp": [0, 1], "zero_row": 3}
    if not holds(case, 3):
        raise M.NotExact("normalize case n = %d" % n)
    return case


def spliced_case(D, L, R, T, N=50, seed=0):
    """Integer features [T][D], a spliced first (and only) affine layer on the 2^-3 grid, softmax, a prior: the logits
    are exact, so both fp16 modes feed the reference-order tail the same fp32 values the fp32 path feeds it."""
    def make(density):
        rng = np.random.default_rng([0xE6, D, L, R, T, seed])
        feats = _ints(rng, (T, D), -3, 3)
        feats[0, 0] = 3.0
        W = _ints(rng, (N, D * (L + R + 1)), -2, 2, density) * np.float32(0.125)
        W[0, 0] = 0.25
        b = _ints(rng, (N,), -8, 8) * np.float32(0.25)
        prior = rng.integers(1, 9, size=N).astype(np.float32)
        return {"feats": feats, "layers": [("linear", W, b), ("softmax",)], "x_exp": [0], "prior": prior / prior.sum(),
                "ctx": (L, R)}

    def spliced(density):
        from oracle import oracle as O
        case = make(density)
        case["x"] = O.splice(case["feats"], L, R)
        return case
    return _thin(spliced, [0.5, 0.2])


NAMED = {
    "edge_257_15_257": lambda: integer_affine(257, 15, 257, True),
    "edge_64_48_64": lambda: integer_affine(64, 48, 64, False),
    "tiles_5x6": lambda: integer_affine(1100, 16, 1300, True),
    "w_lo_64_48_300": lambda: w_lo_affine(64, 48, 300),
    "x_lo_257_40_257": lambda: x_lo_affine(257, 40, 257),
    "big_hidden_2": lambda: big_hidden_stack(2),
}


def run_gpu(case, precision, x_exp=None):
    """The case through pocketkaldi_amd.AcousticModel.propagate -> (fp32 output, w_exp)."""
    import pocketkaldi_amd as pk
    layers = [l for l in case["layers"] if l[0] != "softmax"]
    am = pk.AcousticModel(layers, num_pdfs=layers[-1 if layers[-1][0] == "linear" else -2][1].shape[0], precision=precision)
    x_exp = case["x_exp"] if x_exp is None else x_exp
    if any(x_exp):
        am.set_input_exponents(x_exp)
    w, xe = am.exponents()
    assert list(xe) == list(x_exp)
    out = am.propagate(case["x"])
    am.close()
    return out, [int(e) for e in w]
