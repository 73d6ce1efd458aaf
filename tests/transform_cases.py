"""The yardstick of the feature transforms (include/pk_mi355.h): a numpy restatement of the rule --
Kaldi's splice-feats (the first and last frame repeated at the edges) and transform-feats (AddMatMat, then the offset
column with AddVecToRows: "offset last") -- and the inputs the tests share.  With Dp = in_dim, L, R, K = (L + R + 1) Dp,
one output o of frame t of an utterance of T frames, in float:

    acc = +0.0f
    for j = -L .. R ascending, for d = 0 .. Dp - 1 ascending:
        acc = acc + (m[o][(j + L) * Dp + d] * x[clamp(t + j, 0, T - 1)][d])      a rounded product, a rounded add, no fma
    if affine (cols == K + 1): acc = acc + m[o][K]

No tap is skipped (a zero entry times an inf is NaN).  The per-utterance stage is the same rule with L = R = 0 and
utterance u's own matrix.

numpy float32 arrays multiply and add with one rounding each, and a loop over k in which whole [T][rows] arrays are
added IS the sequential order of every output.  Also here: five variants of the rule that a wrong implementation might
be, as switches, for the tests that show the comparisons tell them apart.

The restatement is from the tools' description and has not been compared with a Kaldi binary; Kaldi leaves the
product's order to BLAS, so agreement with Kaldi is within rounding."""
import numpy as np

import norm_cases

# (in_dim, L, R, rows, affine)
HOST_SPECS = ((1, 0, 0, 1, True), (13, 3, 3, 40, True), (40, 4, 4, 40, False), (65, 1, 2, 63, True), (39, 0, 0, 39, True), (512, 8, 8, 3, False))
VARIANT_SPECS = ((13, 3, 3, 40, True), (40, 4, 4, 40, False), (1, 0, 0, 1, True))
VARIANTS = ("fused", "descending", "offset_first", "zero_padding")       # (the fifth, a neighbour's matrix: transform_utts)


def frame_counts(L, R, extra=(33,)):
    """T in {0, 1, 2, L, R, L + R, L + R + 1} and the extras, ascending, each once."""
    return tuple(sorted({0, 1, 2, L, R, L + R, L + R + 1} | set(extra)))


def matrix(in_dim, L, R, rows, affine, seed=5):
    """N(0, 1) / sqrt(K): outputs of the inputs' order of magnitude."""
    K = (L + R + 1) * in_dim
    return (np.random.default_rng(seed).standard_normal((rows, K + (1 if affine else 0))) / np.sqrt(K)).astype(np.float32)


def transform(x, m, L, R, fused=False, descending=False, offset_first=False, zero_padding=False):
    """The rule -> float32 [T][rows]; in_dim is x's width, affine when m has one column more than K.  The keywords switch
    the wrong variants on."""
    x = np.ascontiguousarray(x, np.float32)
    m = np.ascontiguousarray(m, np.float32)
    T, Dp = x.shape
    rows, cols = m.shape
    K = (L + R + 1) * Dp
    assert cols in (K, K + 1), (cols, K)
    affine = cols == K + 1
    ft = np.float64 if fused else np.float32
    acc = np.zeros((T, rows), ft)
    if T == 0:
        return acc.astype(np.float32)
    t = np.arange(T)
    with np.errstate(all="ignore"):
        if affine and offset_first:
            acc = acc + m[:, K].astype(ft)[None, :]
        ks = range(K - 1, -1, -1) if descending else range(K)
        for k in ks:
            j, d = k // Dp - L, k % Dp
            col = x[np.clip(t + j, 0, T - 1), d]
            if zero_padding:
                col = np.where((t + j < 0) | (t + j >= T), np.float32(0.0), col)
            if fused:                                # one rounding per tap: the product is exact in double
                acc = (acc + m[:, k].astype(np.float64)[None, :] * col.astype(np.float64)[:, None]).astype(np.float32).astype(np.float64)
            else:
                acc = acc + (m[None, :, k] * col[:, None])
        if affine and not offset_first:
            acc = (acc + m[:, K].astype(ft)[None, :]).astype(np.float32)
    return acc.astype(np.float32)


def transform_utts(xs, mats, neighbour=False):
    """The per-utterance stage: utterance u through mats[u] with L = R = 0.  neighbour: the wrong variant that gives
    utterance u the matrix of utterance u - 1."""
    return [transform(x, mats[(u - 1) % len(mats)] if neighbour else mats[u], 0, 0) for u, x in enumerate(xs)]


def features(T, D, seed=7):
    return norm_cases.features(T, D, seed)


def normal(T, D, seed=3):
    return np.random.default_rng(seed).standard_normal((T, D)).astype(np.float32)


def wide(T, D, seed=11):
    """N(0, 1) 2^k, k uniform in [-20, 20]: every exponent range in one matrix."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, D)) * np.exp2(rng.integers(-20, 21, (T, D)))).astype(np.float32)


def float64_bound(x, m, L, R):
    """(the float64 product of the spliced rows, the bound on the rule's distance from it): gamma * sum |m_k x_k| + one
    ulp of the result, gamma = (K + 2) u / (1 - (K + 2) u), u = 2^-24 -- K products, K adds and the offset's add, each
    one rounding (Higham, Accuracy and Stability, section 3.1).  A consequence of the rule, not a measurement."""
    x64, m64 = np.asarray(x, np.float64), np.asarray(m, np.float64)
    T, Dp = x64.shape
    K = (L + R + 1) * Dp
    t = np.arange(T)
    idx = np.clip(t[:, None] + np.arange(-L, R + 1)[None, :], 0, max(T - 1, 0))
    sp = x64[idx].reshape(T, K) if T else np.zeros((0, K))
    ref = sp @ m64[:, :K].T
    mag = np.abs(sp) @ np.abs(m64[:, :K]).T
    if m64.shape[1] == K + 1:
        ref = ref + m64[:, K]
        mag = mag + np.abs(m64[:, K])
    u = 2.0 ** -24
    gamma = (K + 2) * u / (1 - (K + 2) * u)
    return ref, gamma * mag + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_but_nan(a, b):
    """Equal as bits wherever b is not NaN, NaN exactly where b is (a NaN's payload and sign are not part of the rule)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(b)
    return bool(np.array_equal(a.view(np.uint32)[ok], b.view(np.uint32)[ok]))


def outputs_differing(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())
