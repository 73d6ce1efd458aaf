"""The yardstick of delta features (include/pk_mi355.h): a numpy restatement of the rule -- Kaldi's
DeltaFeatures -- and the inputs the tests share.  Every column is independent.

    scales:  s[0] = [1.0f]; s[i] has len(s[i-1]) + 2 window entries, +0.0f at first; po = (len(s[i-1]) - 1) / 2;
             for j = -window .. window ascending, for k = -po .. po ascending:
                 s[i][j + k + po + window] += (float)j * s[i-1][k + po]          a rounded product, a rounded add
             then s[i] *= (float)(1.0 / (double)normalizer), normalizer = sum of j * j accumulated in float
    apply:   block i of frame t: acc = +0.0f; for j = -M_i .. M_i ascending (M_i = i * window):
                 if s[i][j + M_i] != 0.0f: acc = acc + (s[i][j + M_i] * x[clamp(t + j, 0, T - 1)])     two roundings, no fma

numpy float32 arrays multiply and add with one rounding each, and a loop over j in which whole [T][Db] arrays are added
IS the sequential order of every output.  Also here: five variants of the rule that a wrong implementation might be,
as switches, for the tests that show the comparisons tell them apart.

Kaldi leaves the axpy to BLAS, so agreement with Kaldi is within rounding; this restatement has not been compared with
a Kaldi binary."""
import numpy as np

SPECS = ((1, 1), (2, 2), (3, 1), (2, 5), (3, 8))
VARIANTS = ("fused", "descending", "keep_zero_taps", "zero_padding", "double_scales")


def reach(order, window):
    return order * window


def frame_counts(order, window, extra=(130,)):
    """T in {0, 1, 2, M, M + 1, 2M, 2M + 1} and the extras, ascending, each once."""
    M = reach(order, window)
    return tuple(sorted({0, 1, 2, M, M + 1, 2 * M, 2 * M + 1} | set(extra)))


def scales(order, window, double_scales=False):
    """A list of order + 1 float32 arrays, s[i] of 2 i window + 1 entries.  double_scales: the variant that forms them in
    double and rounds once at the end."""
    ft = np.float64 if double_scales else np.float32
    s = [np.ones(1, ft)]
    for i in range(1, order + 1):
        prev = s[-1]
        cur = np.zeros(len(prev) + 2 * window, ft)
        po = (len(prev) - 1) // 2
        normalizer = ft(0.0)
        for j in range(-window, window + 1):
            normalizer = ft(normalizer + ft(j * j))
            for k in range(-po, po + 1):
                p = ft(ft(j) * prev[k + po])
                cur[j + k + po + window] = ft(cur[j + k + po + window] + p)
        inv = ft(1.0 / float(normalizer))            # (float)(1.0 / (double)normalizer)
        s.append((cur * inv).astype(ft))
    return [a.astype(np.float32) for a in s]


def scale_table(order, window):
    """The flat table of pk.delta_scales: [order + 1][2 order window + 1], row i centred, zeros around it."""
    M = reach(order, window)
    out = np.zeros((order + 1, 2 * M + 1), np.float32)
    for i, s in enumerate(scales(order, window)):
        out[i, M - i * window:M + i * window + 1] = s
    return out


def add_deltas(x, order, window, fused=False, descending=False, keep_zero_taps=False, zero_padding=False, double_scales=False):
    """The rule -> float32 [T][(order + 1) Db].  The keywords switch the wrong variants on."""
    x = np.ascontiguousarray(x, np.float32)
    T, Db = x.shape
    out = np.zeros((T, (order + 1) * Db), np.float32)
    if T == 0:
        return out
    s = scales(order, window, double_scales)
    t = np.arange(T)
    with np.errstate(all="ignore"):
        for i in range(order + 1):
            M = i * window
            acc = np.zeros((T, Db), np.float64 if fused else np.float32)
            taps = range(M, -M - 1, -1) if descending else range(-M, M + 1)
            for j in taps:
                sc = s[i][j + M]
                if sc == 0.0 and not keep_zero_taps:
                    continue
                rows = x[np.clip(t + j, 0, T - 1)]
                if zero_padding:
                    rows = np.where(((t + j < 0) | (t + j >= T))[:, None], np.float32(0.0), rows)
                if fused:                            # one rounding per tap: the product is exact in double
                    acc = (acc + np.float64(sc) * rows.astype(np.float64)).astype(np.float32).astype(np.float64)
                else:
                    acc = acc + (sc * rows)
            out[:, i * Db:(i + 1) * Db] = acc.astype(np.float32)
    return out


def wide(T, D, seed=11):
    """N(0, 1) 2^k, k uniform in [-20, 20]: every exponent range in one matrix."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, D)) * np.exp2(rng.integers(-20, 21, (T, D)))).astype(np.float32)


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
