"""The yardstick of the normalisation spec (include/pk_mi355.h): a numpy restatement of the rule --
Kaldi's AccCmvnStats and ApplyCmvn -- and the inputs the tests share.  Every column is independent:

    utterance mode: S0 += (double)x[t][d], S1 += (double)x[t][d] * (double)x[t][d], t ascending from 0.0; N = T
    speaker mode:   S0, S1, N are the caller's
    mean = norm_means ? S0 / N : 0;  no norm_vars: scale = 1, offset = -mean
    norm_vars: var = S1 / N - mean * mean, raised to 1e-20 where below (NaN stays); scale = 1 / sqrt(var); offset = -(mean * scale)
    y = norm_vars ? (x * (float)scale) + (float)offset : x + (float)offset      in float, two roundings

numpy adds two float64 rows element by element, so a loop over t IS the sequential order of every column; float32
arrays multiply and add with one rounding each (no fma).  Also here: three variants of the rule that a wrong
implementation might be (float accumulation, a fused apply, another summation order), for the tests that show the
comparisons tell them apart."""
import numpy as np

MODES = ("none", "utterance", "speaker")
SWITCHES = ((True, False), (True, True), (False, True))       # (norm_means, norm_vars): the three pairs a stats mode takes
VAR_FLOOR = 1e-20


def features(T, D, seed=7):
    """5 N(0, 1) + 3, column 0 shifted by 1e4: a large mean in front of a small variance, where float sums fail."""
    x = (5.0 * np.random.default_rng(seed).standard_normal((T, D)) + 3.0).astype(np.float32)
    x[:, 0] += np.float32(1e4)
    return x


def accumulate(x, acc=np.float64):
    """The 2 x (D + 1) record of x [T][D]: sums and count, sums of squares and 0.  acc: the accumulator's type (the
    rule's is float64)."""
    T, D = x.shape
    rec = np.zeros((2, D + 1), acc)
    xa = x.astype(acc)
    with np.errstate(all="ignore"):
        for t in range(T):
            rec[0, :D] += xa[t]
            rec[1, :D] += xa[t] * xa[t]
    rec[0, D] = T
    return rec.astype(np.float64)


def accumulate_interleaved(x, ways=4):
    """Another summation order: `ways` partial sums over t % ways, added at the end."""
    T, D = x.shape
    part = np.zeros((ways, 2, D), np.float64)
    xa = x.astype(np.float64)
    for t in range(T):
        part[t % ways, 0] += xa[t]
        part[t % ways, 1] += xa[t] * xa[t]
    rec = np.zeros((2, D + 1), np.float64)
    for w in range(ways):
        rec[:, :D] += part[w]
    rec[0, D] = T
    return rec


def finalize(rec, norm_means, norm_vars):
    """A record -> (offset, scale) as float32 [D] each."""
    rec = np.asarray(rec, np.float64)
    D = rec.shape[1] - 1
    n = rec[0, D]
    with np.errstate(all="ignore"):
        mean = rec[0, :D] / n if norm_means else np.zeros(D)
        if not norm_vars:
            return (-mean).astype(np.float32), np.ones(D, np.float32)
        var = rec[1, :D] / n - mean * mean
        var = np.where(var < VAR_FLOOR, VAR_FLOOR, var)           # (NaN < x is false: a NaN stays)
        scale = 1.0 / np.sqrt(var)
        return (-(mean * scale)).astype(np.float32), scale.astype(np.float32)


def apply(x, offs, scale, norm_vars, fused=False):
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        if fused:                                                 # one rounding: the product is exact in double
            return (x.astype(np.float64) * scale.astype(np.float64) + offs.astype(np.float64)).astype(np.float32) if norm_vars else x + offs
        return (x * scale) + offs if norm_vars else x + offs


def normalize(x, mode, norm_means=True, norm_vars=False, stats=None, acc=np.float64, fused=False):
    """The rule -> (y float32 [T][D], the record an utterance-mode call accumulated or None)."""
    x = np.ascontiguousarray(x, np.float32)
    if mode == "none":
        return x.copy(), None
    rec = accumulate(x, acc) if mode == "utterance" else np.asarray(stats, np.float64)
    if x.shape[0] == 0:
        return x.copy(), (rec if mode == "utterance" else None)
    offs, scale = finalize(rec, norm_means, norm_vars)
    return apply(x, offs, scale, norm_vars, fused), (rec if mode == "utterance" else None)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def columns_differing(a, b):
    """Columns in which two float arrays of one shape differ in some bit."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return int((a.view(u) != b.view(u)).reshape(a.shape).any(axis=0).sum()) if a.ndim == 2 else int((a.view(u) != b.view(u)).sum())
