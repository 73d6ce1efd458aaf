"""The log-likelihood tail without a GPU: a float64 reference, a per-element error bound worked out from the kernels'
operations, exact bit predictions for rows whose arithmetic cannot round, and a float32 restatement of TailWaveRows'
chunk ownership (csrc/pk_tail_wave.h) into which named faults can be injected.

    out = scale * (max(x - lse, log 1e-20) - log prior),     lse = m + log sum exp(x - m)

The bound (error_bound below), from the operations of each kernel, u = 2^-24 (half an ulp, relative):

  wave form (TailWaveRows; stand-alone and fused):
    nm  = fl(-m L), L = fl(log2 e)      one rounding of a value of size 1.44 |m|.  It is the SAME for every column, so
                                        it multiplies the sum by 2^(nm error): lse moves by <= u |m| L ln 2 = u |m|
                                        (about 0.7 ulp of m).                                              -> 1 |m|
    a_j = fma(x_j, L, nm)               one rounding, relative u, of (x_j - m) L; L itself is off by 0.22 u relative.
                                        The term's relative error is ln 2 |a_j| 1.22 u = 1.22 u |x_j - m|.
    e_j = v_exp_f32(a_j)                1 ulp: 2 u relative.  (Results below 2^-126 are flushed: n 2^-126 of a sum
                                        that is >= 1.)
    s   = sum e_j                       per lane 4 C terms in turn, six wave levels, one pair add: depth 4 C + 6 (+ 1);
                                        positive terms, so relative (depth) u.  The per-term errors enter with the
                                        term's share w_j = e_j / s: sum w_j |x_j - m| =: D <= log n.
                                        relative error of s <= (2 + 1.22 D + depth) u
    logf(s)                             1 ulp: 2 u log s, on top of the relative error of s (d log s = ds / s)
    lse = fl(m + logf s)                u |lse| <= u (|m| + log s)                                         -> 1 |m|
    t   = fl(x_j - lse)                 u |x_j - lse|
    max(t, floor)                       1-Lipschitz; the float constant is off by 1.2e-7 of 46.05 u
    lp' = fl(-fl(logf prior) scale)     the host's logf: 1 ulp = 2 u |log prior|; the product: u |log prior| scale
    o   = fma(t, scale, lp')            u |o|

    |o - ref| <= scale u (2 max(|m|, 1) + |x_j - lse| + c) + 3 u scale |log prior| + 2 u |o|   (one ulp of the output),
    c = 2 + 1.22 D + depth + 3 log s                       (D, log s <= log n: c <= 111 at n = 8192)

  It grows with |m| (the rounding of m log2 e and of m + log s), not with |ref|.  An element whose exact t lies below
  the floor by more than the bound on t comes out as the floor constant whatever the rest did: its bound is the
  constant's own error.

  TailKernel / TailWideKernel: d_j = fl(x_j - m) (u |x_j - m|, instead of the nm and fma roundings; no |m| term from
  nm), libm expf (1 ulp), per thread ceil(n4 / 256) * 4 terms in turn (n / 256 for the wide kernel), six wave levels,
  two LDS levels; then fl(t - lp) (u |t - lp|) and the product with scale (u |o|).  The same shape with 1 max(|m|, 1).
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
LOG2E32 = np.float32(1.4426950408889634)
FLOOR32 = np.float32(-46.051701859880914)
FLOOR = math.log(1e-20)

FAULTS = ("no_select_last", "no_select_clamped", "half1_not_in_max", "half1_not_in_sum", "last_col_unwritten",
          "no_floor", "prior_neighbour")


# ------------------------------------------------------------------ shapes (pk_tail_wave.h, tail.hip)

def wave_chunks(n):
    return (((n + 3) >> 2) + 63) >> 6


def wave_shape(n):
    """(C, PAIR, EXACT) of the TailWaveRows instantiation LaunchTailWave and the fused launch pick for n columns."""
    c = wave_chunks(n)
    assert 1 <= c <= 32
    exact = c in (4, 8, 12, 16, 24, 32)
    if exact:
        return (c, False, True) if c <= 16 else (c // 2, True, True)
    for cap, shape in ((4, (4, False)), (8, (8, False)), (12, (12, False)), (16, (16, False)), (24, (12, True))):
        if c <= cap:
            return shape + (False,)
    return (16, True, False)


def kernel_cache(n):
    """TailKernel's register cache (LaunchTailMode): 1, 3 or 8 float4s per thread, or "wide"."""
    n4 = (n + 3) // 4
    return 1 if n4 <= 256 else 3 if n4 <= 768 else 8 if n4 <= 2048 else "wide"


def sum_depth(n, form):
    if form == "wave":
        C, pair, _ = wave_shape(n)
        return 4 * C + 6 + (1 if pair else 0)
    k = kernel_cache(n)
    return (-(-n // 256) if k == "wide" else 4 * k) + 6 + 2


# ------------------------------------------------------------------ reference and bound

def _row_stats(x):
    x64 = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x64.max(axis=1)
        d = x64 - m[:, None]
        e = np.exp(d)
        s = e.sum(axis=1)
        lse = m + np.log(s)
        D = np.where(e > 0, e * -d, 0.0).sum(axis=1) / s
    bad = np.isnan(x64).any(axis=1) | np.isposinf(x64).any(axis=1) | np.isneginf(m)
    return x64, m, s, lse, D, bad


def reference(x, prior, scale):
    """float64 on the float32 logits x[T][n]; a row with a NaN or a +inf, or of nothing but -inf, is NaN."""
    x64, m, s, lse, D, bad = _row_stats(x)
    with np.errstate(invalid="ignore"):
        t = np.maximum(x64 - lse[:, None], FLOOR)
        out = float(np.float32(scale)) * (t - np.log(np.asarray(prior, np.float32).astype(np.float64))[None, :])
    out[bad] = np.nan
    return out


def error_bound(x, prior, scale, form):
    """Per-element bound on |kernel - reference| (module docstring); form: "wave" | "kernel".  NaN rows: 0."""
    x64, m, s, lse, D, bad = _row_stats(x)
    n = x64.shape[1]
    sc = float(np.float32(scale))
    lp = np.abs(np.log(np.asarray(prior, np.float32).astype(np.float64)))[None, :]
    with np.errstate(invalid="ignore"):
        am = np.maximum(np.abs(m), 1.0)
        c = 2.0 + 1.22 * D + sum_depth(n, form) + 3.0 * np.log(s)
        t = x64 - lse[:, None]
        a = 2.0 if form == "wave" else 1.0
        e_t = U * ((a * am + c)[:, None] + np.abs(np.where(np.isfinite(t), t, 0.0)))
        floored = ~(t + e_t >= FLOOR)                                 # certainly below the floor (t = -inf included)
        e_t = np.where(floored, abs(float(FLOOR32) - FLOOR), e_t)
        ref = sc * (np.maximum(t, FLOOR) - np.log(np.asarray(prior, np.float32).astype(np.float64))[None, :])
        extra = U * np.abs(np.maximum(t, FLOOR)) + U * lp if form == "kernel" else 0.0     # fl(t - lp)
        b = sc * (e_t + extra) + 3.0 * U * sc * lp + 2.0 * U * np.abs(ref)
    b[bad] = 0.0
    return b


# ------------------------------------------------------------------ exact predictions

def round_f32(q):
    """The float32 nearest to the rational q (ties to even)."""
    q = Fraction(q)
    if q == 0:
        return np.float32(0.0)
    sign, a = (-1.0 if q < 0 else 1.0), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, -126)
    k = round(a / Fraction(2) ** (e - 23))                            # Fraction.__round__: ties to even
    v = math.ldexp(k, e - 23)
    return np.float32(sign * v) if v <= 3.4028234663852886e38 else np.float32(sign * np.inf)


def predict_bits(t, log_prior32, scale, form):
    """The kernel's float32 output for rows whose t = max(x - lse, floor) is known EXACTLY (float32 t[P][n], the floor
    already applied as FLOOR32): exact rational arithmetic, rounded once per device operation.
    form "wave":   fma(t, scale, fl(-log prior * scale));   form "kernel": fl(fl(t + -1 * log prior) * scale)."""
    t = np.ascontiguousarray(t, np.float32)
    lp = np.broadcast_to(np.ascontiguousarray(log_prior32, np.float32)[None, :], t.shape)
    sc = Fraction(float(np.float32(scale)))
    key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.ascontiguousarray(lp).view(np.uint32).astype(np.uint64)
    uniq, inv = np.unique(key, return_inverse=True)
    vals = np.empty(len(uniq), np.float32)
    for i, k in enumerate(uniq):
        tv = float(np.array([int(k) >> 32], np.uint32).view(np.float32)[0])
        lv = float(np.array([int(k) & 0xFFFFFFFF], np.uint32).view(np.float32)[0])
        if form == "wave":
            vals[i] = round_f32(Fraction(tv) * sc + Fraction(float(round_f32(-Fraction(lv) * sc))))
        else:
            vals[i] = round_f32(Fraction(float(round_f32(Fraction(tv) - Fraction(lv)))) * sc)
    return vals[inv.reshape(t.shape)]


# ------------------------------------------------------------------ TailWaveRows, restated

def _fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays: the product is exact in float64; the sum is rounded to odd there, so the
    second rounding to float32 is the only one that counts."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    with np.errstate(invalid="ignore"):
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def wave_model(x, n, scale, prior, fault=None, log_prior32=None):
    """TailWaveRows on logits x[T][n] in float32 numpy: which lane of which wave half owns which 16-byte chunk
    (q = lane + 64 c + 64 C half), the clamp of the read position to n4 - 1, the select to -inf under
    !EXACT || c == C - 1, the pair exchange of maxima and sums, vec_out and the range-checked stores, and the prior
    read at the clamped position.  A model of the OWNERSHIP, not of the hardware: exp2, log and the order of the
    wave-level sum are numpy's.  Unwritten outputs stay 0.  fault: one of FAULTS."""
    assert fault is None or fault in FAULTS
    x = np.ascontiguousarray(x, np.float32)
    T = x.shape[0]
    assert x.shape[1] == n
    C, pair, exact = wave_shape(n)
    H = 2 if pair else 1
    n4 = (n + 3) >> 2
    scale = np.float32(scale)
    lp32 = np.log(np.asarray(prior, np.float32)) if log_prior32 is None else np.asarray(log_prior32, np.float32)
    xp = np.zeros((T, 4 * n4), np.float32)                           # the row's padding columns hold 0 (zero weights, zero bias)
    xp[:, :n] = x
    lpp = np.zeros(4 * n4, np.float32)                               # the prior table is zero-padded
    lpp[:n] = lp32
    table = (-lpp * scale).astype(np.float32)                        # TailWavePriorEntry
    h, lane, c, e = np.meshgrid(np.arange(H), np.arange(64), np.arange(C), np.arange(4), indexing="ij")
    q = lane + 64 * (C * h + c)
    qc = np.minimum(q, n4 - 1)
    col = 4 * q + e                                                  # the unclamped column: selects and stores
    v = xp[:, 4 * qc + e]                                            # [T][H][64][C][4]
    sel = np.ones_like(col, bool) if not exact else (c == C - 1)
    if fault == "no_select_last":
        sel = sel & (c != C - 1)
    dead = sel & (col >= n)
    if fault == "no_select_clamped":                                 # a clamped chunk keeps the real columns it re-read
        dead = dead & ~((q >= n4) & (4 * qc + e < n))
    v = np.where(dead[None], np.float32(-np.inf), v)
    mh = v.max(axis=(2, 3, 4))                                       # [T][H]: each half's maximum
    m = mh[:, 0] if fault == "half1_not_in_max" else mh.max(axis=1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nm = (-m * LOG2E32).astype(np.float32)
        arg = _fma32(v, np.broadcast_to(LOG2E32, v.shape), np.broadcast_to(nm[:, None, None, None, None], v.shape))
        ex = np.exp2(arg).astype(np.float32)
        acc = np.zeros(v.shape[:3], np.float32)
        for cc in range(C):                                          # a lane's own terms in turn
            for ee in range(4):
                acc = acc + ex[:, :, :, cc, ee]
        w = 64
        while w > 1:                                                 # the wave's tree
            w //= 2
            acc = acc[:, :, :w] + acc[:, :, w:2 * w]
        sh = acc[:, :, 0]                                            # [T][H]
        s = sh[:, 0] if (H == 1 or fault == "half1_not_in_sum") else sh[:, 0] + sh[:, 1]
        lse = (m + np.log(s).astype(np.float32)).astype(np.float32)
        row_floor = np.where(lse == lse, FLOOR32, lse)
        t = (v - lse[:, None, None, None, None]).astype(np.float32)
        if fault != "no_floor":
            t = np.where(np.isnan(t) | np.isnan(row_floor)[:, None, None, None, None], np.float32(np.nan),
                         np.maximum(t, row_floor[:, None, None, None, None]))
        qp = np.minimum(q + 64, n4 - 1) if fault == "prior_neighbour" else qc
        o = _fma32(t, np.broadcast_to(scale, t.shape), np.broadcast_to(table[4 * qp + e][None], t.shape))
    out = np.zeros((T, n), np.float32)
    # vec_out: one 16-byte store per chunk, inside the row or dropped whole (n % 4 == 0); otherwise four 4-byte stores,
    # each range-checked against the row's n floats
    live = col < n
    if fault == "last_col_unwritten" and n % 4 != 0:
        live = live & (col != n - 1)
    out[:, col[live]] = o[:, live]
    return out


def ulp32(v):
    v = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)
