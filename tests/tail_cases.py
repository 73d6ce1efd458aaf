"""Designed logits for the log-likelihood tail (csrc/pk_tail_wave.h, csrc/tail.hip).

The tail cannot be called alone; pocketkaldi_amd.Decodable(am, scale, feats) with no splice context and
layers = [("linear", W, b), ("softmax",)] reaches it.  The fp32 GEMM is a k-ordered FMA chain, so with feats[t] one-hot at
d, b = 0 and W finite, row t of the logits IS column d of W (adding 0 * w adds +-0): P designed rows make a model with
K = P inputs, and feats chooses which row pattern each frame gets (frame t gets pattern t mod P; P is odd, so a row read
from the wrong place of a 4-row workgroup or a 128-row tile shows).  Infinite logits come from the bias (0 * inf is NaN).
The fused tail needs an affine layer in front of the last one (the first layer of the scoring path writes feature-major
panels, which no tail reads): an identity layer, which hands the one-hot rows on unchanged.

A case holds the pattern matrix X[P][n], a kind per pattern and, for the "bits" kind, the exact t = max(x - lse, floor):
  bits    one column holds M, a power of two (M log2 e is a float, the peak's exponent argument is exactly 0), the rest
          lie >= 32 below: every other term is < 2^-46, s = 1.0f and lse = M exactly in any summation order, so the
          output is predict_bits(...) bit for bit.  The rest is M - 32 (not floored) or M - 64 (floored); at M = +-2^127,
          where M - 32 is no float, it is the float next below M (2^103 / 2^104 away: floored).
  flat    every column 0: s = n exactly in any order; one column dropped or doubled moves lse by >= 1 / 8192.
          Tolerance: two ulps of log n times the scale plus one ulp of the output.
  bound   compared with tail_model.reference under tail_model.error_bound.
  nan     the whole row is NaN.
test_tail_cases.py checks all of this without a GPU; test_gpu_tail_edges.py runs it on one.
"""
import functools

import numpy as np

import tail_model as M

TILE = 128
SCALES = (0.125, 0.1)              # a power of two (both forms owe the same bits at prior 1) and one that is none

STANDALONE_WIDTHS = [1, 3, 4, 5, 255, 256, 257, 700, 768, 769, 1023, 1024, 1025, 1501, 1792, 1793, 2048, 2049, 2817, 3000,
                     3001, 3072, 3073, 3841, 4095, 4096, 4097, 5000, 5889, 6100, 6143, 6144, 6145, 7936, 7937, 8000, 8191,
                     8192]
FUSED_WIDTHS = [1000, 1024, 1800, 2048, 3000, 3072, 4096, 6100, 6144, 8000, 8192]
KERNEL_WIDTHS = [1, 5, 1023, 1024, 1025, 3072, 3073, 8191, 8192, 8193, 8200]
REFERENCE_WIDTHS = [3008, 3009, 8000]
PLAIN_WIDTHS = [1024, 1025, 8193]
SINGLE_PASS_ROWS = 4096            # pk_decodable_init walks an utterance in passes of 4 096 frames (pk_score.h: kSingleChunk)

PEAKS = [(0.0, -32.0), (0.0, -64.0), (2.0 ** 10, -32.0), (2.0 ** 10, -64.0), (-2.0 ** 10, -32.0), (-2.0 ** 10, -64.0),
         (2.0 ** 127, None), (-2.0 ** 127, None)]


# ------------------------------------------------------------------ routes (the documented rules, restated)

def tiles_j(n):
    return (n + TILE - 1) // TILE


def strip_eligible(n):
    """capi_exec.hip: the last column tile goes through a 64 x 64 strip launch when at most 64 of its columns are real."""
    return tiles_j(n) > 8 and n <= (tiles_j(n) - 1) * TILE + TILE // 2


def fused_route(rows, n, min_tiles=384):
    """"fused" / "fused+strip" / "wave": what a launch of `rows` rows takes in fp32 stable mode behind an affine layer
    (GemmFusesTail: tiles_i * tiles_j >= 384 and a row of exactly 4 / 8 / 12 / 16 / 24 / 32 chunks)."""
    ti = (rows + TILE - 1) // TILE
    if not (ti * tiles_j(n) >= min_tiles and M.wave_shape(n)[2]):
        return "wave"
    return "fused+strip" if strip_eligible(n) and ti * (tiles_j(n) - 1) >= min_tiles else "fused"


def fused_row_counts(n):
    """Row counts (<= one 4 096-row pass) at which the launch fuses with the fewest row tiles -- the last tile holding one
    row, and full -- and the same where the strip launch joins in.  Empty where one pass cannot hold 384 tiles."""
    need = {-(-384 // tiles_j(n))}
    if strip_eligible(n):
        need.add(-(-384 // (tiles_j(n) - 1)))
    return [r for ti in sorted(need) for r in ((ti - 1) * TILE + 1, ti * TILE) if r <= SINGLE_PASS_ROWS]


# ------------------------------------------------------------------ patterns

def peak_columns(n):
    """The columns where a row maximum must be tried: chunk, group, wave-half, strip and row edges."""
    n4 = (n + 3) >> 2
    cols = [0, 3, 4, 255, 256, n - 1, n - 2, 4 * (n4 - 1), 256 * (n4 // 64) - 1, 256 * (n4 // 64), TILE * (tiles_j(n) - 1)]
    if n <= 8192 and M.wave_shape(n)[1]:
        C = M.wave_shape(n)[0]
        cols += [256 * C - 1, 256 * C]
    return sorted({c for c in cols if 0 <= c < n})


def _below(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def _peak_row(n, col, m, off):
    rest = _below(m) if off is None else np.float32(m + off)
    x = np.full(n, rest, np.float32)
    x[col] = m
    t = (x - np.float32(m)).astype(np.float32)                        # exact: 0, -32, -64 or one ulp of 2^127
    return x, np.maximum(t, M.FLOOR32)


@functools.lru_cache(maxsize=4)
def main_case(n):
    """Every finite family at width n: {"key", "n", "X", "kinds", "names", "t"} (t: NaN outside the bits rows)."""
    rows, kinds, names, ts = [], [], [], []

    def add(name, x, kind, t=None):
        rows.append(np.asarray(x, np.float32))
        kinds.append(kind)
        names.append(name)
        ts.append(np.full(n, np.nan, np.float32) if t is None else t)

    for i, col in enumerate(peak_columns(n)):
        for v in (range(8) if col in (0, n - 1) else [(3 * i + k) % 8 for k in range(3)]):
            x, t = _peak_row(n, col, *PEAKS[v])
            add("peak %g at %d, rest %s" % (PEAKS[v][0], col, PEAKS[v][1]), x, "bits", t)
    add("flat 0", np.zeros(n), "flat")
    add("flat 1024", np.full(n, 1024.0), "bound")
    j = np.arange(n)
    for zero_at in sorted({0, n - 1}):                                 # floor straddle: log 1e-20 = -46.05 lies inside [-47, -45]
        x = -47.0 + (j % 33) / 16.0
        x[zero_at] = 0.0
        add("straddle, 0 at %d" % zero_at, x, "bound")
    rng = np.random.default_rng([0x7A11, n])
    for std in (1, 10, 40):
        base = rng.standard_normal(n) * std
        for shift in (0, 1000, -1000):
            add("spread %d%+d" % (std, shift), base + shift, "bound")
    x = rng.standard_normal(n)
    x[1::5] = -3e38                                                    # far below, beside ordinary ones
    add("mix -3e38", x, "bound")
    if len(rows) % 2 == 0:
        add("flat 0", np.zeros(n), "flat")
    return {"key": ("main", n), "n": n, "X": np.stack(rows), "kinds": tuple(kinds), "names": tuple(names), "t": np.stack(ts)}


def _subset(c, key, keep):
    if len(keep) % 2 == 0:
        keep = keep[:-1]
    return {"key": key, "n": c["n"], "X": c["X"][keep], "kinds": tuple(c["kinds"][i] for i in keep),
            "names": tuple(c["names"][i] for i in keep), "t": c["t"][keep]}


@functools.lru_cache(maxsize=4)
def peaks_case(n):
    """The bits rows of main_case alone (an odd number of them): for launches of thousands of rows."""
    c = main_case(n)
    return _subset(c, ("peaks", n), [i for i, k in enumerate(c["kinds"]) if k == "bits"])


@functools.lru_cache(maxsize=4)
def f16_case(n):
    """The bits rows whose values (0, -32, -64) the fp16 split carries exactly."""
    c = main_case(n)
    return _subset(c, ("f16", n), [i for i, k in enumerate(c["kinds"]) if k == "bits" and np.abs(c["X"][i]).max() <= 64.0])


@functools.lru_cache(maxsize=4)
def small_case(n):
    """Five finite rows, the base of the models whose bias is infinite."""
    c = main_case(n)
    keep = [c["names"].index(name) for name in ("flat 0", "straddle, 0 at 0", "spread 1+0", "spread 10+0", "spread 40-1000")]
    return _subset(c, ("small", n), keep)


def infinite_cases(n):
    """[(name, case with a "bias")]: a few columns -inf (those are floor, the rest right), all -inf (NaN), one +inf (the
    whole row NaN in stable mode)."""
    base = small_case(n)
    out = []
    for name, cols, v in (("some -inf", sorted({0, n // 2, n - 1}), -np.inf), ("all -inf", list(range(n)), -np.inf),
                          ("one +inf", [n - 1], np.inf)):
        b = np.zeros(n, np.float32)
        b[cols] = v
        nan = v > 0 or len(cols) == n
        out.append((name, dict(base, key=(name, n), bias=b, kinds=("nan",) * 5 if nan else ("bound",) * 5)))
    return out


@functools.lru_cache(maxsize=4)
def range_case(n):
    """Row maxima past FLT_MAX / log2 e = 2.36e38, where the wave form's -m * log2 e overflows (pk_tail_wave.h: the
    documented domain).  Pattern 0: 2.5e38 in column 0, the rest 0.  Pattern 1: every column -2.5e38 but the last, which
    holds -3e38.  Pattern 2: all zero (an ordinary row between them)."""
    X = np.zeros((3, n), np.float32)
    X[0, 0] = 2.5e38
    X[1, :] = -2.5e38
    X[1, n - 1] = -3e38
    return {"key": ("range", n), "n": n, "X": X, "kinds": ("range+", "range-", "flat"), "t": np.full((3, n), np.nan, np.float32)}


@functools.lru_cache(maxsize=4)
def reference_case(n):
    """The finite families with |x| <= 80 (the reference's own expf overflows at 88.7)."""
    c = main_case(n)
    case = _subset(c, ("reference", n), [i for i in range(len(c["kinds"])) if np.abs(c["X"][i]).max() <= 80.0])
    assert {"bits", "flat", "bound"} <= set(case["kinds"])
    return case


@functools.lru_cache(maxsize=4)
def plain_case(n):
    """Non-negative rows for the tail without a softmax layer (a ReLU net): peaks over zeros, and zeros."""
    rows = [np.zeros(n, np.float32)]
    for i, col in enumerate(peak_columns(n)):
        x = np.zeros(n, np.float32)
        x[col] = (1.0, 2.0 ** 10, 2.0 ** 127, 2.0 ** -70)[i % 4]
        rows.append(x)
    if len(rows) % 2 == 0:
        rows.append(np.full(n, 0.5, np.float32))
    return {"key": ("plain", n), "n": n, "X": np.stack(rows)}


def prior(n, kind):
    """"ones": log prior exactly 0.  "varied": distinct per column over a factor of two, period 37 (coprime to 64)."""
    if kind == "ones":
        return np.ones(n, np.float32)
    return ((37.0 + np.arange(n) % 37) / (74.0 * n)).astype(np.float32)


def log_prior32(p):
    """What the model holds: the C library's logf of the float32 prior (am.cc:43)."""
    from oracle import oracle as O
    return O.logf(p)


# ------------------------------------------------------------------ models and features

def layers(case, identity_first=False, softmax=True, pad_k=1):
    """[("linear", W, b), ("softmax",)] whose logits for a one-hot frame at d are pattern d."""
    X = case["X"]
    P, n = X.shape
    K = -(-P // pad_k) * pad_k
    W = np.zeros((n, K), np.float32)
    W[:, :P] = X.T
    out = [("linear", np.eye(K, dtype=np.float32), np.zeros(K, np.float32))] if identity_first else []
    out.append(("linear", W, case.get("bias", np.zeros(n, np.float32))))
    return out + ([("softmax",)] if softmax else [])


def features(case, rows, pad_k=1):
    P = case["X"].shape[0]
    K = -(-P // pad_k) * pad_k
    f = np.zeros((rows, K), np.float32)
    f[np.arange(rows), np.arange(rows) % P] = 1.0
    return f


def logits(case):
    """The float32 logits the tail sees for each pattern."""
    with np.errstate(invalid="ignore"):
        return (case["X"] + case.get("bias", np.float32(0.0))).astype(np.float32)


# ------------------------------------------------------------------ the assertion (CPU model and GPU alike)

@functools.lru_cache(maxsize=6)
def _expect(case_key, prior_kind, scale, form):
    case = _CASES[case_key]
    n, x, p = case["n"], logits(case), prior(case["n"], prior_kind)
    ref = M.reference(x, p, scale)
    tol = M.error_bound(x, p, scale, form)
    bits = np.zeros_like(x)
    for i, k in enumerate(case["kinds"]):
        if k == "flat":                                                # (and the log prior's: the host's logf, 1 ulp, and its product
            lp = np.abs(np.log(p.astype(np.float64)))                  # with the scale: 3 u |log prior|, as in error_bound)
            tol[i] = float(np.float32(scale)) * (2.0 * M.ulp32(np.log(n)) + 3.0 * M.U * lp) + M.ulp32(ref[i])
    rows = [i for i, k in enumerate(case["kinds"]) if k == "bits"]
    if rows:
        bits[rows] = M.predict_bits(case["t"][rows], log_prior32(p), scale, form)
    return ref, tol, bits


_CASES = {}


def check(case, got, scale, prior_kind, form, where=""):
    """got[r] is the tail's output for pattern r mod P.  Raises AssertionError naming `where` (the route), the pattern,
    its kind and the column; returns the largest err / bound seen over the bound and flat rows."""
    key = case["key"]
    _CASES[key] = case
    ref, tol, bits = _expect(key, prior_kind, float(scale), form)
    P, n = case["X"].shape
    got = np.ascontiguousarray(got, np.float32)
    assert got.shape[1] == n, (where, got.shape, n)
    worst = 0.0
    for p in range(min(P, got.shape[0])):
        g, kind = got[p::P], case["kinds"][p]
        tag = "%s n=%d scale=%g prior=%s pattern %d (%s: %s)" % (where, n, scale, prior_kind, p, kind, case["names"][p])
        if kind == "bits":
            bad = np.argwhere(g.view(np.uint32) != bits[p].view(np.uint32)[None, :])
            assert bad.size == 0, ("%s: %d values differ from the predicted bits, first at row %d column %d: got %r, want %r; "
                                   "the reference there %r" % (tag, len(bad), bad[0][0] * P + p, bad[0][1], g[tuple(bad[0])],
                                                               bits[p][bad[0][1]], ref[p][bad[0][1]]))
            assert np.all(np.abs(bits[p].astype(np.float64) - ref[p]) <= tol[p]), tag + ": the prediction leaves the bound"
        elif kind == "nan":
            assert np.isnan(g).all(), "%s: %d of %d values are not NaN" % (tag, (~np.isnan(g)).sum(), g.size)
        else:
            err = np.abs(g.astype(np.float64) - ref[p][None, :])
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(err == 0, 0.0, err / tol[p][None, :])
            ok = ratio <= 1.0                                          # (a NaN where a number is owed fails)
            if not ok.all():
                r, c = np.argwhere(~ok)[0]
                raise AssertionError("%s: %d values outside the bound, first at row %d column %d: got %r, reference %r, err %.3e, "
                                     "bound %.3e (err / bound %.3g)" % (tag, (~ok).sum(), r * P + p, c, g[r, c], ref[p][c],
                                                                         err[r, c], tol[p][c], ratio[r, c]))
            worst = max(worst, float(ratio.max()))
    return worst
