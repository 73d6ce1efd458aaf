"""The arithmetic of the fp16 matrix-core modes (csrc/gemm_f16.hip, capi_exec.hip: RunLayersF16) as plain numpy, in
float64.  No GPU, no product code.

  operand      Split(clamp(x 2^e_in)), Split(W 2^e_w):  hi = fp16(v), lo = fp16(v - hi), clamp at +-65504
  accumulator  sum_k  hi hi + hi lo + lo hi   ("f16x3", terms = 3);   hi hi only ("f16", terms = 1)
  epilogue     one fma(acc, 2^(e_out - e_in - e_w), bias 2^e_out), then ReLU; written as fp32 (e_out = 0: the last
               layer, or the input of a Normalize) or re-split into the next layer's operand
  Normalize    y = x float(sqrt(n / sum x^2)) 2^e_x on the fp32 rows, an all-zero row stays zero, then Split

The GPU sums in fp32 in an order of its own; this model sums in float64.  The two agree bit for bit whenever no sum
rounds, and `exactness_guard` states a condition under which none can: every product term of a GEMM is a multiple of
one power of two g, and sum_k |term| <= 2^21 g for every output.  All partial sums, in ANY order and association, are
then multiples of g below 2^21 g: 22-bit integers times g, exact in any accumulator of at least fp32's 24 bits.  2^21
is a construction condition (3 bits of slack under fp32), never fitted to what a kernel returns.
"""
import numpy as np

F16_MAX = 65504.0
RANGE_TOO_SMALL = 2.0 ** -5          # capi_exec.hip: EvalRange (pk_host.h: kRangeTooSmall)
SPAN_CAP_LOG2 = 21


class NotExact(AssertionError):
    """A case is not provably exact: the construction (not the kernel) has to change."""


def split(x):
    x = np.clip(x.astype(np.float32), -65504.0, 65504.0)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def f16x3_matmul(X, W):
    xh, xl = split(X)
    wh, wl = split(W)
    return xh @ wh.T + xh @ wl.T + xl @ wh.T           # fp64 sums: isolates the operand error from the accumulation order


def finalize_exponent(W):
    """capi_model.hip, pk_mi355_am_finalize: 13 - ilogb(max |W|), clamped to +-60."""
    m = np.abs(W).max()
    return 0 if m == 0 else int(np.clip(13 - int(np.floor(np.log2(m))), -60, 60))


# ------------------------------------------------------------------ the exactness guard

def lowest_bit(a):
    """The value of the lowest set mantissa bit of every element (inf for zeros): a is an odd multiple of it."""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)
    mi = np.abs(np.ldexp(m, 53)).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    with np.errstate(over="ignore"):
        return np.where(a == 0, np.inf, np.ldexp(low, e - 53))


def _is_f32(a):
    with np.errstate(over="ignore"):
        return bool(np.all(np.isfinite(a)) and np.array_equal(a.astype(np.float32).astype(np.float64), a))


def _family_g(a, b):
    """Largest power of two dividing every non-zero product a[i][k] b[j][k]: the lowest bit of a product is the
    product of the lowest bits, so the minimum is taken column by column."""
    if a.size == 0 or b.size == 0:
        return np.inf
    return float(np.min(lowest_bit(a).min(axis=0) * lowest_bit(b).min(axis=0)))


def exactness_guard(xop, wop, terms):
    """Raises NotExact unless the GEMM of these operand halves is exact in any fp32-or-wider accumulator in any
    order.  Returns log2 of the span max_out sum_k |term| / g (-inf when every product is zero)."""
    (xh, xl), (wh, wl) = xop, wop
    if terms == 3 and xl.any() and wl.any():
        raise NotExact("both operands carry lo halves: the dropped lo x lo term is not zero")
    fams = [(xh, wh)] + ([(xh, wl), (xl, wh)] if terms == 3 else [])
    g = min(_family_g(a, b) for a, b in fams)
    if not np.isfinite(g):
        return -np.inf
    span = sum(np.abs(a) @ np.abs(b).T for a, b in fams).max() / g
    if span > 2.0 ** SPAN_CAP_LOG2:
        raise NotExact("sum |terms| = 2^%.2f g, the cap is 2^%d g" % (np.log2(span), SPAN_CAP_LOG2))
    return float(np.log2(span)) if span > 0 else -np.inf


# ------------------------------------------------------------------ one layer, Normalize, a stack

def _operand(x, e_in):
    if isinstance(x, tuple):
        return x
    return split(np.asarray(x, np.float32) * np.float32(2.0 ** e_in))


def f16_layer(x, W, b, e_in, e_w, e_out, terms, relu, guard=None):
    """x: fp32 [T][K] (split here as x 2^e_in) or the (hi, lo) operand a previous layer returned (already scaled by
    2^e_in).  e_out None: the fp32 output [T][N]; otherwise the (hi, lo) operand of the next layer, split after
    scaling by 2^e_out.  guard: a list -- the exactness guard is asserted and the GEMM's span (log2) appended."""
    xh, xl = xop = _operand(x, e_in)
    wh, wl = wop = split(np.asarray(W, np.float32) * np.float32(2.0 ** e_w))
    acc = xh @ wh.T
    if terms == 3:
        acc = acc + xh @ wl.T + xl @ wh.T
    eo = 0 if e_out is None else e_out
    bb = np.asarray(b, np.float32).astype(np.float64) * 2.0 ** eo
    if guard is not None:
        guard.append(exactness_guard(xop, wop, terms))
        if not _is_f32(acc):
            raise NotExact("accumulator not representable in fp32")
    acc = acc.astype(np.float32).astype(np.float64)
    a = acc * 2.0 ** (eo - e_in - e_w)
    v = a + bb[None, :]
    if guard is not None:
        if not (np.array_equal(v - a, np.broadcast_to(bb, v.shape)) and np.array_equal(v - bb, a)):
            raise NotExact("acc + bias rounds in float64")
        if not (_is_f32(a) and _is_f32(bb) and _is_f32(v)):
            raise NotExact("scaled accumulator, bias or output not representable in fp32")
    v = v.astype(np.float32)
    if relu:
        v = np.maximum(v, np.float32(0.0))
    return v if e_out is None else split(v)


def normalize_split(v, e_x, guard=None):
    """NormalizeSplitKernel: fp32 rows in, the next layer's (hi, lo) operand out."""
    v = np.asarray(v, np.float32).astype(np.float64)
    n = v.shape[1]
    sq = v * v
    ssq = sq.sum(axis=1)
    if guard is not None:
        g = lowest_bit(sq).min(axis=1)
        if not (_is_f32(sq) and _is_f32(ssq) and np.all(ssq[np.isfinite(g)] <= 2.0 ** SPAN_CAP_LOG2 * g[np.isfinite(g)])):
            raise NotExact("the sum of squares can round")
    nz = ssq > 0
    scale = np.zeros_like(ssq)
    scale[nz] = np.sqrt(float(n) / ssq[nz].astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    if guard is not None and not np.array_equal(scale[nz] * scale[nz] * ssq[nz], np.full(int(nz.sum()), float(n))):
        raise NotExact("sqrt(n / ssq) is not exact")
    y = v * (scale * 2.0 ** e_x)[:, None]
    if guard is not None and not _is_f32(y):
        raise NotExact("normalized values not representable in fp32")
    return split(y.astype(np.float32))


def f16_stack(x, layers, w_exp, x_exp, terms, guard=None, operands=None):
    """RunLayersF16 on (Linear [ReLU] [Normalize])+: layers as pocketkaldi_amd.AcousticModel takes them, w_exp / x_exp
    as AcousticModel.exponents() returns them.  Returns the fp32 output of the last affine layer.  operands: a list
    that receives the (hi, lo) operand of every affine layer."""
    kinds = [l[0] for l in layers]
    lin = [i for i, k in enumerate(kinds) if k == "linear"]
    op = _operand(x, int(x_exp[0]))
    for li, i in enumerate(lin):
        if operands is not None:
            operands.append(op)
        relu = i + 1 < len(kinds) and kinds[i + 1] == "relu"
        after = i + 1 + (1 if relu else 0)
        norm = after < len(kinds) and kinds[after] == "normalize"
        e_out = None if (li == len(lin) - 1 or norm) else int(x_exp[li + 1])
        op = f16_layer(op, layers[i][1], layers[i][2], int(x_exp[li]), int(w_exp[li]), e_out, terms, relu, guard)
        if norm:
            op = normalize_split(op, int(x_exp[li + 1]), guard)
    return op


def operands_in_range(operands):
    """What EvalRange accepts: max |hi| of every operand below the clamp and, unless the operand is all zero, >= 2^-5."""
    for hi, _ in operands:
        m = np.abs(hi).max() if hi.size else 0.0
        if m >= F16_MAX or 0.0 < m < RANGE_TOO_SMALL:
            return False
    return True
