"""The layer kinds 4 to 8, restated in numpy for the tests; not collected by pytest.
  * the five rules.  E is libm's expf, called through ctypes element by element: independent of csrc/pk_expf.h, which
    the library computes it with
  * the designed inputs
  * a composer of expected log-likelihoods: every affine layer through oracle.Nnet([linear]).propagate (the GPU's affine
    layers are bit-identical to it), relu / normalize / softmax through the oracle's, the new kinds through the rules
    here, and the tail of am.cc:106-112 in float32."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O                                                 # noqa: E402

_libm = C.CDLL("libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]

F32 = np.float32


def E(x):
    x = np.ascontiguousarray(x, F32)
    flat = x.ravel()
    return np.array([_libm.expf(float(v)) for v in flat], F32).reshape(x.shape)


def _exp_side(x):
    x = np.ascontiguousarray(x, F32)
    pos = x > 0                                   # False for NaN: it takes the second branch
    with np.errstate(all="ignore"):
        e = E(np.where(pos, -x, x))
    return x, pos, e


def sigmoid(x):
    x, pos, e = _exp_side(x)
    e = e.astype(np.float64)
    with np.errstate(all="ignore"):
        y = np.where(pos, 1.0 / (1.0 + e), e / (e + 1.0))
    return y.astype(F32)


def tanh(x):
    x, pos, t = _exp_side(x)
    with np.errstate(all="ignore"):
        q = (t * t).astype(F32)                   # the float product
        r = 2.0 / (1.0 + q.astype(np.float64))
        y = np.where(pos, -1.0 + r, 1.0 - r)
    return y.astype(F32)


def pnorm(x, out_dim):
    x = np.ascontiguousarray(x, F32)
    T, D = x.shape
    assert D % out_dim == 0
    G = D // out_dim
    g3 = x.reshape(T, out_dim, G)
    s = np.zeros((T, out_dim), F32)
    with np.errstate(all="ignore"):
        for g in range(G):
            p = (g3[:, :, g] * g3[:, :, g]).astype(F32)
            s = (s + p).astype(F32)
        return np.sqrt(s).astype(F32)             # float32 sqrt: correctly rounded


def add(x, v):
    with np.errstate(all="ignore"):
        return (np.ascontiguousarray(x, F32) + np.ascontiguousarray(v, F32)[None, :]).astype(F32)


def mul(x, v):
    with np.errstate(all="ignore"):
        return (np.ascontiguousarray(x, F32) * np.ascontiguousarray(v, F32)[None, :]).astype(F32)


def apply(kind, x, param=None):
    return {"sigmoid": lambda: sigmoid(x), "tanh": lambda: tanh(x), "pnorm": lambda: pnorm(x, param), "add": lambda: add(x, param),
            "mul": lambda: mul(x, param)}[kind]()


# ---------------------------------------------------------------- designed inputs

# finite: signed zeros, tiny values, subnormals (the smallest, the largest, one in between), the branch point's
# neighbours, the ranges where expf saturates sigmoid / tanh (17), overflows its argument's square (88) and underflows
# (104); 2e19: its square overflows the p-norm's float sum
FINITE = np.array([0.0, -0.0, 1e-8, -1e-8, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 5.877472e-39, -5.877472e-39, 1.0, -1.0, 17.0, -17.0,
                   88.0, -88.0, 104.0, -104.0, 2e19, -2e19], F32)
NONFINITE = np.array([np.inf, -np.inf, np.nan], F32)


def designed(T, D, seed):
    """[T][D]: seeded normals (sigma 3) with the FINITE values written over up to 60 of them (all of them, three times,
    from 60 elements on); for T >= 8 the three NONFINITE values in three rows (an affine layer in front spreads a
    non-finite value over its whole row: 0 * inf)."""
    rng = np.random.default_rng([0x1A7E, seed, T, D])
    x = (rng.standard_normal((T, D)) * 3.0).astype(F32)
    flat = x.reshape(-1)
    n = flat.shape[0]
    where = rng.choice(n, size=min(n, 3 * len(FINITE)), replace=False)
    flat[where] = FINITE[np.arange(where.shape[0]) % len(FINITE)]
    if T >= 8:
        for k, t in enumerate((T // 3, T // 2, T - 2)):
            x[t, int(rng.integers(0, D))] = NONFINITE[k]
    return x


def same(got, want):
    """Bit for bit, NaN for NaN (a NaN's payload is not part of any rule here)."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


# ---------------------------------------------------------------- composer

def propagate(layers, x):
    """The network's raw output rows for input rows x [T][in_dim] (already spliced)."""
    x = np.ascontiguousarray(x, F32)
    for l in layers:
        if l[0] == "linear":
            x = O.Nnet([l]).propagate(x)
        elif l[0] == "relu":
            x = O.relu(x)
        elif l[0] == "normalize":
            x = O.normalize_rows(x)
        elif l[0] == "softmax":
            x = O.softmax_rows(x)
        else:
            x = apply(l[0], x, l[1] if len(l) > 1 else None)
    return x


def loglik(layers, feats, prior, left, right, scale):
    """pk_decodable_init's rows for CMVN'd features [T][feat_dim] (softmax mode "reference"): the network on the spliced
    rows, then am.cc:106-112 and decodable.cc:15 -- floor at 1e-20, libm logf, minus the log prior, times the scale."""
    feats = np.ascontiguousarray(feats, F32)
    if feats.shape[0] == 0:
        return np.zeros((0, len(prior)), F32)
    y = propagate(layers, O.splice(feats, left, right))
    lp = O.logf(np.ascontiguousarray(prior, F32))
    with np.errstate(all="ignore"):
        p = np.where(y < F32(1e-20), F32(1e-20), y).astype(F32)
        t = O.logf(p).reshape(p.shape)
        return ((t + F32(-1.0) * lp[None, :]).astype(F32) * F32(scale)).astype(F32)


# ---------------------------------------------------------------- the stack of the GPU tests

STACK_FEAT_DIM, STACK_LEFT, STACK_RIGHT, STACK_PDFS = 6, 2, 1, 7
STACK_LENGTHS = [1, 3, 64, 67, 129]


def _linear(rng, n_in, n_out):
    return ("linear", (rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(F32), (rng.standard_normal(n_out) * 0.1).astype(F32))


def stack():
    """feat_dim 6, left 2 / right 1 (input 24): Linear 24->40, p-norm ->10, Normalize, Linear 10->34, p-norm ->17,
    Linear 17->12, tanh, Linear 12->9, sigmoid, Linear 9->7, mul, add, Softmax.  The widths 10 and 17 are no multiples of
    16 on purpose.  -> (layers, prior)"""
    rng = np.random.default_rng(0x57AC)
    layers = [_linear(rng, 24, 40), ("pnorm", 10), ("normalize",), _linear(rng, 10, 34), ("pnorm", 17), _linear(rng, 17, 12), ("tanh",),
              _linear(rng, 12, 9), ("sigmoid",), _linear(rng, 9, 7), ("mul", rng.uniform(0.5, 2.0, 7).astype(F32)),
              ("add", rng.standard_normal(7).astype(F32)), ("softmax",)]
    prior = rng.uniform(0.05, 0.3, STACK_PDFS).astype(F32)
    return layers, prior


def stack_feats():
    return [(np.random.default_rng([0xFEA7, u, T]).standard_normal((T, STACK_FEAT_DIM)) * 1.5).astype(F32) for u, T in enumerate(STACK_LENGTHS)]
