"""The time-splice layer, kind 9, restated in numpy for the tests; not collected by pytest.
  * the layer in its shrinking form: rows [T][D] -> [T - lo - hi][n D]
  * loglik_time: the expected log-likelihoods of a network with such layers under the edge rule -- the normalised
    features extended by Lh / Rh copies of the first / last frame, the first layer's splice over the extended rows, every
    layer through layer_cases.propagate's rules with the time-splice shrinking the row set, and layer_cases.loglik's tail
    on the T rows that are left
  * the WRONG rule (every hidden splice clamped at the utterance's own edge), which the GPU tests must be able to tell
    from the right one
  * the stack of the GPU tests."""
import numpy as np

import layer_cases as LC
from layer_cases import F32, O


def lo_hi(offsets):
    return max(0, -int(offsets[0])), max(0, int(offsets[-1]))


def time_splice(x, offsets):
    """[T][D] -> [T - lo - hi][n D]: output row r is the input frames r + lo + o_c side by side, bits kept."""
    x = np.ascontiguousarray(x, F32)
    lo, hi = lo_hi(offsets)
    rows = x.shape[0] - lo - hi
    assert rows > 0
    return np.ascontiguousarray(np.concatenate([x[lo + o:lo + o + rows] for o in offsets], axis=1))


def time_splice_clamped(x, offsets):
    """The wrong rule: [T][D] -> [T][n D], frame t + o_c clamped to [0, T)."""
    x = np.ascontiguousarray(x, F32)
    T = x.shape[0]
    t = np.arange(T)
    return np.ascontiguousarray(np.concatenate([x[np.clip(t + o, 0, T - 1)] for o in offsets], axis=1))


def time_context(layers):
    Lh = Rh = 0
    for l in layers:
        if l[0] == "splice":
            lo, hi = lo_hi(l[1])
            Lh, Rh = Lh + lo, Rh + hi
    return Lh, Rh


def propagate_time(layers, x, splice=time_splice):
    """layer_cases.propagate with the time-splice layers in between (the runs of other layers go through it unchanged)."""
    run = []
    for l in layers:
        if l[0] == "splice":
            x = splice(LC.propagate(run, x), l[1])
            run = []
        else:
            run.append(l)
    return LC.propagate(run, x)


def _tail(y, prior, scale):
    """layer_cases.loglik's tail on finished rows (no layer, no context: its splice and its network are the identity)."""
    return LC.loglik([], y, prior, 0, 0, scale)


def loglik_time(layers, feats, prior, left, right, scale):
    """The rows of a whole-utterance scorer for normalised features [T][feat_dim] (softmax mode "reference")."""
    feats = np.ascontiguousarray(feats, F32)
    T = feats.shape[0]
    if T == 0:
        return np.zeros((0, len(prior)), F32)
    Lh, Rh = time_context(layers)
    ext = np.concatenate([np.repeat(feats[:1], Lh, axis=0), feats, np.repeat(feats[-1:], Rh, axis=0)], axis=0)
    y = propagate_time(layers, O.splice(ext, left, right))
    assert y.shape[0] == T
    return _tail(y, prior, scale)


def loglik_wrong(layers, feats, prior, left, right, scale):
    """The same network with every hidden splice clamped at the utterance's own edge: NOT what the library computes."""
    feats = np.ascontiguousarray(feats, F32)
    if feats.shape[0] == 0:
        return np.zeros((0, len(prior)), F32)
    return _tail(propagate_time(layers, O.splice(feats, left, right), time_splice_clamped), prior, scale)


# ---------------------------------------------------------------- the stack of the GPU tests (test 3d)

FEAT_DIM, LEFT, RIGHT, PDFS, LH, RH = 6, 2, 1, 7, 4, 5
LENGTHS = [1, 3, 0, 64, 67, 129, 2]
SCALE = 0.1


def stack():
    """feat_dim 6, left 2 / right 1: Linear 24->40, p-norm ->10, Normalize, splice [-1, 2], Linear 20->34, ReLU, splice
    [-3, 3], Linear 68->12, tanh, Linear 12->7, Softmax.  Lh = 4, Rh = 5.  -> (layers, prior)"""
    rng = np.random.default_rng(0x7D33)
    layers = [LC._linear(rng, 24, 40), ("pnorm", 10), ("normalize",), ("splice", [-1, 2]), LC._linear(rng, 20, 34), ("relu",), ("splice", [-3, 3]),
              LC._linear(rng, 68, 12), ("tanh",), LC._linear(rng, 12, 7), ("softmax",)]
    prior = rng.uniform(0.05, 0.3, PDFS).astype(F32)
    return layers, prior


def feats_of(lengths, seed=0):
    return [(np.random.default_rng([0x7FEA, seed, u, T]).standard_normal((T, FEAT_DIM)) * 1.5).astype(F32) for u, T in enumerate(lengths)]


def stack_feats():
    return feats_of(LENGTHS)
