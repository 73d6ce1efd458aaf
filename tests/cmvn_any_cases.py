"""CMVN at any feature dimension: the chunk rule, and the inputs of the tests that use it.

cmvn.cc is elementwise in the feature index, so the 40-dim oracle is the yardstick at every D: column d of a [T][D]
matrix must equal, bit for bit, oracle.cmvn on any [T][40] matrix that holds that column, with the column's global sum
in the same position and the global count in entry 40.  cmvn_any states that rule once: chunks of 40 columns,
zero-padded."""
import numpy as np

from oracle import oracle as O

WINDOW, GLOBAL_FRAMES = 600, 200     # cmvn.h:10-11
COUNT = 2500.0                       # the global statistics' frame count
BIG_COLUMN_MEAN = 1.0e4              # one column (D // 2) of every input sits around this value


def cmvn_any(stats, raw):
    """stats: D sums, then the count; raw: [T][D] float32 -> [T][D] float32, through oracle.cmvn 40 columns at a time."""
    stats = np.ascontiguousarray(stats, np.float32)
    raw = np.ascontiguousarray(raw, np.float32)
    T, D = raw.shape
    assert stats.shape == (D + 1,)
    out = np.zeros((T, D), np.float32)
    for d0 in range(0, D, 40):
        n = min(40, D - d0)
        g = np.zeros(41, np.float32)
        g[:n], g[40] = stats[d0:d0 + n], stats[D]
        x = np.zeros((T, 40), np.float32)
        x[:, :n] = raw[:, d0:d0 + n]
        out[:, d0:d0 + n] = O.cmvn(g, x)[:, :n]
    return out


def features(T, D, seed):
    """5 N(0, 1) + 3, and one column (D // 2) around 1e4."""
    x = (5.0 * np.random.default_rng([0xC3A7, seed, T, D]).standard_normal((T, D)) + 3.0).astype(np.float32)
    if T:
        x[:, D // 2] += np.float32(BIG_COLUMN_MEAN)
    return x


def stats_for(D):
    """Count 2500, sums mean x 2500 (means 3, and 1e4 + 3 in the big column)."""
    mean = np.full(D, 3.0, np.float64)
    mean[D // 2] += BIG_COLUMN_MEAN
    return np.concatenate([mean * COUNT, [COUNT]]).astype(np.float32)


def restated_chain(stats, raw, double_step):
    """The rule of the issue restated in numpy, every operation rounded to float32 as the kernels round it:
        acc = s + x_t; if t >= 600: acc += -x_{t-600}; s = (float)acc      in f64 (double_step) or in f32
        st  = s;  if t + 1 < 600: st += alpha[t] * g
        y_t = x_t + neg_scale[t] * st
    with alpha and neg_scale as BuildCmvnTables makes them (cmvn.cc:73-101).  With double_step it is the oracle; without,
    it is what a kernel that drops the widen / narrow step would compute."""
    stats = np.ascontiguousarray(stats, np.float32)
    raw = np.ascontiguousarray(raw, np.float32)
    T, D = raw.shape
    g, G = stats[:D], np.float32(stats[D])
    out = np.zeros((T, D), np.float32)
    s = np.zeros(D, np.float32)
    for t in range(T):
        if double_step:
            acc = s.astype(np.float64) + raw[t].astype(np.float64)
            if t >= WINDOW:
                acc = acc + -1.0 * raw[t - WINDOW].astype(np.float64)
            s = acc.astype(np.float32)
        else:
            s = s + raw[t]
            if t >= WINDOW:
                s = s + -raw[t - WINDOW]
        tt = min(t, WINDOW - 1)
        cnt, alpha = np.float32(tt + 1), np.float32(0.0)
        if tt + 1 < WINDOW:
            alpha = np.float32(min(float(WINDOW - (tt + 1)), float(GLOBAL_FRAMES)) / float(G))
            cnt = np.float32(cnt + np.float32(alpha * G))
        neg_scale = -np.float32(1.0 / float(cnt))
        st = s
        if t + 1 < WINDOW:
            st = s + (alpha * g).astype(np.float32)
        out[t] = raw[t] + (neg_scale * st).astype(np.float32)
    return out
