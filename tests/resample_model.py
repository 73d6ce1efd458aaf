"""The resampler's rule restated in numpy: the polyphase table in double, and the float32 sum
(acc = f32(acc + f32(w * x)), ascending taps, from +0.0) over a GIVEN table -- so that the GPU tests can hand it the
library's table and ask for the same bits.  No GPU, no library."""
import collections
import math

import numpy as np

FO = 16000
ZEROS = 6
Table = collections.namedtuple("Table", "rate Q P max_taps first count weights")    # weights: float64 [P][max_taps]


def plan(rate):
    g = math.gcd(rate, FO)
    return rate // g, FO // g


def table(rate):
    """first[P], count[P] and the weights in double (zero-padded rows), by the rule's own words."""
    fi = rate
    Q, P = plan(fi)
    fc = 0.99 * 0.5 * min(fi, FO)
    w = ZEROS / (2 * fc)
    first, count = np.zeros(P, np.int64), np.zeros(P, np.int64)
    rows = []
    for p in range(P):
        tau = p / FO
        lo, hi = int(math.floor((tau - w) * fi)) - 2, int(math.ceil((tau + w) * fi)) + 2
        taps = [i for i in range(lo, hi + 1) if abs(i / fi - tau) < w]
        assert taps == list(range(taps[0], taps[-1] + 1))
        first[p], count[p] = taps[0], len(taps)
        row = []
        for i in taps:
            d = i / fi - tau
            x = 2 * fc * d
            sinc = 1.0 if x == 0 else math.sin(math.pi * x) / (math.pi * x)
            window = 0.5 * (1 + math.cos(2 * math.pi * fc * d / ZEROS))
            row.append(2 * fc * sinc * window / fi)
        rows.append(row)
    max_taps = int(count.max())
    weights = np.zeros((P, max_taps), np.float64)
    for p, row in enumerate(rows):
        weights[p, :len(row)] = row
    return Table(rate, Q, P, max_taps, first, count, weights)


def with_weights(t, weights_f32):
    """t with another weight array (the library's float32 one)."""
    return t._replace(weights=np.asarray(weights_f32))


def num_output(t, n):
    return n * t.P // t.Q


def num_final(t, n, closed=False):
    """The outputs that are final once n inputs have arrived: every j below it has base + count[p] - 1 < n."""
    if closed:
        return num_output(t, n)
    j = 0
    if n > 0:
        j = max(0, (n - int((t.first + t.count).max())) // t.Q) * t.P      # every earlier unit's windows end below n
    while True:
        u, p = divmod(j, t.P)
        if int(t.first[p]) + u * t.Q + int(t.count[p]) - 1 >= n:
            return j
        j += 1


def outputs(t, x, x0, j0, j1):
    """Outputs [j0, j1) in float32 from the samples x = signal[x0 : x0 + len(x)]; anything outside reads +0.0."""
    x = np.asarray(x, np.float32)
    w32 = t.weights.astype(np.float32)
    max_taps = t.max_taps
    j = np.arange(j0, j1, dtype=np.int64)
    u, p = j // t.P, j % t.P
    base = t.first[p].astype(np.int64) + u * t.Q - x0
    cnt = t.count[p]
    acc = np.zeros(j.shape[0], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(max_taps):
            idx = base + k
            ok = (idx >= 0) & (idx < x.shape[0])
            xv = np.where(ok, x[np.clip(idx, 0, max(x.shape[0] - 1, 0))] if x.shape[0] else np.float32(0), np.float32(0)).astype(np.float32)
            term = (w32[p, k] * xv).astype(np.float32)
            acc = np.where(k < cnt, (acc + term).astype(np.float32), acc)
    return acc


def resample(t, x):
    """The whole signal."""
    x = np.asarray(x, np.float32)
    return outputs(t, x, 0, 0, num_output(t, x.shape[0]))


def resample_chunked(t, x, sizes):
    """The signal pushed in chunks of the given sizes and then closed: after every push the newly final outputs are
    computed from the samples still held (everything from the first sample the next output reads)."""
    x = np.asarray(x, np.float32)
    held = np.zeros(0, np.float32)
    x0 = received = produced = 0
    out = []
    pos = 0
    for size in list(sizes) + [None]:
        if size is None:
            final = num_final(t, received, closed=True)
        else:
            held = np.concatenate([held, x[pos:pos + size]])
            pos += size
            received = pos
            final = num_final(t, received)
        if final > produced:
            out.append(outputs(t, held, x0, produced, final))
            produced = final
        keep = max(x0, (produced // t.P) * t.Q + int(t.first.min()))     # nothing before this is read again
        held, x0 = held[keep - x0:], keep
    assert pos == x.shape[0]
    return np.concatenate(out) if out else np.zeros(0, np.float32)
