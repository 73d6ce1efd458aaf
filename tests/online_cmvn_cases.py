"""The yardstick of online CMVN (include/pk_mi355.h): a numpy restatement of the rule -- Kaldi's
OnlineCmvn::ComputeStatsForFrame, SmoothOnlineCmvnStats and ApplyCmvn, not compared with a Kaldi binary -- and the
inputs the tests share.  Every column is independent; the state S0, S1 is float64 and starts at 0.0.  For t ascending:

    1. S0 += (double)x[t];  S1 += (double)x[t] * (double)x[t]
    2. if t >= W:  S0 -= (double)x[t - W];  S1 -= (double)x[t - W] * (double)x[t - W]        (after the additions)
    3. N = min(t + 1, W)
    4. on copies s0, s1, N, every a + f * b a rounded product and a rounded add; nothing if N >= W;
       a speaker record with count C > 0: c = min(W - N, speaker_frames, C); if c > 0: f = c / C,
           s0 += f * spk[0], s1 += f * spk[1], N += f * C
       if still N < W and global_frames > 0: c = min(W - N, global_frames), f = c / G,
           s0 += f * glob[0], s1 += f * glob[1], N += f * G
    5. norm_cases.finalize and norm_cases.apply on (s0, s1, N), means always: y[t]

numpy works on float64 rows element by element and rounds every product and every sum once (no fma), so the loop over t
IS the order of every column.  Also here: four variants a wrong implementation might be, as switches -- the state
carried in float between frames, a fused apply, the window sums as differences of prefix sums, and the subtraction in
front of the addition -- for the tests that show the comparisons tell them apart."""
import numpy as np

import norm_cases as NC

SPECS = ((1, 0, 0), (2, 1, 1), (8, 3, 2), (50, 600, 200), (600, 600, 200))      # (cmn_window, speaker_frames, global_frames)
SPEAKER_COUNT = 37


def features(T, D, seed=7):
    return NC.features(T, D, seed)


def wide(T, D, seed=11):
    """N(0, 1) * 2^k, k uniform in [-30, 30]: double sums round at every step."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, D)) * np.exp2(rng.integers(-30, 31, (T, D)))).astype(np.float32)


def record(x, count=None):
    """A 2 x (D + 1) record: x's own statistics, scaled to `count` frames when one is given (0: the zero record)."""
    rec = NC.accumulate(x)
    if count is not None:
        D = x.shape[1]
        rec = rec * (count / rec[0, D]) if count else np.zeros_like(rec)
        rec[0, D] = count
    return rec


def smooth(s0, s1, n, W, speaker_frames, global_frames, glob, spk):
    """Step 4 for one frame's row of sums -> (s0, s1, N)."""
    D = s0.shape[0]
    n = float(n)
    if n >= W:
        return s0, s1, n
    if spk is not None and spk[0, D] > 0.0:
        C = float(spk[0, D])
        c = min(W - n, float(speaker_frames), C)
        if c > 0.0:
            f = c / C
            s0 = s0 + f * spk[0, :D]
            s1 = s1 + f * spk[1, :D]
            n = n + f * C
    if n < W and global_frames > 0:
        G = float(glob[0, D])
        c = min(W - n, float(global_frames))
        f = c / G
        s0 = s0 + f * glob[0, :D]
        s1 = s1 + f * glob[1, :D]
        n = n + f * G
    return s0, s1, n


def online_cmvn(x, W, speaker_frames, global_frames, norm_vars, glob=None, spk=None,
                float_state=False, fused=False, prefix=False, subtract_first=False):
    """The rule -> (y float32 [T][D], the window state behind the last frame: float64 [2][D + 1], row 0 the sums and the
    frames seen, row 1 the sums of squares and 0).  The four switches are the wrong variants."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    xd = x.astype(np.float64)
    glob = None if glob is None else np.asarray(glob, np.float64)
    spk = None if spk is None else np.asarray(spk, np.float64)
    acc = np.float32 if float_state else np.float64
    S0, S1 = np.zeros(D, acc), np.zeros(D, acc)
    P0, P1 = np.zeros((T + 1, D)), np.zeros((T + 1, D))                          # prefix sums (the `prefix` variant)
    y = np.zeros((T, D), np.float32)
    with np.errstate(all="ignore"):
        for t in range(T):
            v = xd[t].astype(acc)
            if prefix:
                P0[t + 1] = P0[t] + xd[t]
                P1[t + 1] = P1[t] + xd[t] * xd[t]
                lo = max(0, t + 1 - W)
                S0, S1 = P0[t + 1] - P0[lo], P1[t + 1] - P1[lo]
            elif subtract_first and t >= W:
                o = xd[t - W].astype(acc)
                S0 = S0 - o
                S1 = S1 - o * o
                S0 = S0 + v
                S1 = S1 + v * v
            else:
                S0 = S0 + v
                S1 = S1 + v * v
                if t >= W:
                    o = xd[t - W].astype(acc)
                    S0 = S0 - o
                    S1 = S1 - o * o
            s0, s1, n = smooth(S0.astype(np.float64), S1.astype(np.float64), min(t + 1, W), W, speaker_frames, global_frames, glob, spk)
            rec = np.zeros((2, D + 1))
            rec[0, :D], rec[1, :D], rec[0, D] = s0, s1, n
            offs, scale = NC.finalize(rec, True, norm_vars)
            y[t] = NC.apply(x[t], offs, scale, norm_vars, fused)
    state = np.zeros((2, D + 1))
    state[0, :D], state[1, :D], state[0, D] = S0, S1, T
    return y, state


def frame_counts(W):
    """The T values of the restatement test at window W."""
    return sorted({0, 1, 2, max(W - 1, 0), W, W + 1, 2 * W + 3}) + ([1307] if W == 600 else [])
