"""Designed waves and layouts for the isolation and reuse properties of the scorers (include/pk_mi355.h, "Isolation
and reuse"): in an f32 call an utterance's (an online slot's) results are a function of that utterance's samples alone,
and a call's results are a function of that call's inputs alone, whatever the object did before.

The kernels read memory they do not own on the promise never to use it (whole 64-frame CMVN tiles behind an utterance,
24 frames in front of the first sliding tile, the next frame's samples, the padding rows of a four-row group and of the
last 128-row tile).  In a fresh object all of it is zero, and adding zero is harmless -- so the neighbours here are
poisoned: NaN surfaces any use, even under the 1e-4 contract of the stable tail; a loud finite wave complements it
(fmaxf, v_max_f32 and `<` drop NaN silently) and takes FbankKernel's ordered-sum path beside the exact tree sum of its
integer-valued neighbours.

What the reference does with a poisoned wave is exactly predictable (test_isolation_cases.py holds the oracle, and the
live reference where it is built, to it):
  * frame t of fbank reads samples [160 t, 160 t + 400): a frame holding a NaN or an Inf sample is NaN in all 40 bins
    (Inf: the DC mean is Inf, Inf - Inf = NaN, and the FFT spreads it);
  * online CMVN is a running sum: NaN from the first such frame to the END of the utterance, however few samples are bad;
  * log-likelihood row r splices frames r - L .. r + R: NaN from (first bad frame) - R to the end, and nowhere else.
test_gpu_isolation.py runs all of it on a GPU.
"""
import functools

import numpy as np

from pocketkaldi_amd import synth

KINDS = ("nan_all", "nan_from", "inf_one", "loud")
FRAME_LENGTH, FRAME_SHIFT = 400, 160
LOUD_SIGMA = 3e4


def samples_for(T):
    """Exactly T frames and no sample left over (T = 0: 240 samples, no frame)."""
    return FRAME_LENGTH + FRAME_SHIFT * (T - 1)


def frames_of(n):
    return 0 if n < FRAME_LENGTH else 1 + (n - FRAME_LENGTH) // FRAME_SHIFT


@functools.lru_cache(maxsize=None)
def _healthy(seed, T):
    n = samples_for(T)
    w = synth.utterance(seed, seconds=(n + 0.25) / synth.SAMPLE_RATE)[:n]
    assert w.shape == (n,) and np.all(w == np.round(w)) and np.abs(w).max() <= 32767
    w.setflags(write=False)
    return w


def healthy(seed, T):
    """synth.utterance cut to exactly T frames: integer-valued float samples (read-only; shared)."""
    return _healthy(int(seed), int(T))


def first_bad_frame(T):
    """Where the poison of nan_from / inf_one begins: mid-utterance, no multiple of 4 (nor of 64)."""
    f0 = T // 2
    if f0 % 4 == 0:
        f0 += 1
    assert 0 < f0 < T and f0 % 4 and f0 % 64, (T, f0)
    return f0


def bad_sample(T):
    """Sample 160 (f0 - 1) + 437: the last 123 samples of frame f0 and later -- frame f0 - 1 ends 37 samples before."""
    return FRAME_SHIFT * (first_bad_frame(T) - 1) + FRAME_LENGTH + 37


class Prediction:
    """Which frames / rows of a poisoned utterance are NaN (entirely: all 40 bins, all pdfs), per stage."""

    def __init__(self, T, fbank_frames, first):
        self.T, self.first = T, first
        self.fbank = np.zeros(T, bool)
        self.fbank[list(fbank_frames)] = True
        self.cmvn = np.arange(T) >= (T if first is None else first)
        assert first is None or (self.fbank[first] and not self.fbank[:first].any())

    def loglik(self, right):
        return np.arange(self.T) >= (self.T if self.first is None else max(self.first - right, 0))


@functools.lru_cache(maxsize=None)
def _poisoned(kind, seed, T):
    w = _healthy(seed, T).copy()
    n = w.shape[0]
    if kind == "nan_all":
        w[:] = np.nan
        pred = Prediction(T, range(T), 0 if T else None)
    elif kind == "nan_from":
        f0, s0 = first_bad_frame(T), bad_sample(T)
        w[s0:] = np.nan
        pred = Prediction(T, range(f0, T), f0)
    elif kind == "inf_one":
        f0, s0 = first_bad_frame(T), bad_sample(T)
        w[s0] = np.inf
        holding = [t for t in range(T) if FRAME_SHIFT * t <= s0 < FRAME_SHIFT * t + FRAME_LENGTH]
        assert holding[0] == f0
        pred = Prediction(T, holding, f0)
    elif kind == "loud":
        w = (np.random.default_rng([0x10DD, seed]).standard_normal(n) * LOUD_SIGMA).astype(np.float32)
        assert np.isfinite(w).all() and not np.all(w == np.round(w))
        pred = Prediction(T, [], None)
    else:
        raise KeyError(kind)
    w.setflags(write=False)
    return w, pred


def poisoned(kind, seed, T):
    """-> (wave, Prediction) (read-only; shared)."""
    return _poisoned(kind, int(seed), int(T))


# ------------------------------------------------------------------ batch layouts (frames, poisoned?)

# A, model "tiny", small-tile kernels: 37 frames leave three padding rows that read the poisoned neighbour's columns; the
# one-frame utterance sits between two poisoned ones with a frameless one beside it; 601 poisoned frames put a poisoned
# utterance's raw rows in front of the next utterance's CMVN tiles (and slide its own window by one frame).
LAYOUT_A = ((37, False), (130, True), (1, False), (0, False), (3, True), (66, False), (601, True), (200, False))
# B, model "S": 2 116 compact rows = 17 row tiles x 24 column tiles = 408 >= 384: the fused tail, with the strip launch
# (17 x 23 = 391); NaN rows and healthy rows share 128-row tiles, one workgroup's tail phase handles both.
LAYOUT_B = ((700, False), (333, True), (650, False), (5, True), (420, False))
# C, model "S": 6 292 compact rows (>= 6 144: big tiles in every layer); no length a multiple of four.
LAYOUT_C = ((901, False), (887, True), (893, False), (899, False), (905, True), (882, False), (910, False))
LAYOUTS = {"A": ("tiny", LAYOUT_A, 3000), "B": ("S", LAYOUT_B, 3100), "C": ("S", LAYOUT_C, 3200)}
ROTATIONS = range(len(KINDS))

assert sum(-(-T // 4) * 4 for T, _ in LAYOUT_B) == 2116 and -(-2116 // 128) * 24 >= 384 and -(-2116 // 128) * 23 >= 384
assert sum(-(-T // 4) * 4 for T, _ in LAYOUT_C) >= 6144 and all(T % 4 for T, _ in LAYOUT_C)


def compact_rows(layout):
    return sum(-(-T // 4) * 4 for T, _ in layout)


def layout_utterances(name, rotation):
    """The utterances of layout `name`: [{"wave", "T", "kind" (None: healthy), "pred", "seed"}].  The p-th poisoned
    utterance is of kind KINDS[(p + rotation) % 4]: over the four rotations every poisoned place sees every kind."""
    _, layout, seed0 = LAYOUTS[name]
    out, p = [], 0
    for u, (T, bad) in enumerate(layout):
        if bad:
            kind = KINDS[(p + rotation) % len(KINDS)]
            p += 1
            w, pred = poisoned(kind, seed0 + u, T)
        else:
            kind, w, pred = None, healthy(seed0 + u, T), Prediction(T, [], None)
        out.append({"wave": w, "T": T, "kind": kind, "pred": pred, "seed": seed0 + u})
    return out


# ------------------------------------------------------------------ batch reuse: one scorer, many layouts

REUSE_MAX_UTTS = 8
# the poison call: max_utts utterances and exactly max_total_samples samples; 640 frames slide the CMVN window, 1 520
# frames are six 256-row passes (PK_MI355_CHUNK=128 is rounded up to 256), three on each lane with PK_MI355_LANES=2
REUSE_POISON_FRAMES = (640, 150, 150, 97, 150, 33, 150, 150)
REUSE_CAP = sum(samples_for(T) for T in REUSE_POISON_FRAMES)
REUSE_LAYOUTS = (
    ("fewer_shorter", (90, 41, 200)),
    ("each_a_little_shorter", tuple(T - (1 + u % 3) for u, T in enumerate(REUSE_POISON_FRAMES))),   # pads land where features were
    ("frameless_between", (0, 77, 0, 130, 0, 0, 61, 0)),
    ("one_frame", (1,)),
    ("empty", ()),
    ("full", REUSE_POISON_FRAMES),              # straight after the empty batch: the poison call's leftovers are still there
)
assert all(len(f) <= REUSE_MAX_UTTS and sum(samples_for(T) for T in f) <= REUSE_CAP for _, f in REUSE_LAYOUTS)


def reuse_poison_waves(kind):
    return [poisoned(kind, 4000 + u, T)[0] for u, T in enumerate(REUSE_POISON_FRAMES)]


def reuse_poison_waves_i16():
    """What int16 ingestion can carry of `loud`: full-scale integer noise."""
    return [np.clip(np.round(poisoned("loud", 4000 + u, T)[0]), -32768, 32767).astype(np.int16)
            for u, T in enumerate(REUSE_POISON_FRAMES)]


def reuse_healthy_waves(index):
    return [healthy(4100 + 10 * index + u, T) for u, T in enumerate(REUSE_LAYOUTS[index][1])]


# ------------------------------------------------------------------ single-utterance workspace

SINGLE_POISON_T = 4500                          # two 4 096-row passes (pk_score.h: kSingleChunk)
SINGLE_T = (1, 127, 129, 4097)
SINGLE_STACKS = ("normalize", "no_softmax", "softmax")


@functools.lru_cache(maxsize=None)
def single_stack(name):
    """Small random stacks on 40 features, context 2 + 2 -> (layers, prior, L, R).  "normalize": a Normalize layer
    inside; "no_softmax": a ReLU net whose outputs go to the tail as they are (am.cc:109); "softmax": the plain one."""
    rng = np.random.default_rng([0x51C, SINGLE_STACKS.index(name)])
    L, R, D, H, N = 2, 2, 40, 96, 70
    K = D * (L + R + 1)

    def lin(n, k, bias=0.1):
        return ("linear", (rng.standard_normal((n, k)) * np.sqrt(2.0 / k)).astype(np.float32),
                (rng.standard_normal(n) * bias).astype(np.float32))

    if name == "normalize":
        layers = [lin(H, K), ("relu",), ("normalize",), lin(N, H), ("softmax",)]
    elif name == "no_softmax":
        last = lin(N, H)
        layers = [lin(H, K), ("relu",), ("linear", last[1], np.abs(last[2]) + np.float32(0.05)), ("relu",)]
    else:
        layers = [lin(H, K), ("relu",), lin(N, H), ("softmax",)]
    prior = rng.uniform(0.5, 1.5, N)
    return layers, (prior / prior.sum()).astype(np.float32), L, R


def single_features(T, seed=0):
    return np.random.default_rng([0xFEA7, seed, T]).standard_normal((T, 40)).astype(np.float32)


# ------------------------------------------------------------------ online scorer

ONLINE_SLOTS = 4
ONLINE_POISONED_SLOT = 1
ONLINE_T = {0: 203, 1: 310, 2: 187, 3: 241}     # frames per slot's wave
# samples per step: 5, 10, 7 and 3 new frames a step once the stream runs -- for the healthy slots no multiple of four
ONLINE_CHUNK = {0: 800, 1: 1600, 2: 1120, 3: 480}
ONLINE_REUSE_T = 705                            # >= 700: d_tails, d_sums, d_raw_hist (600 frames) and d_hist are all written
ONLINE_BIG_STEP = (50, 625)                     # frames of history, then more than 600 new frames in ONE step
ONLINE_LONG_T = 1307                            # > 1 200: the 600-frame ring wraps twice


def online_neighbour_waves(kind):
    """-> ([wave per slot], Prediction of the poisoned slot)."""
    waves = [healthy(5000 + s, ONLINE_T[s]) for s in range(ONLINE_SLOTS)]
    waves[ONLINE_POISONED_SLOT], pred = poisoned(kind, 5000 + ONLINE_POISONED_SLOT, ONLINE_T[ONLINE_POISONED_SLOT])
    return waves, pred


def online_reuse_waves():
    return poisoned("nan_all", 5100, ONLINE_REUSE_T)[0], healthy(5101, ONLINE_REUSE_T + 9)


def online_big_step_wave():
    return healthy(5200, sum(ONLINE_BIG_STEP) + 31)


def online_long_wave():
    return healthy(5300, ONLINE_LONG_T)


# ------------------------------------------------------------------ every designed poisoned wave, for the CPU checks

def designed_waves():
    """[(name, kind, wave, Prediction)]: every poisoned wave the GPU tests use, once."""
    out, seen = [], set()
    for name in LAYOUTS:
        for rot in ROTATIONS:
            for u, e in enumerate(layout_utterances(name, rot)):
                if e["kind"] and (e["kind"], e["seed"], e["T"]) not in seen:
                    seen.add((e["kind"], e["seed"], e["T"]))
                    out.append(("%s[%d] %s" % (name, u, e["kind"]), e["kind"], e["wave"], e["pred"]))
    for kind in ("nan_all", "loud"):
        for u, T in enumerate(REUSE_POISON_FRAMES):
            out.append(("reuse[%d] %s" % (u, kind), kind) + poisoned(kind, 4000 + u, T))
    for kind in ("nan_from", "loud"):
        waves, pred = online_neighbour_waves(kind)
        out.append(("online slot %s" % kind, kind, waves[ONLINE_POISONED_SLOT], pred))
    out.append(("online reuse nan_all", "nan_all") + poisoned("nan_all", 5100, ONLINE_REUSE_T))
    return out


# ------------------------------------------------------------------ comparisons (CPU and GPU tests alike)

def same_bits(a, b):
    """Bit for bit, NaN where the other has NaN (whatever its payload)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    both = np.isnan(a) & np.isnan(b)
    return np.array_equal(np.where(both, 0, a.view(np.uint32)), np.where(both, 0, b.view(np.uint32)))


def nan_rows(a, what=""):
    """bool[T]: the rows of a that are NaN -- a row is NaN in every column or in none."""
    a = np.asarray(a)
    if a.size == 0:
        return np.zeros(a.shape[0], bool)
    n = np.isnan(a).reshape(a.shape[0], -1)
    full, some = n.all(axis=1), n.any(axis=1)
    assert np.array_equal(full, some), "%s: rows %s are NaN in some columns only" % (what, np.flatnonzero(full != some)[:8].tolist())
    return some


def assert_nan_rows(a, want, what):
    got = nan_rows(a, what)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d rows differ from the predicted NaN rows, first %s (NaN there: %s)" % (
        what, bad.size, bad[:8].tolist(), got[bad[:8]].tolist())
