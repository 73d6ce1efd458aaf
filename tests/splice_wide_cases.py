"""Wide spliced first layers: the case tables of test_gpu_splice_wide.py and the builders of
their nets and features.

The first affine layer reads the spliced operand without materialising it: operand row k is feature k % D of the
frame k / D places into the context window (am.cc:65-88).  With K = D (L + R + 1) above 512 the fp32 kernel restarts
its accumulator at every 512-chunk and adds the chunks in order (gemm.cc:95-123), K is padded to the k-slab (16 rows
in fp32, 32 k's in the fp16 modes) and the padding rows must read zeros, never the frame behind the context.  Every
case names the route it is there for and states the numbers that put it there; test_splice_wide_cases.py recomputes
them from the rules below (restated from gemm.hip LaunchGemm / LaunchGeo, capi_exec.hip RunLayers, capi_batch.hip
SetLayoutFrames), so that an edit to a width cannot quietly move a case onto another route.

Every builder is seeded with np.random.default_rng([tag, D, L, R, ...]): a case's inputs depend on nothing but its
own numbers."""
import numpy as np

CHUNK = 512                 # gemm.h:50 KC; gemm.hip kChunkK
SLAB_F32, SLAB_F16 = 16, 32  # kBK, kBKF16: K is padded to these
TILE = 128                  # kTile: rows and output columns are padded to it
BIG_TILES = 384             # LaunchGemm: fewer 128 x 128 tiles than this run the 64 x 64-tile kernel
PASS_ROWS = 4096            # pk_score.h kSingleChunk: rows per pass of pk_decodable_init
SCALE = 0.1

N_PDFS = 60
SMALL_H, SMALL_T = 200, (1, 5, 130, 500)
BIG_H, BIG_T = 1536, 4100
# first-layer launches of those frame counts: (rows of the pass, tiles = Npad / 128 * rows_pad / 128)
SMALL_PASSES = {1: [(1, 2)], 5: [(5, 2)], 130: [(130, 4)], 500: [(500, 8)]}
BIG_PASSES = [(4096, 384), (4, 12)]

# a batch scorer's pass holds all of its rows: utterances of these lengths, each padded to four rows (compact rows),
# make 4 244 rows = 34 row tiles x 12 = 408 tiles, and every utterance behind the first has a non-zero column shift
SCORER_FRAMES = (4093, 0, 1, 3, 130, 7)
SCORER_COMPACT_ROWS = 4244
SCORER_TILES = 408
SCORER_PADDED_LAYOUT = ((80, 5, 5), (43, 6, 5), (57, 4, 4))      # also under PK_MI355_COMPACT_ROWS=0
SCORER_STABLE = (80, 5, 5)                                        # also with the default (stable) softmax

# (D, L, R): K, Kpad, chunks of 512, padding rows, big-tile passes too, what it is there for
F32_CASES = [
    dict(D=128, L=1, R=2, K=512, Kpad=512, chunks=1, pad=0, big=True,
         why="exactly one chunk: the boundary on the single-chunk side"),
    dict(D=57, L=4, R=4, K=513, Kpad=528, chunks=2, pad=15, big=True,
         why="K odd: one two-row piece holds a real row and a zero row; 15 padding rows"),
    dict(D=43, L=6, R=5, K=516, Kpad=528, chunks=2, pad=12, big=True,
         why="odd D; the second chunk is one slab; 12 padding rows: skip_last_half together with MULTICHUNK"),
    dict(D=65, L=4, R=3, K=520, Kpad=528, chunks=2, pad=8, big=True,
         why="exactly 8 padding rows: the skip_last_half threshold"),
    dict(D=79, L=3, R=3, K=553, Kpad=560, chunks=2, pad=7, big=True,
         why="7 padding rows: just under the skip_last_half threshold"),
    dict(D=64, L=4, R=4, K=576, Kpad=576, chunks=2, pad=0, big=True,
         why="no padding; D a multiple of the slab"),
    dict(D=80, L=5, R=5, K=880, Kpad=880, chunks=2, pad=0, big=True,
         why="the common 80-bin model; two chunks"),
    dict(D=130, L=5, R=5, K=1430, Kpad=1440, chunks=3, pad=10, big=True,
         why="three chunks, the last one partial"),
    dict(D=130, L=70, R=3, K=9620, Kpad=9632, chunks=19, pad=12, big=False,
         why="19 chunks; T = 1, 5 and 130 are shorter than or near the context"),
]

# A padding row that read the frame behind the context instead of zeros would go unnoticed on finite features (its
# weight is zero): these frames hold a NaN in feature 0 or feature pad - 1, the features the first and the last padding
# row would fetch.  Frame t belongs to the context of rows t - R .. t + L and no others; the row a wrong fetch would
# spoil is t - R - 1.  (130 frames: small tiles; 4 100: big tiles, NaN frames at both ends of the 4 096-row pass.)
NAN_FRAMES = {130: (3, 64, 129), 4100: (7, 2000, 4094, 4098)}

# big tiles, K <= 512: PK_MI355_L1_RING selects the two-slab (default) or the three-slab ring
RING_VALUES = ("3", "2")
RING_CASES = [
    dict(D=40, L=5, R=5, K=440, Kpad=448, chunks=1, pad=8, why="the 40-bin model: K = 440, skip_last_half"),
    dict(D=31, L=1, R=1, K=93, Kpad=96, chunks=1, pad=3, why="K = 93, odd: D and K multiples of nothing"),
]

# f16x3: the first layer reads the overlapping-row view of the split copy (row stride 2 D halves), K padded to 32
F16_SMALL_H, F16_SMALL_FRAMES = 300, (1, 257, 700)
F16_BIG_H, F16_BIG_FRAMES = 1536, (4500,)
F16_CASES = [
    dict(D=88, L=1, R=1, K=264, Kpad=288, pad=24, why="24 k's read past the context: the largest overhang"),
    dict(D=80, L=5, R=5, K=880, Kpad=896, pad=16, why="the common 80-bin model"),
    dict(D=128, L=2, R=2, K=640, Kpad=640, pad=0, why="no overhang"),
    dict(D=136, L=5, R=5, K=1496, Kpad=1504, pad=8, why="the widest"),
]
F16_OVERHANG = (88, 1, 1)       # this one's scorer first scores loud features of the same layout
LOUD_SIGMA = 1.0e4

# the seeded fuzz of test_gpu_splice_wide.py
FUZZ_D = (49, 160)
FUZZ_CONTEXT = (0, 7)
FUZZ_H = (137, 1536)
FUZZ_T = {137: (1, 64, 500), 1536: (2, 131, 4096, 4097)}
FUZZ_NORMALIZE_P = 0.25


def name(c):
    return "%d-%d-%d" % (c["D"], c["L"], c["R"])


def by_shape(cases, shape):
    return next(c for c in cases if (c["D"], c["L"], c["R"]) == tuple(shape))


# ------------------------------------------------------------------ the rules, restated

def round_up(x, m):
    return -(-x // m) * m


def derived(D, L, R, slab=SLAB_F32):
    """{"K", "Kpad", "chunks", "pad"} of a first layer."""
    K = D * (L + R + 1)
    Kpad = round_up(K, slab)
    return {"K": K, "Kpad": Kpad, "chunks": -(-Kpad // CHUNK), "pad": Kpad - K}


def skip_last_half(c):
    """gemm.hip: the last slab's second half is nothing but padding, its MFMAs are skipped."""
    return c["Kpad"] - c["K"] >= SLAB_F32 // 2


def decodable_passes(T, H):
    """[(rows, tiles)] of pk.Decodable's first-layer launches: passes of at most 4 096 rows."""
    return [(rows, round_up(H, TILE) // TILE * (round_up(rows, TILE) // TILE))
            for rows in (min(PASS_ROWS, T - r0) for r0 in range(0, T, PASS_ROWS))]


def scorer_rows(frames, L, R, compact=True):
    """Rows of a batch scorer's pass: compact, an utterance's rows start where the one before it ended, rounded up to
    four; otherwise row = column of the padded feature matrix (T + L + R columns an utterance).  An empty utterance
    takes neither.  The pass ends at the last frame of the last utterance that has one."""
    base = rows = 0
    for T in frames:
        if T == 0:
            continue
        rows = base + T
        base += round_up(T, 4) if compact else T + L + R
    return rows


def scorer_tiles(frames, L, R, H, compact=True):
    return round_up(H, TILE) // TILE * (round_up(scorer_rows(frames, L, R, compact), TILE) // TILE)


def variant(Kpad, tiles, ring=2):
    """(S, MULTICHUNK, R) of the spliced GemmKernel<S, true, MULTICHUNK, 1, R> a first-layer launch takes (LaunchGemm,
    LaunchGeo): big tiles from 384 tiles on, MULTICHUNK past one chunk, the two-slab ring for big tiles at K <= 512
    unless PK_MI355_L1_RING=3."""
    S = 2 if tiles >= BIG_TILES else 1
    multi = Kpad > CHUNK
    return (S, multi, 2 if S == 2 and not multi and ring == 2 else 3)


# ------------------------------------------------------------------ nets and features

def net(D, L, R, H, N=N_PDFS, normalize=False, tag=0x5A1C):
    """linear(H x K), relu, [normalize,] linear(N x H), softmax, and a prior."""
    rng = np.random.default_rng([tag, D, L, R, H, N])
    K = D * (L + R + 1)
    layers = [("linear", (rng.standard_normal((H, K)) * np.sqrt(2.0 / K)).astype(np.float32),
               (rng.standard_normal(H) * 0.1).astype(np.float32)), ("relu",)]
    if normalize:
        layers.append(("normalize",))
    layers += [("linear", (rng.standard_normal((N, H)) * np.sqrt(2.0 / H)).astype(np.float32),
                (rng.standard_normal(N) * 0.1).astype(np.float32)), ("softmax",)]
    prior = rng.uniform(0.5, 1.5, N)
    return layers, (prior / prior.sum()).astype(np.float32)


def features(D, L, R, T, seed=0, sigma=1.0):
    return (np.random.default_rng([0xFEA7, D, L, R, T, seed]).standard_normal((T, D)) * sigma).astype(np.float32)


def nan_features(c, T):
    """features(T) with a NaN in feature 0 / feature pad - 1 (alternating) of the frames NAN_FRAMES[T]."""
    f = features(c["D"], c["L"], c["R"], T, seed=9)
    for i, t in enumerate(NAN_FRAMES[T]):
        f[t, (0, c["pad"] - 1)[i % 2]] = np.nan
    return f


def nan_rows(c, T):
    """The rows whose context holds a NaN frame."""
    rows = np.zeros(T, bool)
    for t in NAN_FRAMES[T]:
        rows[max(0, t - c["R"]):t + c["L"] + 1] = True
    return rows


def same_bits_and_nans(a, b):
    """Equal bit for bit where both are numbers, NaN in the same places."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, a.view(np.uint32)), np.where(both, 0, b.view(np.uint32)))


def scorer_features(c, frames, sigma=1.0):
    """One matrix per utterance (seed = its position)."""
    return [features(c["D"], c["L"], c["R"], T, seed=1 + u, sigma=sigma) for u, T in enumerate(frames)]


def fuzz_case(seed):
    """(D, L, R, H, N, T, normalize) of fuzz seed `seed`: D in 49..160, L and R in 0..7 redrawn until K > 512."""
    rng = np.random.default_rng([0xF022, seed])
    D = int(rng.integers(FUZZ_D[0], FUZZ_D[1] + 1))
    while True:
        L, R = (int(v) for v in rng.integers(FUZZ_CONTEXT[0], FUZZ_CONTEXT[1] + 1, 2))
        if D * (L + R + 1) > CHUNK:
            break
    H = int(rng.choice(FUZZ_H))
    N = int(rng.integers(2, 200))
    T = int(rng.choice(FUZZ_T[H]))
    return D, L, R, H, N, T, bool(rng.random() < FUZZ_NORMALIZE_P)


# ------------------------------------------------------------------ float64 restatement (am.cc:65-112, nnet.cc)

def restated(layers, prior, L, R, feats, scale=SCALE):
    """AcousticModel::Compute in float64: splice with the edge frames replicated, the layers, floor 1e-20, log, minus
    the log prior, times the scale."""
    x = np.asarray(feats, np.float64)
    T = x.shape[0]
    x = np.concatenate([x[np.clip(np.arange(T) - L + c, 0, T - 1)] for c in range(L + R + 1)], axis=1)
    for l in layers:
        if l[0] == "linear":
            x = x @ l[1].astype(np.float64).T + l[2].astype(np.float64)
        elif l[0] == "relu":
            x = np.maximum(x, 0.0)
        elif l[0] == "normalize":
            x = x * np.sqrt(x.shape[1] / np.sum(x * x, axis=1, keepdims=True))
        else:
            e = np.exp(x)
            x = e / e.sum(axis=1, keepdims=True)
    return float(np.float32(scale)) * (np.log(np.maximum(x, 1e-20)) - np.log(prior.astype(np.float64)))


def first_difference(got, ref):
    """(row, column) of the first value whose bits differ, or None."""
    a = np.ascontiguousarray(got, np.float32).view(np.uint32)
    b = np.ascontiguousarray(ref, np.float32).view(np.uint32)
    if a.shape != b.shape:
        return ("shape", a.shape, b.shape)
    bad = np.argwhere(a != b)
    return None if bad.size == 0 else (int(bad[0][0]), int(bad[0][1]))
