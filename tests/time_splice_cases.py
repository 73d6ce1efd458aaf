"""The time-splice layer, kind 9, restated in numpy for the tests; not collected by pytest.
  * the layer in its shrinking form: rows [T][D] -> [T - lo - hi][n D]
  * loglik_time: the expected log-likelihoods of a network with such layers under the edge rule -- the normalised
    features extended by Lh / Rh copies of the first / last frame, the first layer's splice over the extended rows, every
    layer through layer_cases.propagate's rules with the time-splice shrinking the row set, and layer_cases.loglik's tail
    on the T rows that are left
  * the WRONG rule (every hidden splice clamped at the utterance's own edge), which the GPU tests must be able to tell
    from the right one
  * the stack of the GPU tests
  * the models, batches and layout arithmetic of the tests at the limits, the pass edges and behind audio."""
import os

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


def feats_of(lengths, seed=0, dim=FEAT_DIM):
    return [(np.random.default_rng([0x7FEA, seed, u, T]).standard_normal((T, dim)) * 1.5).astype(F32) for u, T in enumerate(lengths)]


def stack_feats():
    return feats_of(LENGTHS)


# ================================================================ the limits, the pass edges and the audio path
# (tests/test_gpu_time_splice_limits.py on the GPU; tests/test_time_splice_host.py checks on the CPU that these cases can
# tell the right rule from the wrong one, that the finite ones are finite and that only the designed rows are NaN)

def same_rows(a, b):
    """Per row: equal bit for bit, NaN for NaN."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape
    an, bn = np.isnan(a), np.isnan(b)
    return ((an == bn) & (an | (a.view(np.uint32) == b.view(np.uint32)))).all(axis=1)


def nan_rows_allowed(layers, feats, left, right):
    """The output rows a non-finite input frame can reach: the frames' marks carried through the edge rule, the first
    layer's splice and every time-splice (all other layers work row by row) -> bool [T]."""
    Lh, Rh = time_context(layers)
    bad = ~np.isfinite(np.ascontiguousarray(feats, F32)).all(axis=1)
    bad = np.concatenate([np.repeat(bad[:1], left + Lh), bad, np.repeat(bad[-1:], right + Rh)])
    rows = bad.shape[0] - left - right
    bad = np.array([bad[r:r + left + right + 1].any() for r in range(rows)])
    for l in layers:
        if l[0] == "splice":
            lo, hi = lo_hi(l[1])
            rows = bad.shape[0] - lo - hi
            bad = np.array([any(bad[r + lo + o] for o in l[1]) for r in range(rows)])
    assert bad.shape[0] == feats.shape[0]
    return bad


# ---------------------------------------------------------------- 1. the kind alone, at its limits

def identity(D):
    return ("linear", np.eye(D, dtype=F32), np.zeros(D, F32))


def alone_layers(D, offsets, seed):
    """An identity Linear of width D, the splice, a seeded Linear n D -> 5 (left 0 / right 0, prior of ones).  With the
    identity in front and no first-layer context the activations at the virtual frames ARE the edge frame's: this form
    checks the copy and its index arithmetic, and the right and the wrong edge rule give the same rows on it."""
    rng = np.random.default_rng([0xA10E, D, seed])
    n = len(offsets) * D
    return [identity(D), ("splice", offsets), ("linear", (rng.standard_normal((5, n)) / np.sqrt(n)).astype(F32), (rng.standard_normal(5) * 0.1).astype(F32))]


SIXTEEN = list(range(-32, 0, 4)) + list(range(1, 32, 4))       # -32, -28, ..., -4 (0 mod 4) and 1, 5, ..., 29 (1 mod 4)
# (name, D, offsets): |o| = 32; 16 offsets; n D = 528, two k-chunks of the GEMM behind the splice; n D = 512 exactly
LIMIT_CASES = [("o32", 17, [-32, 32]), ("n16_D7", 7, SIXTEEN), ("n16_D33", 33, SIXTEEN), ("n16_D32", 32, SIXTEEN)]
LIMIT_T = (1, 2, 33, 64, 65, 131)                              # 1 and 2: every row is made of edge frames
LIMIT_SEED = 7


def limit_input(D, T):
    return LC.designed(T, D, LIMIT_SEED)


DEEP_LENGTHS = [1, 1, 130, 2, 1]
DEEP_CONTEXT = (64, 64)


def deep():
    """feat_dim 6, left 2 / right 1, four splices [-16, 16]: the context is (64, 64), the 128 the model accepts.
    -> (layers, prior)"""
    rng = np.random.default_rng(0xDEE9)
    s = ("splice", [-16, 16])
    layers = [LC._linear(rng, 24, 12), s, LC._linear(rng, 24, 10), ("relu",), s, LC._linear(rng, 20, 8), ("tanh",), s, LC._linear(rng, 16, 8), s,
              LC._linear(rng, 16, PDFS), ("softmax",)]
    return layers, rng.uniform(0.05, 0.3, PDFS).astype(F32)


def deep_feats():
    return feats_of(DEEP_LENGTHS, seed=21)


# ---------------------------------------------------------------- 2. a multisplice shape, shrunk

MS_FEAT_DIM, MS_LEFT, MS_RIGHT, MS_PDFS, MS_LH, MS_RH = 13, 2, 2, 11, 11, 8
MS_LENGTHS = [1, 7, 0, 19, 20, 140]
MS_POISON_LENGTHS = [150, 30, 9, 64, 1, 21, 141, 5]


def multisplice():
    """feat_dim 13, left 2 / right 2: Linear 65->520, p-norm ->260, Normalize, splice [-1, 2], Linear 520->300, p-norm
    ->150, Normalize, splice [-3, 4], Linear 300->96, p-norm ->48, Normalize, splice [-7, 2], Linear 96->24, tanh, Linear
    24->11, Softmax.  Lh = 11, Rh = 8: neither is a multiple of four, and the first spliced panel (520 rows) is read by the
    second k-chunk of the GEMM behind it.  -> (layers, prior)"""
    rng = np.random.default_rng(0x3517)
    layers = [LC._linear(rng, 65, 520), ("pnorm", 260), ("normalize",), ("splice", [-1, 2]),
              LC._linear(rng, 520, 300), ("pnorm", 150), ("normalize",), ("splice", [-3, 4]),
              LC._linear(rng, 300, 96), ("pnorm", 48), ("normalize",), ("splice", [-7, 2]),
              LC._linear(rng, 96, 24), ("tanh",), LC._linear(rng, 24, MS_PDFS), ("softmax",)]
    return layers, rng.uniform(0.05, 0.3, MS_PDFS).astype(F32)


def ms_feats(lengths=MS_LENGTHS, seed=31):
    return feats_of(lengths, seed, MS_FEAT_DIM)


# ---------------------------------------------------------------- 3. the pass boundary and the end of the batch
# The documented layout: row = column of Yt, every utterance with frames takes T + pad columns,
# pad = left + right + Lh + Rh.  In ROWS utterance u holds Lh virtual frames at pad_base[u], its T frames, Rh virtual frames
# and left + right rows of no frame; in COLUMNS left + Lh copies of the first frame, the T frames, right + Rh copies of the
# last.  PK_MI355_CHUNK=128 gives passes of 256 rows; a pass runs from HaloLeft = RoundUp(Lh, 4) rows in front of the rows
# it owns, in tiles of 128 rows.

PASS_ROWS, TILE = 256, 128
SWEEP_REST = [40, 300]


def pad_bases(lengths, pad):
    out, col = [], 0
    for T in lengths:
        out.append(col)
        col += T + pad if T else 0
    return out


def place(lengths, left, right, Lh, Rh, at):
    """What lies at position `at` -> (utterance, what it is as a row, what it is as a column)."""
    pad = left + right + Lh + Rh
    for u, (base, T) in enumerate(zip(pad_bases(lengths, pad), lengths)):
        i = at - base
        if T and 0 <= i < T + pad:
            row = "left virtual" if i < Lh else "frame" if i < Lh + T else "right virtual" if i < Lh + T + Rh else "no frame"
            col = "left copy" if i < left + Lh else "frame" if i < left + Lh + T else "right copy"
            return u, row, col
    return None, None, None


def sweep_lengths(left, right, Lh, Rh, margin=3):
    """The T0 of a batch [T0] + SWEEP_REST for which position PASS_ROWS lies anywhere from `margin` before utterance 0's
    last frame to `margin` behind utterance 1's first, as a row (frame t at pad_base + Lh + t) or as a column (at
    pad_base + left + Lh + t)."""
    pad = left + right + Lh + Rh
    first = PASS_ROWS - margin - (pad + left + Lh)          # utterance 1's frame 0 as a column: T0 + pad + left + Lh
    last = PASS_ROWS + margin - (Lh - 1)                    # utterance 0's last frame as a row: Lh + T0 - 1
    return list(range(first, last + 1))


def sweep_first(T0):
    """Utterance 0 of the sweep at T0 frames: the first T0 of one fixed run of frames."""
    return ms_feats([PASS_ROWS], seed=34)[0][:T0]


def end_batches(left, right, Lh, Rh):
    """[30, T]: the last frame of the last utterance (row 30 + pad + Lh + T - 1) on the last and on the first row of a tile,
    counted from row 0 (what a walk of one pass runs) and counted from the last pass's first row, PASS_ROWS - HaloLeft
    (what the last of several passes runs).  On a last row the Rh virtual frames lie in a tile of their own."""
    base = 30 + left + right + Lh + Rh + Lh
    origin = PASS_ROWS - (Lh + 3) // 4 * 4
    t_abs = 3 * TILE - base
    t_pass = origin + TILE - base
    assert base + t_pass > PASS_ROWS
    return {"last_row_of_a_tile": [30, t_abs], "first_row_of_a_tile": [30, t_abs + 1],
            "last_row_of_a_tile_of_the_pass": [30, t_pass], "first_row_of_a_tile_of_the_pass": [30, t_pass + 1]}


# ---------------------------------------------------------------- 4. behind the fused CMVN writer and behind audio

AUDIO_LEFT, AUDIO_RIGHT, AUDIO_PDFS, AUDIO_CONTEXT = 2, 1, 9, (7, 9)
RAW_LENGTHS = [1, 2, 63, 64, 65, 0, 601, 664]     # both pads from one tile of 64 frames; the last tile ragged and full; the window slides
RAW_POISON_LENGTHS = [700, 5, 800, 66, 130, 64, 70, 2, 9]


def audio_model():
    """feat_dim 40, left 2 / right 1: Linear 160->24, splice [-5, 0, 3], Linear 72->16, ReLU, splice [-2, 6], Linear 32->9,
    Softmax.  Lh = 7, Rh = 9.  -> (layers, prior)"""
    rng = np.random.default_rng(0xAD10)
    layers = [LC._linear(rng, 160, 24), ("splice", [-5, 0, 3]), LC._linear(rng, 72, 16), ("relu",), ("splice", [-2, 6]),
              LC._linear(rng, 32, AUDIO_PDFS), ("softmax",)]
    return layers, rng.uniform(0.05, 0.3, AUDIO_PDFS).astype(F32)


def raw_rows(lengths, seed, dim=40):
    """Rows like log-mel energies: 3 N(0, 1) + 12."""
    return [(np.random.default_rng([0x4A77, seed, u, T]).standard_normal((T, dim)) * 3.0 + 12.0).astype(F32) for u, T in enumerate(lengths)]


def stats_of(rows):
    """Global statistics of count 2500 with the rows' own means (far-off means would leave an utterance's first frames
    unnormalised, and the reference softmax overflows on them)."""
    mean = np.concatenate([r for r in rows if r.shape[0]]).astype(np.float64).mean(axis=0)
    return np.concatenate([mean * 2500.0, [2500.0]]).astype(F32)


def raw_front():
    """-> (statistics, the raw rows, oracle.cmvn of each)"""
    raw = raw_rows(RAW_LENGTHS, 41)
    g = stats_of(raw)
    return g, raw, [O.cmvn(g, r) if r.shape[0] else r for r in raw]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_WAVES = ("en-us-hello.wav", "en-us-cat.wav")


def golden_waves():
    """-> (the statistics of the golden model, the two waves, the oracle's fbank + CMVN of each)"""
    stats = O.read_vec(os.path.join(GOLDEN, "cmvn_stats.bin"))
    waves = [O.wav_read(os.path.join(GOLDEN, name)) for name in GOLDEN_WAVES]
    return stats, waves, [O.cmvn(stats, O.Fbank().compute(w)) for w in waves]


NARROW_PDFS, NARROW_CONTEXT = 7, (3, 4)


def narrow(D):
    """A time-splice model at any feature dimension, left 2 / right 1: Linear 4 D->20, splice [-2, 1], Linear 40->12, tanh,
    splice [-1, 3], Linear 24->7, Softmax.  Lh = 3, Rh = 4.  -> (layers, prior)"""
    rng = np.random.default_rng([0x4A80, D])
    layers = [LC._linear(rng, 4 * D, 20), ("splice", [-2, 1]), LC._linear(rng, 40, 12), ("tanh",), ("splice", [-1, 3]),
              LC._linear(rng, 24, NARROW_PDFS), ("softmax",)]
    return layers, rng.uniform(0.05, 0.3, NARROW_PDFS).astype(F32)


PRODUCERS = ("norm", "deltas", "lda", "frontend")
PRODUCER_LENGTHS = [1, 9, 0, 70]


def producer_case(name):
    """One case per remaining producer of the layout's input, the front half of the expectation from the case module the
    suite has for it -> dict: dim (the model's feature dimension), input (rows [T][13], or waves), front (the normalised
    features the layer stack must see), and what the scorer is made with."""
    import cmvn_any_cases as CA
    import delta_cases as DC
    import frontend_any_cases as FA
    import norm_cases as NC
    import transform_cases as XC
    rows = [NC.features(T, 13, 50 + u) for u, T in enumerate(PRODUCER_LENGTHS)]
    utt = [NC.normalize(x, "utterance", True, True)[0] for x in rows]
    if name == "norm":                      # utterance CMVN with variance
        return {"dim": 13, "input": rows, "front": utt}
    if name == "deltas":                    # ... and add-deltas (2, 2) behind it: 39
        return {"dim": 39, "input": rows, "front": [DC.add_deltas(x, 2, 2) for x in utt]}
    if name == "lda":                       # splice 3 / 3 + an affine 40 x 92 matrix on N(0, 1) rows, no normalisation
        m = XC.matrix(13, 3, 3, 40, True)
        rows = [XC.normal(T, 13, 50 + u) for u, T in enumerate(PRODUCER_LENGTHS)]
        return {"dim": 40, "input": rows, "front": [XC.transform(x, m, 3, 3) for x in rows], "matrix": m}
    if name == "frontend":                  # MFCC, 13 of 23 bins, and the sliding CMVN at 13 dimensions
        import pocketkaldi_amd as pk
        spec = FA.BATCH_SPECS[13]
        waves = [FA.wave_i16(n, 60 + u) for u, n in enumerate((1237, 399, 4321, 9000))]
        tables = pk.frontend_tables(spec)
        mfcc = [FA.frontend_any(w, spec, tables) for w in waves]
        g = stats_of(mfcc)
        return {"dim": 13, "input": waves, "front": [CA.cmvn_any(g, r) if r.shape[0] else r for r in mfcc], "spec": spec, "stats": g}
    raise KeyError(name)


def limit_batches():
    """Every batch of the GPU tests of the limits -> (name, layers, prior, left, right, features, designed): what the
    host test checks (designed: LC.designed inputs, whose non-finite rows are part of the case)."""
    for name, D, offsets in LIMIT_CASES:
        layers = alone_layers(D, offsets, 1)
        yield "alone " + name, layers, np.ones(5, F32), 0, 0, [limit_input(D, T) for T in LIMIT_T], True
    layers, prior = deep()
    yield "deep", layers, prior, LEFT, RIGHT, deep_feats(), False
    layers, prior = multisplice()
    yield "multisplice", layers, prior, MS_LEFT, MS_RIGHT, ms_feats(), False
    rest = ms_feats(SWEEP_REST, seed=33)
    yield "sweep rest", layers, prior, MS_LEFT, MS_RIGHT, rest, False
    yield "sweep", layers, prior, MS_LEFT, MS_RIGHT, [sweep_first(T0) for T0 in sweep_lengths(MS_LEFT, MS_RIGHT, MS_LH, MS_RH)], False
    for name, lengths in end_batches(MS_LEFT, MS_RIGHT, MS_LH, MS_RH).items():
        yield "end " + name, layers, prior, MS_LEFT, MS_RIGHT, ms_feats(lengths, seed=35), False
    layers, prior = audio_model()
    yield "raw rows", layers, prior, AUDIO_LEFT, AUDIO_RIGHT, raw_front()[2], False
    yield "golden waves", layers, prior, AUDIO_LEFT, AUDIO_RIGHT, golden_waves()[2], False
    for name in PRODUCERS:
        case = producer_case(name)
        layers, prior = narrow(case["dim"])
        yield "producer " + name, layers, prior, 2, 1, case["front"], False
