"""Batches past the launch caps, for the tests; not collected by pytest.

Every per-utterance, per-slot, per-row and per-item kernel is launched on a capped grid and walks what lies past the cap in
a stride loop (or, the resampler and the audio front-end, in a second launch).  The cases here are the smallest batches in
which each of those walks takes a second turn: cap + 2 units of almost nothing.

  * The caps, as constants, and where the launchers' sources state them (SOURCE_PINS).
  * Pools.  Unit u has the content of pool[u % 7] -- features or samples, and length -- and, where a kernel indexes a
    parameter by the unit (a speaker record, a per-utterance matrix), the parameter params[u % 11].  No cap and no cap + 1
    is a multiple of 7 or 11, so unit u and unit u +- cap never share a content or a parameter, and the expectation is
    computed once per (content, parameter) pair -- 77 at most -- and assembled into one [sum T][N] array by index.  The
    rows of the row walk have the content of rows_pool[r % 1021].
  * The expectation of a pair: the stage under test through the existing restatements (norm_cases, online_cmvn_cases,
    cmvn_any_cases, delta_cases, transform_cases, resample_model, frontend_any_cases, the oracle's fbank and CMVN), then
    the model through layer_cases.loglik (oracle affine layers, softmax mode "reference"): bit for bit what the scorers
    give.
  * What three wrong kernels would give (Case.variant): "unprocessed" -- units at or past the cap never computed, the
    model reads a zeroed buffer (the in-place layer kinds: the pre-activation values); "wrapped" -- unit u >= cap computed
    from the content and the parameter of unit u - cap; "twice" (the row walk only) -- rows at or past the cap activated
    twice.
  * The device memory of each case, by the create path's formulas."""
import numpy as np

import pocketkaldi_amd as pk
from oracle import oracle as O

import cmvn_any_cases as CA
import delta_cases as DC
import frontend_any_cases as FA
import layer_cases as LC
import norm_cases as NC
import online_cmvn_cases as OC
import resample_model as RM
import transform_cases as TC

F32 = np.float32

UTT_CAP = 65535                     # utterances, slots or records on grid.y / grid.z of one launch
LAYER_LINES_CAP = 32768 * 4         # lines of a layer kind's launch: kMaxGridY workgroups of kLayerThreads / 64 lines
RESAMPLE_ITEMS_CAP = 32768          # items of one ResampleKernel launch

N_UTTS = UTT_CAP + 2
POOL, PARAMS, ROWS_POOL = 7, 11, 1021
D, N, SCALE = 3, 4, 0.1
LEFT, RIGHT = 2, 1
LENGTHS = (3, 0, 5, 1, 2, 4, 2)     # frames of pool[i]: below, at and above LEFT + RIGHT; unit UTT_CAP is pool[1], the empty one
CHUNK = 262144                      # rows of a pass (PublicChunkCap)

# (file under pocketkaldi_amd/csrc, the text that states the cap there, how often it stands in the file)
SOURCE_PINS = (
    ("layers.hip", "constexpr int kLayerThreads = %d;" % (LAYER_LINES_CAP // 32768 * 64), 1),
    ("layers.hip", "constexpr int kMaxGridY = %d;" % (LAYER_LINES_CAP // 4), 1),
    ("layers.hip", "lines < kMaxGridY ? lines : kMaxGridY", 2),
    ("layers.hip", "o += gridDim.y * kLayerWaves", 2),
    ("features.hip", "num_utts < %d ? num_utts : %d" % (UTT_CAP, UTT_CAP), 2),
    ("features.hip", "u += gridDim.y", 2),
    ("norm.hip", "num_utts < %d ? num_utts : %d" % (UTT_CAP, UTT_CAP), 2),
    ("norm.hip", "u += gridDim.y", 2),
    ("delta.hip", "num_utts < %d ? num_utts : %d" % (UTT_CAP, UTT_CAP), 1),
    ("delta.hip", "n < %d ? n : %d" % (UTT_CAP, UTT_CAP), 1),
    ("delta.hip", "+= gridDim.z", 2),
    ("transform.hip", "num_utts < %d ? num_utts : %d" % (UTT_CAP, UTT_CAP), 1),
    ("transform.hip", "n < %d ? n : %d" % (UTT_CAP, UTT_CAP), 1),
    ("transform.hip", "+= gridDim.z", 2),
    ("stream.hip", "n < %d ? n : %d" % (UTT_CAP, UTT_CAP), 1),
    ("stream.hip", "k += gridDim.y", 1),
    ("capi_resample.hip", "constexpr int kMaxGridY = %d;" % RESAMPLE_ITEMS_CAP, 1),
    ("capi_resample.hip", "d_items + at", 1),
    ("frontend.hip", "constexpr int kMaxFbankGridY = %d;" % UTT_CAP, 1),
    ("frontend.hip", "at += kMaxFbankGridY", 2),
)

# the lines of the create path that core_bytes restates (it leaves out a time-splice model's halo, which no case has)
FORMULA_PINS = (
    ("capi_batch.hip", "c->max_cols = RoundUp(max_rows + (int64_t)units * pad, kTileF16);", 1),
    ("capi_batch.hip", "c->ldy = RoundUp(c->max_cols, c->chunk) + 256 + c->zero_span;", 1),
    ("capi_batch.hip", "chk(hipMalloc(&c->d_ll, sizeof(float) * c->max_cols * am->num_pdfs));", 1),
    ("pk_score.h", "return RoundUp(units * pad + 2 * kTile, 256);", 1),
    ("capi_exec.hip", "e->act_floats = (int64_t)am->max_dim_pad * rows_cap;", 1),
    ("capi_exec.hip", "e->in_floats = RoundUp(am->input_dim, kBK) * rows_cap;", 1),
)


def model(feat_dim, left=LEFT, right=RIGHT):
    """Linear K -> 8, ReLU, Linear 8 -> N, Softmax -> (layers, prior)"""
    rng = np.random.default_rng([0x6A1D, feat_dim, left, right])
    layers = [LC._linear(rng, feat_dim * (left + right + 1), 8), ("relu",), LC._linear(rng, 8, N), ("softmax",)]
    return layers, rng.uniform(0.1, 0.4, N).astype(F32)


def features(T, dim, seed):
    """2 N(0, 1) + 1"""
    return (2.0 * np.random.default_rng([0x91D, seed, T, dim]).standard_normal((T, dim)) + 1.0).astype(F32)


def global_stats(dim):
    """Count 2500, every mean 1."""
    return np.concatenate([np.full(dim, 2500.0), [2500.0]]).astype(F32)


def same(got, want):
    return LC.same(got, want)


class Case:
    """One batch past a cap.  A subclass gives content(i), param(j) where it has one, and stage(x, p): the rows the model's
    first layer splices."""
    cap, n_units = UTT_CAP, N_UTTS
    content_period, param_period = POOL, 0
    feat_dim, left, right = D, LEFT, RIGHT          # the model's
    variants = ("unprocessed", "wrapped")

    def __init__(self):
        self.layers, self.prior = model(self.feat_dim, self.left, self.right)
        self._table = None

    # ---- what a subclass states
    def content(self, i):
        return features(LENGTHS[i], D, i)

    def param(self, j):
        return None

    def stage(self, x, p):
        raise NotImplementedError

    def frames(self, x):
        return x.shape[0]

    # ---- the expectation
    @property
    def num_pdfs(self):
        return len(self.prior)

    def tail(self, feats):
        return LC.loglik(self.layers, feats, self.prior, self.left, self.right, SCALE)

    def rows(self, x, p):
        if self.frames(x) == 0:
            return np.zeros((0, self.num_pdfs), F32)
        return self.tail(self.stage(x, p))

    def periods(self):
        return self.content_period, max(self.param_period, 1)

    def key(self, u):
        cp, pp = self.periods()
        return (u % cp) * pp + u % pp

    def table(self):
        """rows of every (content, parameter) pair, in key order: computed once, shared, left unchanged"""
        if self._table is None:
            cp, pp = self.periods()
            self._table = [self.rows(self.content(i), self.param(j) if self.param_period else None) for i in range(cp) for j in range(pp)]
        return self._table

    def unit_lengths(self):
        cp, pp = self.periods()
        per_key = np.array([t.shape[0] for t in self.table()], np.int64)
        u = np.arange(self.n_units)
        return per_key[(u % cp) * pp + u % pp]

    def expected(self):
        """-> ([sum T][N] rows of all units one after the other, the units' frame counts)"""
        cp, pp = self.periods()
        tab = self.table()
        per_key = np.array([t.shape[0] for t in tab], np.int64)
        start = np.concatenate([[0], np.cumsum(per_key)])[:-1]
        flat = np.concatenate(tab)
        u = np.arange(self.n_units)
        keys = (u % cp) * pp + u % pp
        T = per_key[keys]
        first = np.concatenate([[0], np.cumsum(T)])[:-1]
        idx = np.repeat(start[keys] - first, T) + np.arange(int(T.sum()))
        return flat[idx], T

    # ---- the wrong kernels
    def late_units(self):
        """(unit at or past the cap, the unit a dropped offset would compute it from)"""
        return [(u, u - self.cap) for u in range(self.cap, self.n_units)]

    def wrapped_content(self, u, src):
        cp, _ = self.periods()
        own = self.content(u % cp)
        return np.resize(self.content(src % cp), own.shape).astype(own.dtype)

    def variant(self, which):
        assert which in self.variants, which
        cp, pp = self.periods()
        rows, T = self.expected()
        rows = rows.copy()
        first = np.concatenate([[0], np.cumsum(T)])
        for u, src in self.late_units():
            x, p = self.content(u % cp), self.param(u % pp) if self.param_period else None
            if self.frames(x) == 0:
                continue
            if which == "unprocessed":
                alt = self.tail(np.zeros_like(self.stage(x, p)))
            else:
                alt = self.rows(self.wrapped_content(u, src), self.param(src % pp) if self.param_period else None)
            assert alt.shape[0] == T[u], (u, alt.shape, T[u])
            rows[first[u]:first[u + 1]] = alt
        return rows

    # ---- memory, by the create path's formulas (capi_batch.hip CreateScorerCore, capi_exec.hip AllocExec)
    def total_frames(self):
        return int(self.unit_lengths().sum())

    def extra_bytes(self):
        """the stage's own buffers beyond the scorer core"""
        return 0

    def device_bytes(self, live=False):
        return core_bytes(self.feat_dim, self.num_pdfs, [l[1].shape[0] for l in self.layers if l[0] == "linear"], self.left, self.right,
                          self.n_units, self.total_frames(), live) + self.extra_bytes()


def _round_up(x, m):
    return (x + m - 1) // m * m


def core_bytes(feat_dim, num_pdfs, widths, left, right, units, max_frames, live=False, extra_rows_per_unit=0):
    """Yt [feat_dim][ldy], the log-likelihood rows [max_cols][num_pdfs], the layer buffers of one pass (two activation
    buffers of the widest padded layer and the first layer's input), the layout block with its shift4 table; a live
    object's rows allow right + 3 (+ the stages' look-ahead) more per slot, and its history is 2 hist_len frames a slot."""
    pad = left + right
    max_rows = max_frames + (units * (right + 3 + extra_rows_per_unit) if live else 0)
    max_cols = _round_up(max_rows + units * pad, 256)
    chunk = min(CHUNK, max_cols)
    zero_span = _round_up(units * pad + 256, 256)
    ldy = _round_up(max_cols, chunk) + 256 + zero_span
    exec_floats = (2 * _round_up(max(widths + [num_pdfs]), 128) + _round_up(feat_dim * (pad + 1), 16)) * chunk
    layout = _round_up(28 * units, 256) * (2 if live else 1) + 4 * (max_cols // 4 + 256)
    hist = 4 * units * 2 * max(pad, 1) * feat_dim if live else 0
    return 4 * (ldy * feat_dim + max_cols * num_pdfs + exec_floats) + layout + hist


# ---------------------------------------------------------------- b. the utterance walk, features

class Layout(Case):
    """FeatureLayoutKernel: NORMALIZED features, compact rows, the shift4 table at the shifts of 65 537 utterances"""
    def stage(self, x, p):
        return x

    def extra_bytes(self):
        return 4 * self.total_frames() * D


class CmvnChain(Case):
    """CmvnChainKernel: RAW features under D + 1 global statistics"""
    stats = global_stats(D)

    def stage(self, x, p):
        return CA.cmvn_any(self.stats, x)

    def extra_bytes(self):
        return 2 * 4 * self.total_frames() * D


class NormUtterance(Case):
    """NormKernel, mode "utterance" with norm_vars; record(i): the statistics norm_stats gives for pool[i]"""
    def stage(self, x, p):
        return NC.normalize(x, "utterance", True, True)[0]

    def record(self, i):
        return NC.accumulate(self.content(i))

    def extra_bytes(self):
        return 2 * 4 * self.total_frames() * D + self.n_units * (8 * 2 * (D + 1) + 4 * 2 * D)


def speaker_record(j):
    """the statistics of 20 + j frames of their own"""
    return NC.accumulate(features(20 + j, D, 100 + j))


class NormSpeaker(NormUtterance):
    """NormKernel, mode "speaker": utterance u under record u % 11"""
    param_period = PARAMS

    def param(self, j):
        return speaker_record(j)

    def stage(self, x, p):
        return NC.normalize(x, "speaker", True, True, stats=p)[0]


class OnlineCmvn(NormUtterance):
    """OnlineCmvnKernel: a window of 4 frames (the longest utterances slide it), speaker records of period 11"""
    param_period = PARAMS
    spec = (4, 3, 2, True)                          # cmn_window, speaker_frames, global_frames, norm_vars
    glob = NC.accumulate(features(50, D, 99))

    def param(self, j):
        return speaker_record(j)

    def stage(self, x, p):
        W, sf, gf, nv = self.spec
        return OC.online_cmvn(x, W, sf, gf, nv, glob=self.glob, spk=p)[0]

    def extra_bytes(self):
        return 2 * 4 * self.total_frames() * D + self.n_units * 8 * 2 * (D + 1)


class Delta(Case):
    """DeltaKernel, order 2, window 2: the model reads 3 D features"""
    feat_dim, order, window = 3 * D, 2, 2

    def stage(self, x, p):
        return DC.add_deltas(x, self.order, self.window)

    def extra_bytes(self):
        return 4 * self.total_frames() * (D + 2 * self.feat_dim)


class TransformGlobal(Case):
    """TransformKernel with a global affine matrix at left_context = right_context = 1"""
    xl, xr = 1, 1
    matrix = TC.matrix(D, 1, 1, D, True, seed=21)

    def stage(self, x, p):
        return TC.transform(x, self.matrix, self.xl, self.xr)

    def extra_bytes(self):
        return 4 * self.total_frames() * 3 * D


def utt_matrix(j, dim=D):
    return TC.matrix(dim, 0, 0, dim, True, seed=40 + j)


class TransformUtt(Case):
    """TransformKernel with mat_stride != 0: utterance u through the affine matrix u % 11"""
    param_period = PARAMS

    def param(self, j):
        return utt_matrix(j)

    def stage(self, x, p):
        return TC.transform(x, p, 0, 0)

    def extra_bytes(self):
        return 4 * self.total_frames() * 3 * D + 4 * self.n_units * (D + 1) * 64          # d_umats: (D + 1) x Ldo(D) floats each


class Chained(TransformUtt):
    """utterance norm -> deltas -> global transform -> per-utterance matrices"""
    matrix = TC.matrix(3 * D, 1, 1, D, True, seed=22)

    def stage(self, x, p):
        y = NC.normalize(x, "utterance", True, True)[0]
        y = DC.add_deltas(y, 2, 2)
        y = TC.transform(y, self.matrix, 1, 1)
        return TC.transform(y, p, 0, 0)

    def extra_bytes(self):
        return 4 * self.total_frames() * (2 * D + 3 * D + 2 * D) + 4 * self.n_units * (D + 1) * 64 + self.n_units * (8 * 2 * (D + 1) + 4 * 2 * D)


LIVE_LENGTHS = (3, 1, 5, 1, 2, 4, 2)    # every slot pushes a frame at least: a step makes no record for a slot with nothing new


class Live:
    """The live objects' cases.  A step makes one record per slot that has something new, and the kernels see the records
    of the feature slots in REVERSE slot order (capi_stream.hip: rec_at = max_streams - 1 - n_back): with every slot
    taking part, record k is slot n_units - 1 - k.  So the records at and past the cap are the first slots, and record
    k - cap is slot u + cap -- the pools' periods divide no cap, on the record index as on the slot index."""
    def content(self, i):
        return features(LIVE_LENGTHS[i], D, i)

    def records(self, pushed):
        """records of a step: the slots that were pushed something in it, or still owe rows when they are closed"""
        return int((np.asarray(pushed) > 0).sum())

    def slot_of_record(self, k):
        return self.n_units - 1 - k

    def late_units(self):
        return [(self.slot_of_record(k), self.slot_of_record(k - self.cap)) for k in range(self.cap, self.n_units)]


class LiveLayout(Live, Layout):
    """StreamFeatureLayoutKernel: NORMALIZED slots"""


class LiveChain(Live, Case):
    """a live object made with deltas and a transform, RAW slots under norm "none": deltas -> global transform"""
    matrix = Chained.matrix

    def stage(self, x, p):
        return TC.transform(DC.add_deltas(x, 2, 2), self.matrix, 1, 1)

    def device_bytes(self, live=True):
        M, Rt = 4, 1
        core = core_bytes(self.feat_dim, self.num_pdfs, [8], self.left, self.right, self.n_units, self.total_frames(), True, M + Rt)
        rows = self.total_frames() + self.n_units * (M + Rt)
        rings = 4 * self.n_units * (2 * 2 * M * D + 2 * 2 * 3 * D)
        return core + 4 * rows * (D + 3 * D + D) + rings + 3 * _round_up(28 * self.n_units, 256)


# ---------------------------------------------------------------- c. the utterance walk, audio

AUDIO_SAMPLES = (400, 0, 560, 399, 720, 400, 560)    # one frame, none (unit UTT_CAP: no sample at all), two, none, three


class Audio(Case):
    """FbankKernel -> the reference's CMVN: int16 waves through the 40-bin front-end"""
    feat_dim = 40

    def __init__(self):
        Case.__init__(self)
        rows = np.concatenate([self.fbank(i) for i in range(POOL)])
        self.stats = np.concatenate([rows.astype(np.float64).mean(axis=0) * 2500.0, [2500.0]]).astype(F32)

    def content(self, i):
        return FA.wave_i16(AUDIO_SAMPLES[i], 300 + i)

    def frames(self, x):
        return O.num_frames(len(x))

    def front_end(self, x):
        return O.Fbank().compute(x.astype(F32))

    def fbank(self, i):
        x = self.content(i)
        return self.front_end(x) if self.frames(x) else np.zeros((0, self.feat_dim), F32)

    def normalise(self, rows):
        return O.cmvn(self.stats, rows)

    def stage(self, x, p):
        return self.normalise(self.front_end(x))

    def total_samples(self):
        n = np.array(AUDIO_SAMPLES, np.int64)
        return int(n[np.arange(self.n_units) % POOL].sum())

    def extra_bytes(self):
        frames = self.total_samples() // 160 + self.n_units
        return 2 * self.total_samples() + 4 * frames * self.feat_dim

    def device_bytes(self, live=False):
        frames = self.total_samples() // 160 + self.n_units
        return core_bytes(self.feat_dim, self.num_pdfs, [8], self.left, self.right, self.n_units, frames) + self.extra_bytes()


class AudioMfcc(Audio):
    """FbankAnyKernel -> CmvnChainKernel: the 13-of-23 MFCC"""
    feat_dim = 13
    spec = FA.BATCH_SPECS[13]

    def front_end(self, x):
        return FA.frontend_any(x, self.spec, pk.frontend_tables(self.spec))

    def normalise(self, rows):
        return CA.cmvn_any(self.stats, rows)


# ---------------------------------------------------------------- d. resample items

RESAMPLE_POOL = ((8000, 200), (44100, 1103), (8000, 280), (16000, 400), (44100, 1544), (8000, 205), (44100, 1110))   # (rate, samples)
_NATIVE = [i for i, (rate, _) in enumerate(RESAMPLE_POOL) if rate != 16000]


class Resample(Case):
    """Resampler::Run: a unit is a wave, an ITEM a wave that is not at 16 kHz (those are copied): item k is wave
    (k // 6) * 7 + _NATIVE[k % 6], and the batch is as long as it takes for RESAMPLE_ITEMS_CAP + 2 items."""
    cap, n_items = RESAMPLE_ITEMS_CAP, RESAMPLE_ITEMS_CAP + 2
    item_period = len(_NATIVE)
    feat_dim = 40

    def __init__(self):
        Case.__init__(self)
        self.n_units = self.wave_of_item(self.n_items - 1) + 1
        self._tables = {}
        self.stats = case("audio").stats                        # (the statistics of the audio case's features)

    @staticmethod
    def wave_of_item(k):
        return (k // len(_NATIVE)) * POOL + _NATIVE[k % len(_NATIVE)]

    def rtable(self, rate):
        """the model's table with the library's float32 weights"""
        if rate not in self._tables:
            self._tables[rate] = RM.with_weights(RM.table(rate), pk.resample_table(rate).weights)
        return self._tables[rate]

    def content(self, i):
        rate, n = RESAMPLE_POOL[i]
        return rate, np.round(3000 * np.random.default_rng([0x5A3, i]).standard_normal(n)).astype(F32)

    def converted(self, x):
        rate, w = x
        return w if rate == 16000 else RM.resample(self.rtable(rate), w)

    def frames(self, x):
        return O.num_frames(len(self.converted(x)))

    def stage(self, x, p):
        return O.cmvn(self.stats, O.Fbank().compute(self.converted(x)))

    def late_units(self):
        return [(self.wave_of_item(k), self.wave_of_item(k - self.cap)) for k in range(self.cap, self.n_items)]

    def wrapped_content(self, u, src):
        rate, own = self.content(u % POOL)
        return rate, np.resize(self.content(src % POOL)[1], own.shape).astype(F32)

    def total_samples(self):
        n = np.array([len(self.converted(self.content(i))) for i in range(POOL)], np.int64)
        return int(n[np.arange(self.n_units) % POOL].sum())

    def device_bytes(self, live=False):
        native = np.array([0 if rate == 16000 else n for rate, n in RESAMPLE_POOL], np.int64)
        native = int(native[np.arange(self.n_units) % POOL].sum())
        frames = self.total_samples() // 160 + self.n_units
        return (core_bytes(self.feat_dim, self.num_pdfs, [8], self.left, self.right, self.n_units, frames) + 4 * self.total_samples() + 4 * native
                + 4 * frames * self.feat_dim + 128 * self.n_items)


# ---------------------------------------------------------------- a. the row walk of the layer kinds

ROW_UTTS = (100003, 100005)          # one pass of 200 008 rows: the last 68 936 lie in the second turn
ELEMENTWISE = ("tanh", "mul", "add", "sigmoid")


def row_layers(kinds=ELEMENTWISE, pnorm=True):
    """Linear 2 -> 4, ReLU, Linear 4 -> 6, the elementwise kinds, p-norm 6 -> 3, Softmax: everything behind the second
    Linear runs in the frame-major layout -> (layers, prior)"""
    rng = np.random.default_rng(0x20A5)
    v = {"mul": rng.uniform(0.5, 2.0, 6).astype(F32), "add": rng.standard_normal(6).astype(F32)}
    layers = [LC._linear(rng, 2, 4), ("relu",), LC._linear(rng, 4, 6)] + [(k, v[k]) if k in v else (k,) for k in kinds]
    layers += ([("pnorm", 3)] if pnorm else []) + [("softmax",)]
    n = 3 if pnorm else 6
    return layers, np.random.default_rng(0x20A6).uniform(0.1, 0.4, n).astype(F32)


class RowWalk(Case):
    """LayerElementwiseKernel in the rows layout: a unit is a row of the pass, L = R = 0, row r has the content of
    rows_pool[r % 1021] (layer_cases.designed: the special values and three non-finite rows, a +inf and a -inf feature
    among them -- the hidden widths 4 and 6 are no multiples of 16, so the panels' padding rows are in play)."""
    cap, n_units = LAYER_LINES_CAP, sum(ROW_UTTS)
    content_period = ROWS_POOL
    feat_dim, left, right = 2, 0, 0
    variants = ("unprocessed", "wrapped", "twice")

    def __init__(self, kinds=ELEMENTWISE, pnorm=True):
        self.layers, self.prior = row_layers(kinds, pnorm)
        self.pool = LC.designed(ROWS_POOL, 2, 0x20A7)
        self._table = None

    def table(self, times=1):
        """[1021][N]; times: how often each elementwise kind behind the last Linear is applied"""
        if times == 1 and self._table is not None:
            return self._table
        layers = []
        for l in self.layers:
            layers += [l] * (times if l[0] in ELEMENTWISE else 1)
        tab = LC.loglik(layers, self.pool, self.prior, 0, 0, SCALE)
        if times == 1:
            self._table = tab
        return tab

    def utterances(self):
        """the two utterances' features"""
        rows = self.pool[np.arange(self.n_units) % ROWS_POOL]
        return [rows[:ROW_UTTS[0]], rows[ROW_UTTS[0]:]]

    def unit_lengths(self):
        return np.ones(self.n_units, np.int64)

    def expected(self):
        return self.table()[np.arange(self.n_units) % ROWS_POOL], self.unit_lengths()

    def variant(self, which):
        assert which in self.variants, which
        r = np.arange(self.n_units)
        rows = self.table()[r % ROWS_POOL].copy()
        late = r >= self.cap
        if which == "wrapped":
            rows[late] = self.table()[(r[late] - self.cap) % ROWS_POOL]
        else:
            rows[late] = self.table(0 if which == "unprocessed" else 2)[r[late] % ROWS_POOL]
        return rows

    def device_bytes(self, live=False):
        return core_bytes(2, self.num_pdfs, [4, 6], 0, 0, len(ROW_UTTS), self.n_units) + 4 * self.n_units * 2


CASES = {"layout": Layout, "cmvn_chain": CmvnChain, "norm_utterance": NormUtterance, "norm_speaker": NormSpeaker, "online_cmvn": OnlineCmvn,
         "delta": Delta, "transform_global": TransformGlobal, "transform_utt": TransformUtt, "chained": Chained, "live_layout": LiveLayout, "live_chain": LiveChain,
         "audio": Audio, "audio_mfcc": AudioMfcc, "resample": Resample, "row_walk": RowWalk}
LIVE = ("live_layout", "live_chain")                     # the cases the live objects run
_made = {}


def case(name):
    """the case, made once: its table is shared by the tests that need it and left unchanged"""
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]
