"""Every kernel's second grid walk: batches of cap + 2 units -- utterances, slots, rows, resample
items -- of almost nothing, so that each capped launch walks its stride loop a second time (or, the resampler and the
audio front-end, issues its second launch).  The cases and their expectations are tests/grid_walk_cases.py's; every row
of every unit is compared bit for bit (NaN for NaN), f32 layers, softmax mode "reference", all results from one
transfer.  tests/test_grid_walk_cases.py shows without a GPU that these comparisons tell a dropped turn, a wrapped unit
and a doubled activation from the expectation."""
import ctypes as C

import numpy as np
import pytest

import pocketkaldi_amd as pk

import grid_walk_cases as GW
import norm_cases as NC

pytestmark = pytest.mark.gpu

F32 = np.float32
BOUNDARY = (0, GW.UTT_CAP - 1, GW.UTT_CAP, GW.UTT_CAP + 1)


@pytest.fixture(autouse=True)
def one_pass(monkeypatch):
    """Passes of the default 262 144 rows, whatever the environment says."""
    monkeypatch.setenv("PK_MI355_CHUNK", str(GW.CHUNK))


# ---------------------------------------------------------------- helpers

def pooled(c):
    """every unit's content: the pool's arrays, by reference"""
    pool = [c.content(i) for i in range(c.content_period)]
    return [pool[u % c.content_period] for u in range(c.n_units)]


def pooled_params(c):
    params = [c.param(j) for j in range(c.param_period)]
    return [params[u % c.param_period] for u in range(c.n_units)]


def model_of(c):
    return pk.AcousticModel(c.layers, c.prior, c.left, c.right).set_softmax("reference")


def gather(addr, T, N, read):
    """Rows of all units, in unit order, from one span of memory: unit u has T[u] rows of N floats at address addr[u].
    read(first address, floats) -> the span as a float32 array."""
    live = T > 0
    if not live.any():
        return np.zeros((0, N), F32)
    lo = int(addr[live].min())
    hi = int((addr[live] + 4 * N * T[live]).max())
    span = read(lo, (hi - lo) // 4).reshape(-1, N)
    first_row = (addr[live] - lo) // (4 * N)
    t = T[live]
    start = np.concatenate([[0], np.cumsum(t)])[:-1]
    return span[np.repeat(first_row - start, t) + np.arange(int(t.sum()))]


def all_rows(fs):
    """fetch_all: one transfer; -> ([sum T][N] rows in utterance order, the utterances' frame counts).  The views of one
    fetch_all all point into the batch's one page-locked arena (pk_mi355.h), so the span from the lowest view to the end
    of the highest is readable memory; the views' fields are read directly to spare 65 537 copies."""
    views = fs.fetch_all()
    N = fs._am.num_pdfs()
    T = np.fromiter((d._d.log_prob.ncol for d in views), np.int64, len(views))
    addr = np.fromiter((C.cast(d._d.log_prob.data, C.c_void_p).value or 0 for d in views), np.int64, len(views))
    rows = gather(addr, T, N, lambda lo, n: np.ctypeslib.as_array(C.cast(C.c_void_p(lo), C.POINTER(C.c_float)), shape=(n,))).copy()
    del views
    return rows, T


def assert_units(c, got, T, what):
    want, want_T = c.expected()
    assert T.shape == want_T.shape and np.array_equal(T, want_T), "%s: frame counts differ at units %s" % (what, np.flatnonzero(T != want_T)[:8])
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if GW.same(got, want):
        return
    bad = ((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).any(axis=1)
    ends = np.cumsum(want_T)
    units = np.unique(np.searchsorted(ends, np.flatnonzero(bad), side="right"))
    raise AssertionError("%s: %d rows of %d units differ, %d of those units at or past the cap %d; the first: %s"
                         % (what, int(bad.sum()), units.size, int((units >= c.cap).sum()), c.cap, units[:8].tolist()))


def run_features(name, kind, make=None, before=None, after=None):
    """The case through a FeatureScorer: make(am, units, frames) -> the scorer; before / after(fs): the calls in front of
    and behind set_features.  -> the scorer, scored and checked (the caller closes it)"""
    c = GW.case(name)
    am = model_of(c)
    fs = make(am, c.n_units, c.total_frames()) if make else pk.FeatureScorer(am, c.n_units, c.total_frames())
    if before:
        before(fs)
    fs.set_features(pooled(c), kind)
    if after:
        after(fs)
    fs.score(GW.SCALE)
    rows, T = all_rows(fs)
    assert_units(c, rows, T, name)
    return fs, am


def done(fs, am):
    fs.close()
    am.close()


# ---------------------------------------------------------------- a. the row walk of the layer kinds

def run_row_walk(c, what):
    am = model_of(c)
    fs = pk.FeatureScorer(am, len(GW.ROW_UTTS), c.n_units)
    fs.set_features(c.utterances(), "normalized")
    fs.score(GW.SCALE)
    assert fs.total_frames() == c.n_units > GW.LAYER_LINES_CAP
    rows, T = all_rows(fs)
    assert T.tolist() == list(GW.ROW_UTTS)
    assert_units(c, rows, np.ones(c.n_units, np.int64), what)
    done(fs, am)


def test_row_walk_of_the_layer_kinds():
    """tanh, mul, add, sigmoid and the p-norm behind the last Linear, one pass of 200 008 rows: the rows from 131 072 on
    are the second turn of the elementwise kinds' line walk."""
    run_row_walk(GW.case("row_walk"), "row walk")


@pytest.mark.parametrize("kind", GW.ELEMENTWISE)
def test_row_walk_of_each_kind_alone(kind):
    run_row_walk(GW.RowWalk((kind,), pnorm=False), "row walk, %s alone" % kind)


# ---------------------------------------------------------------- b. the utterance walk, features

def test_feature_layout_kernel():
    """L = 2, R = 1: compact rows, and the shift4 table at the shifts 65 537 utterances add up to"""
    done(*run_features("layout", "normalized"))


def test_cmvn_chain_kernel():
    c = GW.case("cmvn_chain")
    done(*run_features("cmvn_chain", "raw", make=lambda am, n, frames: pk.FeatureScorer(am, n, frames, global_stats=c.stats)))


def test_norm_kernel_utterance_mode():
    c = GW.case("norm_utterance")
    fs, am = run_features("norm_utterance", "raw", before=lambda fs: fs.set_norm(pk.NormSpec("utterance", True, True)))
    for u in BOUNDARY:
        assert NC.bits_equal(fs.norm_stats(u), c.record(u % GW.POOL)), u
    empty = fs.norm_stats(GW.UTT_CAP)                   # the `continue` of an empty utterance, on the second turn
    assert fs.num_frames(GW.UTT_CAP) == 0 and empty.tobytes() == np.zeros((2, GW.D + 1)).tobytes()
    done(fs, am)


def test_norm_kernel_speaker_mode():
    c = GW.case("norm_speaker")

    def before(fs):
        fs.set_norm(pk.NormSpec("speaker", True, True))
        fs.set_speaker_stats(pooled_params(c))
    done(*run_features("norm_speaker", "raw", before=before))


def test_online_cmvn_kernel():
    c = GW.case("online_cmvn")

    def before(fs):
        fs.set_norm(pk.OnlineCmvnSpec(*c.spec), c.glob)
        fs.set_speaker_stats(pooled_params(c))
    done(*run_features("online_cmvn", "raw", before=before))


def test_delta_kernel():
    c = GW.case("delta")

    def make(am, n, frames):
        fs = pk.FeatureScorer(am, n, frames, deltas=pk.DeltaSpec(c.order, c.window))
        assert fs.base_dim() == GW.D and fs.feat_dim() == c.feat_dim
        return fs
    done(*run_features("delta", "raw", make=make, before=lambda fs: fs.set_norm(pk.NormSpec("none"))))


def test_transform_kernel_global_matrix():
    c = GW.case("transform_global")
    done(*run_features("transform_global", "raw", make=lambda am, n, frames: pk.FeatureScorer(am, n, frames, transform=pk.TransformSpec(c.matrix, c.xl, c.xr)),
                       before=lambda fs: fs.set_norm(pk.NormSpec("none"))))


def test_transform_kernel_per_utterance_matrices():
    c = GW.case("transform_utt")
    done(*run_features("transform_utt", "raw", make=lambda am, n, frames: pk.FeatureScorer(am, n, frames, transform=pk.TransformSpec(None, in_dim=GW.D)),
                       before=lambda fs: fs.set_norm(pk.NormSpec("none")), after=lambda fs: fs.set_utt_transforms(pooled_params(c))))


def test_chained_stages():
    c = GW.case("chained")
    done(*run_features("chained", "raw",
                       make=lambda am, n, frames: pk.FeatureScorer(am, n, frames, deltas=pk.DeltaSpec(2, 2), transform=pk.TransformSpec(c.matrix, 1, 1)),
                       before=lambda fs: fs.set_norm(pk.NormSpec("utterance", True, True)), after=lambda fs: fs.set_utt_transforms(pooled_params(c))))


# ---------------------------------------------------------------- c. the utterance walk, audio

@pytest.mark.parametrize("name", ["audio", "audio_mfcc"])
def test_audio_front_end(name):
    """65 537 int16 waves: the front-end's launch goes out in two slices, the second at the layout arrays' offset 65 535"""
    c = GW.case(name)
    am = model_of(c)
    bs = pk.BatchScorer(am, c.stats, c.n_units, c.total_samples(), frontend=c.spec if name == "audio_mfcc" else None)
    bs.set_waves_i16(pooled(c))
    bs.score(GW.SCALE)
    for u in BOUNDARY:
        want = c.fbank(u % GW.POOL)
        assert bs.num_frames(u) == want.shape[0], u
        assert NC.bits_equal(bs.fetch_fbank(u), want), "%s: the front-end's rows of utterance %d differ" % (name, u)
    rows, T = all_rows(bs)
    assert_units(c, rows, T, name)
    done(bs, am)


# ---------------------------------------------------------------- d. resample items

def test_resample_items():
    """32 770 waves that are not at 16 kHz (and the 16 kHz ones between them, which are copied): the second launch of
    Resampler::Run starts at item 32 768"""
    c = GW.case("resample")
    am = model_of(c)
    content = pooled(c)
    bs = pk.BatchScorer(am, c.stats, c.n_units, c.total_samples())
    bs.set_waves([w for _, w in content], rates=[rate for rate, _ in content])
    bs.score(GW.SCALE)
    rows, T = all_rows(bs)
    assert_units(c, rows, T, "resample")
    done(bs, am)


# ---------------------------------------------------------------- e. live records

def step_rows(sc, n, N):
    """The rows the last step scored, all slots from one transfer -> (rows in slot order, first frame and count per slot)"""
    first, count, addr = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for u in range(n):
        p, f, k = sc.loglik_device(u)
        first[u], count[u], addr[u] = f, k, p or 0

    def read(lo, floats):
        out = np.zeros(floats, F32)
        assert pk.lib().pk_mi355_memcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(lo), 4 * floats, 2) == 0
        return out
    return gather(addr, count, N, read), first, count


def run_live(sc, c, kind, what):
    """Every slot opened, pushed its pool utterance in one chunk, stepped, closed and stepped: the rows over a slot's
    life are the batch case's."""
    n, N = c.n_units, c.num_pdfs
    feats = pooled(c)
    for u in range(n):
        sc.open_features(u, kind)
    for u in range(n):
        sc.push_features(u, feats[u])
    pushed = np.array([f.shape[0] for f in feats])
    assert c.records(pushed) > GW.UTT_CAP               # a record per slot that was pushed something: past the cap
    sc.step(GW.SCALE)
    rows1, first1, count1 = step_rows(sc, n, N)
    for u in range(n):
        sc.close(u)
    sc.step(GW.SCALE)
    rows2, first2, count2 = step_rows(sc, n, N)
    assert c.records(count2) > GW.UTT_CAP               # the close releases held-back frames in every slot: a record each
    assert not first1[count1 > 0].any() and np.array_equal(first2[count2 > 0], count1[count2 > 0])     # each step goes on where the last ended
    T = count1 + count2
    start = np.concatenate([[0], np.cumsum(T)])[:-1]
    rows = np.zeros((int(T.sum()), N), F32)
    for part, at, count in ((rows1, start, count1), (rows2, start + count1, count2)):
        own = np.concatenate([[0], np.cumsum(count)])[:-1]
        rows[np.repeat(at - own, count) + np.arange(int(count.sum()))] = part
    assert_units(c, rows, T, what)


def test_live_feature_layout():
    """65 537 slots that all push: each step has 65 537 records, and StreamFeatureLayoutKernel's walk takes its second turn"""
    c = GW.case("live_layout")
    am = model_of(c)
    sc = pk.OnlineFeatureScorer(am, c.n_units, c.total_frames())
    try:
        run_live(sc, c, "normalized", "live layout")
    finally:
        sc.destroy()
        am.close()


def test_live_deltas_and_transform():
    """a live object with deltas and a transform: StreamDeltaKernel and StreamTransformKernel past 65 535 records"""
    c = GW.case("live_chain")
    am = model_of(c)
    sc = pk.OnlineFeatureScorer.with_transform(am, c.n_units, c.total_frames(), pk.TransformSpec(c.matrix, 1, 1), deltas=pk.DeltaSpec(2, 2))
    try:
        sc.set_norm(pk.NormSpec("none"))
        run_live(sc, c, "raw", "live deltas and transform")
    finally:
        sc.destroy()
        am.close()
