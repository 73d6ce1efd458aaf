"""Raw features at the model's own dimension: CmvnChainKernel in front of FeatureLayoutKernel in
pk.FeatureScorer, StreamCmvnChainKernel in front of StreamFeatureLayoutKernel in pk.OnlineFeatureScorer.
  * Batch: fetch_cmvn equals the chunk rule (tests/cmvn_any_cases.py: the 40-dim oracle, 40 columns at a time) bit for
    bit at every dimension and context, ragged batches with frameless utterances first, in the middle and last; the RAW
    log-likelihoods equal the same scorer's NORMALIZED ones on the chunk rule's output (the pads, through the scores);
    host and device entry, both softmax modes.
  * Non-finite values stay in their column; reuse and poisoned neighbours change no bit; f16x3 at D = 80 is held to
    the oracle at 1e-4 max(|ref|, 1).
  * Online: over a slot's life the rows are the batch RAW result bit for bit at every chunking, first_frame
    continuing; reopened slots, NaN neighbours; the online decoder downstream.
  * Failure codes, before anything is copied or launched."""
import ctypes as C

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth
from pocketkaldi_amd import synth_graph as SG
from oracle import oracle as O

import cmvn_any_cases as CA
from test_gpu_parity import assert_loglik_close
from test_gpu_stream_features import assert_jobs, job, run_jobs

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
BATCH_DIMS = [1, 3, 39, 41, 63, 64, 65, 80, 130]
BATCH_CONTEXTS = [(0, 0), (2, 1), (5, 5), (70, 3)]
BATCH_FRAMES = (0, 1, 2, 599, 600, 0, 601, 664, 1201, 1307, 0)      # frameless first, in the middle and last
ONLINE_DIMS = [1, 39, 41, 64, 65, 130]
ONLINE_CONTEXTS = [(0, 0), (2, 1), (5, 5)]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def tiny(D, L, R, softmax="stable", precision="f32"):
    layers, prior, _, _ = synth.model("tiny", feat_dim=D, left=L, right=R)
    return pk.AcousticModel(layers, prior, L, R, precision=precision).set_softmax(softmax), layers, prior


def fetch_rows(fs):
    return [fs.fetch(u).log_prob() for u in range(fs.num_utts())]


_cases = {}


def batch_case(D):
    """(statistics, raw utterances, the chunk rule's output) at dimension D: computed once, shared, left unchanged."""
    if D not in _cases:
        g = CA.stats_for(D)
        raw = [CA.features(T, D, u) for u, T in enumerate(BATCH_FRAMES)]
        _cases[D] = (g, raw, [CA.cmvn_any(g, x) for x in raw])
    return _cases[D]


class DeviceCopy:
    """The utterances' rows one after the other in HBM, one row into the allocation (4-byte aligned and no better)."""

    def __init__(self, feats, D):
        cat = np.ascontiguousarray(np.concatenate(feats))
        self.base = pk.lib().pk_mi355_device_malloc(cat.nbytes + 4 * D)
        assert self.base
        self.ptr = self.base + 4 * D
        assert pk.lib().pk_mi355_memcpy(C.c_void_p(self.ptr), cat.ctypes.data_as(C.c_void_p), cat.nbytes, 1) == 0

    def free(self):
        pk.lib().pk_mi355_device_free(C.c_void_p(self.base))


# ---------------------------------------------------------------- batch: the chunk rule, bit for bit

@pytest.mark.parametrize("D", BATCH_DIMS)
def test_batch_raw_is_the_chunk_rule_and_the_pads_hold_through_the_scores(D):
    g, raw, want = batch_case(D)
    frames = [x.shape[0] for x in raw]
    dev = DeviceCopy(raw, D)
    try:
        for k, (L, R) in enumerate(BATCH_CONTEXTS):
            am, _, _ = tiny(D, L, R, softmax=("stable", "reference")[k % 2])
            assert am.feat_dim() == D
            fs = pk.FeatureScorer(am, len(raw), sum(frames), global_stats=g)
            what = "D=%d L=%d R=%d" % (D, L, R)
            fs.enable_timing(True)
            fs.set_features(raw, "raw")
            fs.score(0.1)
            t = fs.timing()
            assert t["fbank"][1] == 0 and t["cmvn"][1] == 1, t               # chain and layout share the CMVN slot
            rows = fetch_rows(fs)
            for u, x in enumerate(raw):
                assert fs.num_frames(u) == x.shape[0]
                assert bits_equal(fs.fetch_fbank(u), x), "%s utterance %d: fetch_fbank is not the input" % (what, u)
                assert bits_equal(fs.fetch_cmvn(u), want[u]), "%s utterance %d (%d frames): CMVN differs" % (what, u, x.shape[0])
                assert rows[u].shape[0] == x.shape[0] and np.isfinite(rows[u]).all()
            fs.set_features(want, "normalized")                               # the same scorer on the chunk rule's output
            fs.score(0.1)
            for u, r in enumerate(fetch_rows(fs)):
                assert bits_equal(r, rows[u]) or frames[u] == 0, "%s utterance %d: RAW rows differ from NORMALIZED rows" % (what, u)
            fs.set_features_device(dev.ptr, frames, "raw")                    # the device entry
            fs.score(0.1)
            for u, r in enumerate(fetch_rows(fs)):
                assert bits_equal(fs.fetch_cmvn(u), want[u]), "%s utterance %d: device entry, CMVN differs" % (what, u)
                assert bits_equal(r, rows[u]) or frames[u] == 0, "%s utterance %d: device entry, rows differ" % (what, u)
            fs.close()
            am.close()
    finally:
        dev.free()


# ---------------------------------------------------------------- non-finite values stay in their column

def test_non_finite_values_stay_in_their_column():
    D, T = 65, 1300
    am, _, _ = tiny(D, 2, 1)
    g = CA.stats_for(D)
    x = CA.features(T, D, 50)
    x[300, 5], x[350, 64], x[100, 7] = np.nan, np.inf, -0.0                  # (the +inf leaves the window at t = 950: inf - inf)
    want = CA.cmvn_any(g, x)
    touched = np.zeros(D, bool)
    touched[[5, 64]] = True
    assert np.isnan(want[:, touched]).any() and np.isfinite(want[:, ~touched]).all()
    fs = pk.FeatureScorer(am, 1, T, global_stats=g)
    fs.set_features([x], "raw")
    fs.score(0.1)
    got = fs.fetch_cmvn(0)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok])  # every other value, the untouched columns among them
    fs.close()
    am.close()


# ---------------------------------------------------------------- reuse and isolation

def test_one_scorer_alternating_sources_and_a_poisoned_neighbour():
    D, L, R = 41, 2, 1
    am, _, _ = tiny(D, L, R)
    g = CA.stats_for(D)
    sets = {"large": [CA.features(T, D, 60 + u) for u, T in enumerate((700, 0, 64, 1))], "small": [CA.features(T, D, 70 + u) for u, T in enumerate((5, 130))]}
    cap = sum(x.shape[0] for x in sets["large"])

    def fresh(feats, kind):
        fs = pk.FeatureScorer(am, 4, cap, global_stats=g)
        fs.set_features(feats, kind)
        fs.score(0.1)
        out = ([fs.fetch_cmvn(u) for u in range(len(feats))], fetch_rows(fs))
        fs.close()
        return out

    want = {(k, kind): fresh(v, kind) for k, v in sets.items() for kind in ("raw", "normalized")}
    devs = {k: DeviceCopy(v, D) for k, v in sets.items()}
    one = pk.FeatureScorer(am, 4, cap, global_stats=g)

    def check(which, kind, device):
        feats = sets[which]
        if device:
            one.set_features_device(devs[which].ptr, [x.shape[0] for x in feats], kind)
        else:
            one.set_features(feats, kind)
        one.score(0.1)
        cm, rows = want[(which, kind)]
        for u in range(len(feats)):
            assert bits_equal(one.fetch_cmvn(u), cm[u]), (which, kind, device, u)
            assert bits_equal(one.fetch(u).log_prob(), rows[u]) or feats[u].shape[0] == 0, (which, kind, device, u)

    def poison():
        one.set_features([np.full(x.shape, np.nan, np.float32) for x in sets["large"]], "raw")
        one.score(0.1)
        assert all(np.isnan(r).all() for r in fetch_rows(one))

    try:
        for which in ("large", "small", "large"):
            for kind, device in (("raw", False), ("normalized", True), ("raw", True), ("normalized", False), ("raw", False)):
                check(which, kind, device)
                if kind == "normalized":
                    poison()
        # a poisoned neighbour: NaN and 1e30 utterances between healthy ones
        feats = list(sets["large"])
        mixed = [feats[0], np.full((650, D), np.nan, np.float32), feats[2], np.full((3, D), 1e30, np.float32), feats[3]]
        wide = pk.FeatureScorer(am, 5, cap + 653, global_stats=g)
        wide.set_features(mixed, "raw")
        wide.score(0.1)
        cm, rows = want[("large", "raw")]
        for at, u in ((0, 0), (2, 2), (4, 3)):
            assert bits_equal(wide.fetch_cmvn(at), cm[u]) and bits_equal(wide.fetch(at).log_prob(), rows[u]), at
        assert np.isnan(wide.fetch(1).log_prob()).all()
        wide.close()
    finally:
        for d in devs.values():
            d.free()
    one.close()
    am.close()


# ---------------------------------------------------------------- f16x3

def test_f16x3_at_80_within_the_contract_of_the_oracle():
    D, L, R = 80, 2, 1
    am, layers, prior = tiny(D, L, R, precision="f16x3")
    g = CA.stats_for(D)
    raw = [CA.features(T, D, 80 + u) for u, T in enumerate((701, 0, 130, 5))]
    fs = pk.FeatureScorer(am, len(raw), sum(x.shape[0] for x in raw), global_stats=g)
    fs.set_features(raw, "raw")
    fs.calibrate()
    fs.score(0.1)
    nn = O.Nnet(layers)
    worst = 0.0
    for u, x in enumerate(raw):
        got = fs.fetch(u).log_prob()
        if x.shape[0] == 0:
            assert got.shape[0] == 0
            continue
        assert bits_equal(fs.fetch_cmvn(u), CA.cmvn_any(g, x)), u            # CMVN is f32, in front of the split
        ref = nn.am_compute(CA.cmvn_any(g, x), prior, L, R, 0.1)
        worst = max(worst, float((np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)).max()))
        print("CMVN_ANY_F16X3_MAX_ERR utterance %d: %.3e" % (u, worst))
        assert_loglik_close(got, ref)
    print("CMVN_ANY_F16X3_MAX_ERR %.3e (contract 1e-4)" % worst)
    fs.close()
    am.close()


# ---------------------------------------------------------------- online

def batch_rows(am, g, feats):
    fs = pk.FeatureScorer(am, len(feats), max(sum(f.shape[0] for f in feats), 1), global_stats=g)
    fs.set_features(feats, "raw")
    fs.score(0.1)
    out = fetch_rows(fs)
    fs.close()
    return out


def ends_at(n, ends, step=97):
    """Chunks whose pushes end at each of `ends` (below n) on the way to n."""
    cuts = sorted({e for e in ends if 0 < e < n} | set(range(step, n, step)) | {n})
    return [b - a for a, b in zip([0] + cuts[:-1], cuts)]


@pytest.mark.parametrize("L,R", ONLINE_CONTEXTS)
@pytest.mark.parametrize("D", ONLINE_DIMS)
def test_online_rows_equal_the_batch_raw_result_at_every_chunking(D, L, R):
    am, _, _ = tiny(D, L, R, softmax=("stable", "reference")[(D + L) % 2])
    g = CA.stats_for(D)
    lengths = [0, 1, 2, R, R + 1, 599, 600, 601, 1307]
    feats = [CA.features(T, D, 100 + u) for u, T in enumerate(lengths)]
    want = batch_rows(am, g, feats)
    assert all(np.isfinite(w).all() for w in want)
    sc = pk.OnlineFeatureScorer(am, len(lengths), sum(lengths), global_stats=g)
    assert sc.feat_dim() == D
    rng = np.random.default_rng([D, L, R])
    # (closed a step later: with R > 0 that step's rows are served from the history alone)
    for how, with_last in (("whole", False), ("whole", True), (1, True), (7, False), (7, True), (64, True), (64, False), ("random", False),
                           ("random", True), ("edges", False), ("edges", True)):
        jobs = [job(u, "raw", f, "whole" if how == "edges" else how, int(rng.integers(0, 4)), with_last, rng) for u, f in enumerate(feats)]
        if how == "edges":
            for j, T in zip(jobs, lengths):
                j["chunks"] = ends_at(T, (599, 600, 601)) if T else [0]
        assert_jobs(sc, jobs, want, "D=%d L=%d R=%d %s close_with_last=%s" % (D, L, R, how, with_last))
    sc.destroy()
    am.close()


def test_online_reopened_slots_and_nan_neighbours_change_no_bit():
    D, L, R = 65, 2, 1
    am, _, _ = tiny(D, L, R)
    g = CA.stats_for(D)
    a, b = CA.features(701, D, 200), CA.features(130, D, 201)
    nan = np.full((705, D), np.nan, np.float32)
    norm = CA.cmvn_any(g, b)
    want_a, want_b = batch_rows(am, g, [a, b])
    sc = pk.OnlineFeatureScorer(am, 3, 3 * 705, global_stats=g)
    # NaN streams beside healthy ones, RAW and NORMALIZED in the same steps
    got = run_jobs(sc, [job(0, "raw", nan, 64), job(1, "raw", a, 64), job(2, "normalized", norm, 10), job(0, "raw", b, 10)])
    assert np.isnan(got[0]).all() and bits_equal(got[1], want_a) and bits_equal(got[2], want_b) and bits_equal(got[3], want_b)
    for slot in range(3):                                    # every slot reopened after a NaN stream that filled ring and sums
        assert np.isnan(run_jobs(sc, [job(slot, "raw", nan, "whole")])[0]).all()
        assert_jobs(sc, [job(slot, "raw", a, 100)], [want_a], "reopened raw %d" % slot)
        assert_jobs(sc, [job(slot, "normalized", norm, 7)], [want_b], "other kind %d" % slot)
    sc.destroy()
    am.close()


def test_online_decoder_over_raw_features_equals_decode_batch(tmp_path):
    D, Lc, Rc = 65, 2, 1
    am, _, _ = tiny(D, Lc, Rc)
    g = CA.stats_for(D)
    graph = SG.word_loop(30, 8, seed=3)
    assert graph["num_tids"] <= am.num_pdfs()
    path = str(tmp_path / "loop.fst")
    SG.write_fst(path, graph["start"], graph["final"], graph["arcs"])
    fst = pk.Fst(path)
    feats = [CA.features(T, D, 300 + u) for u, T in enumerate((120, 1, 0, 75, 640, 33))]
    n = len(feats)
    fs = pk.FeatureScorer(am, n, sum(f.shape[0] for f in feats), global_stats=g)
    fs.set_features(feats, "raw")
    fs.score(0.1)
    whole = pk.Decoder(fst, am, n)
    whole.decode_batch(fs)
    want = [whole.result(u) for u in range(n)]
    sc = pk.OnlineFeatureScorer(am, n, n * 10, global_stats=g)
    dec = pk.OnlineDecoder(fst, am, n)
    pos, state, got, step = [0] * n, ["pending"] * n, [None] * n, 0
    while any(s != "done" for s in state):
        for u in range(n):
            if state[u] == "pending" and step >= u % 3:
                sc.open_features(u, "raw")
                dec.open(u)
                state[u] = "open"
            if state[u] == "open":
                sc.push_features(u, feats[u][pos[u]:pos[u] + 10])
                pos[u] += 10
                if pos[u] >= feats[u].shape[0]:
                    sc.close(u)
                    state[u] = "closed"
        sc.step(0.1, sync=False)
        dec.advance(sc)
        for u in range(n):
            if state[u] == "closed":
                got[u] = dec.result(u)
                state[u] = "done"
        step += 1
    for u in range(n):
        assert got[u][0] == want[u][0] and np.float32(got[u][1]).tobytes() == np.float32(want[u][1]).tobytes(), u
        assert got[u][2] == want[u][2], u
    assert any(w[0] for w in want)
    for o in (sc, dec, whole, fs):
        getattr(o, "destroy", getattr(o, "close", None))()
    am.close()


# ---------------------------------------------------------------- failure codes

def code_of(call, *args, **kw):
    with pytest.raises(pk.PkCodeError) as e:
        call(*args, **kw)
    return e.value.code


def test_every_failure_code_and_the_objects_stay_usable():
    Lib = pk.lib()
    D, L, R = 65, 2, 1
    am, _, _ = tiny(D, L, R)
    am40, _, _ = tiny(40, 2, 1)
    g, g41 = CA.stats_for(D), CA.stats_for(40)
    f32p = C.POINTER(C.c_float)
    gp = g.ctypes.data_as(f32p)
    x = CA.features(6, D, 400)
    (want,) = batch_rows(am, g, [x])
    # create: the length must be feat_dim + 1, and the text names both numbers
    for entry in (Lib.pk_mi355_features_batch_create_stats, Lib.pk_mi355_features_stream_create_stats):
        for n in (41, D, D + 2):
            assert entry(am.handle, gp, n, 2, 100) is None and Lib.pk_mi355_last_error_code() == E_INVALID
            msg = Lib.pk_mi355_last_error().decode()
            assert str(n) in msg and str(D + 1) in msg, msg
        assert entry(am.handle, None, D + 1, 2, 100) is None and Lib.pk_mi355_last_error_code() == E_INVALID
        for units, frames in ((0, 100), (2, 0), (-1, 100)):
            assert entry(am.handle, gp, D + 1, units, frames) is None and Lib.pk_mi355_last_error_code() == E_INVALID
        h = entry(am40.handle, g41.ctypes.data_as(f32p), 41, 2, 100)           # at 40 it is the old entry
        assert h
        (Lib.pk_mi355_batch_destroy if entry is Lib.pk_mi355_features_batch_create_stats else Lib.pk_mi355_stream_destroy)(C.c_void_p(h))
    # the old entries refuse what they refused: 41 statistics with a 65-dim model
    assert code_of(pk.FeatureScorer, am, 2, 100, global_stats=g41) == E_INVALID and "40-dim" in Lib.pk_mi355_last_error().decode()
    assert code_of(pk.OnlineFeatureScorer, am, 2, 100, global_stats=g41) == E_INVALID and "40-dim" in Lib.pk_mi355_last_error().decode()
    with pytest.raises(pk.PkError, match="41"):
        pk.FeatureScorer(am, 2, 100, global_stats=g[:-1])
    # batch: RAW without statistics, capacity; the scorer keeps what it held and stays usable
    plain, stats = pk.FeatureScorer(am, 2, 100), pk.FeatureScorer(am, 2, 100, global_stats=g)
    stats.set_features([x], "raw")
    assert code_of(plain.set_features, [x], "raw") == E_INVALID and "statistics" in Lib.pk_mi355_last_error().decode()
    assert "pk_mi355_features_batch_create_stats" in Lib.pk_mi355_last_error().decode() and "40-dim" not in Lib.pk_mi355_last_error().decode()
    n6 = (C.c_int * 1)(6)
    assert Lib.pk_mi355_features_set_device(plain._h, C.c_void_p(256), n6, 1, 1) == E_INVALID       # (never dereferenced)
    assert code_of(stats.set_features, [CA.features(101, D, 401)], "raw") == E_INVALID and "capacity" in Lib.pk_mi355_last_error().decode()
    assert code_of(stats.set_features, [x, x, x], "raw") == E_INVALID
    assert code_of(stats.set_features, [CA.features(6, 40, 402)], "raw") == E_INVALID
    stats.score(0.1)                                           # what it held before the refusals
    assert bits_equal(stats.fetch(0).log_prob(), want)
    plain.set_features([CA.cmvn_any(g, x)], "normalized")
    plain.score(0.1)
    assert bits_equal(plain.fetch(0).log_prob(), want)
    plain.close()
    stats.close()
    # online: RAW without statistics, capacity
    oplain, ostats = pk.OnlineFeatureScorer(am, 2, 100), pk.OnlineFeatureScorer(am, 2, 100, global_stats=g)
    assert code_of(oplain.open_features, 0, "raw") == E_INVALID and "statistics" in Lib.pk_mi355_last_error().decode()
    ostats.open_features(0, "raw")
    ostats.push_features(0, x[:4])
    assert code_of(ostats.push_features, 0, CA.features(97, D, 403)) == E_INVALID and "capacity" in Lib.pk_mi355_last_error().decode()
    ostats.push_features(0, x[4:])
    ostats.close(0)
    ostats.step(0.1)
    first, rows = ostats.fetch(0)
    assert first == 0 and bits_equal(rows, want)
    assert_jobs(oplain, [job(0, "normalized", CA.cmvn_any(g, x), 4)], [want], "plain object, normalized")
    oplain.destroy()
    ostats.destroy()
    am.close()
    am40.close()
