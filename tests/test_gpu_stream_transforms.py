"""Feature transforms on the online scorers: StreamTransformKernel between the normaliser (or
StreamDeltaKernel) and StreamFeatureLayoutKernel of a scorer made by with_transform, with the spec's matrix and with the
slots' own.  The yardstick everywhere is the batch transform scorer (FeatureScorer / BatchScorer with transform=, itself
pinned to tests/transform_cases.py) on the whole input under the same normalisation, deltas and matrices; every
comparison is bitwise, each step's first_frame continues the last (stream_transform_cases.run_jobs).
  * Every in_dim, context pair, output dimension, affine or linear, model context and softmax mode pairwise; slot
    lengths around Rt, C, Rt + R, C + R and the kernel's run of G frames, each in a slot of one object, opened at different
    steps; pushed whole, 1 and 7 frames a step and in seeded random pushes with empty ones; closed with the last push, a
    step later and after two empty steps.  The widest spec (in_dim 512, C 16: 64 KiB of LDS) once.
  * Deltas in front; every norm mode in front, with norm_stats(slot) at Db; audio through an MFCC front-end at two rates
    with RAW and NORMALIZED slots in the same steps; the global matrix alone, the slots' own alone, both, and slots with and
    without one in the same step; NaN and 1e30 neighbours; a reopened slot in each ring parity; NaN, inf and -0.0 across a
    ring hand-over; scorers of the existing entries in the same process; every failure code.  (The decoder and the
    recognizer behind such a scorer: tests/test_gpu_online_recognizer_transforms.py.)
A matrix-less slot's rows reach the first layer as bits: the host restatement shows that for -0.0 and NaN payloads
(tests/test_stream_transform_host.py); here such a slot's scores are held to the batch scorer's, whose stage is a copy too."""
import os
import re

import numpy as np
import pytest

import pocketkaldi_amd as pk

import cmvn_any_cases as CA
import frontend_any_cases as FA
import norm_cases as NC
import stream_delta_cases as SD
import stream_transform_cases as ST
import transform_cases as TC
from test_gpu_cmvn_any import fetch_rows, tiny

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
IN_DIMS = [1, 13, 63, 64, 65]
SPLICES = [(0, 0), (3, 3), (0, 4), (5, 0), (8, 8)]
ROWS = [1, 40, 64, 65, 130]
CONTEXTS = [(0, 0), (2, 1), (5, 5)]
G = int(re.search(r"kTransformFrames\s*=\s*(\d+)", open(os.path.join(REPO, "pocketkaldi_amd", "csrc", "pk_transform_kernel.h")).read()).group(1))


def cell(i, k):
    """in_dim i and splice k -> (rows, affine, model context, softmax mode): a Latin square in the three five-level factors,
    the others rotating (test_the_cells_cover_every_pair)."""
    return (i + 2 * k) % 5, (i + k) % 5 % 2, (i + 3 * k) % 5 % 3, ((i + k) % 5 + i * k % 2) % 2


def code_of(call):
    with pytest.raises(pk.PkCodeError) as e:
        call()
    return e.value.code, str(e.value)


def rows_equal(got, want):
    """Bit for bit; a frameless input's batch rows have no columns either."""
    return got.shape[0] == 0 if want.shape[0] == 0 else NC.bits_equal(got, want)


def batch_rows(am, spec, raw, norm=None, g=None, glob=None, spk=None, stats=False, deltas=None, mats=None):
    """FeatureScorer(transform=) on the whole matrices as RAW, with per-utterance matrices `mats` when given -> (rows per
    matrix, norm_stats per matrix or None)."""
    fs = pk.FeatureScorer(am, len(raw), max(sum(x.shape[0] for x in raw), 1), global_stats=g, deltas=deltas, transform=spec)
    if isinstance(norm, pk.OnlineCmvnSpec):
        fs.set_norm(norm, glob)
    elif norm is not None:
        fs.set_norm(norm)
    if spk is not None:
        fs.set_speaker_stats(spk)
    fs.set_features(raw, "raw")
    if mats is not None:
        fs.set_utt_transforms(mats)
    fs.score(0.1)
    rows = fetch_rows(fs)
    recs = None
    if stats:
        fs.set_norm(pk.NormSpec("utterance", True, True))
        fs.set_features(raw, "raw")
        fs.score(0.1)
        recs = [fs.norm_stats(u) for u in range(len(raw))]
    fs.close()
    return rows, recs


def slot_matrix(D, affine=True, seed=40):
    """The identity plus N(0, 0.1): a speaker's matrix."""
    m = (np.random.default_rng(seed).standard_normal((D, D + (1 if affine else 0))) * 0.1).astype(np.float32)
    m[:, :D] += np.eye(D, dtype=np.float32)
    return m


# ---------------------------------------------------------------- every shape, chunking and close

def run_cell(Dp, Lt, Rt, rows, affine, L, R, softmax, rng, ts=None, passes=(0, 1)):
    spec = pk.TransformSpec(TC.matrix(Dp, Lt, Rt, rows, affine), Lt, Rt, in_dim=Dp)
    am, _, _ = tiny(rows, L, R, softmax=softmax)
    ts = ST.lengths(0, Lt, Rt, R, G) if ts is None else ts
    raw = [NC.features(T, Dp, 7 + u) if u % 2 else TC.wide(T, Dp, 7 + u) for u, T in enumerate(ts)]
    want, _ = batch_rows(am, spec, raw, pk.NormSpec("none"))
    sc = pk.OnlineFeatureScorer.with_transform(am, len(ts), sum(ts) + 1, spec)
    assert (sc.in_dim(), sc.base_dim(), sc.feat_dim()) == (Dp, Dp, rows)
    sc.set_norm(pk.NormSpec("none"))
    for shift in passes:                                # every length meets two chunkings and two ways to close
        jobs = [dict(slot=u, kind="raw", data=x, chunks=ST.chunks_of(x.shape[0], ST.CHUNKINGS[(u + Lt + 2 * shift) % 4], rng),
                     start=(3 * u + shift) % 5, close_delay=(u + Rt + shift) % 3) for u, x in enumerate(raw)]
        got = ST.run_jobs(sc, jobs)
        for u, (r, _) in enumerate(got):
            assert r.shape[0] == ts[u], (Dp, Lt, Rt, rows, L, R, ts[u], r.shape)
            assert rows_equal(r, want[u]), "in_dim=%d (%d,%d) -> %d %s L=%d R=%d T=%d chunks %s delay %d: rows differ" % (
                Dp, Lt, Rt, rows, "affine" if affine else "linear", L, R, ts[u], jobs[u]["chunks"][:6], jobs[u]["close_delay"])
    sc.destroy()
    am.close()


@pytest.mark.parametrize("Dp", IN_DIMS)
def test_every_shape_chunking_and_close_is_the_batch_scorer(Dp):
    i = IN_DIMS.index(Dp)
    rng = np.random.default_rng(100 + Dp)
    for k, (Lt, Rt) in enumerate(SPLICES):
        r, affine, c, sm = cell(i, k)
        run_cell(Dp, Lt, Rt, ROWS[r], bool(affine), CONTEXTS[c][0], CONTEXTS[c][1], ("stable", "reference")[sm], rng)


def test_the_widest_spec_fills_the_lds():
    """in_dim 512, C = 16: (G + C) x 512 floats are exactly 64 KiB."""
    assert 4 * (G + 16) * 512 == 65536
    run_cell(512, 8, 8, 1, True, 2, 1, "stable", np.random.default_rng(5), ts=[0, 1, 9, 17, G + 1, 40], passes=(0,))


def test_the_cells_cover_every_pair():
    cells = [(i, k) + cell(i, k) for i in range(5) for k in range(5)]
    sizes = (5, 5, 5, 2, 3, 2)
    for x in range(6):
        for y in range(x + 1, 6):
            assert len({(c[x], c[y]) for c in cells}) == sizes[x] * sizes[y], (x, y)


def test_rows_arrive_with_a_lookahead_of_rt_plus_r():
    Dp, Lt, Rt, D, L, R = 13, 3, 3, 40, 2, 1
    spec = pk.TransformSpec(TC.matrix(Dp, Lt, Rt, D, True), Lt, Rt)
    am, _, _ = tiny(D, L, R)
    x = NC.features(40, Dp, 3)
    want, _ = batch_rows(am, spec, [x], pk.NormSpec("none"))
    sc = pk.OnlineFeatureScorer.with_transform(am, 2, 64, spec)
    sc.set_norm(pk.NormSpec("none"))
    sc.open_features(0, "raw")
    n = nx = a = 0
    rows = []
    for c in (3, 2, 1, 0, 10, 24):
        sc.push_features(0, x[n:n + c])
        sc.step(0.1)
        n += c
        nx, b = ST.advance(n, nx, a, Rt, R, False)
        first, r = sc.fetch(0)
        assert r.shape[0] == b - a == max(n - Rt - R, 0) - a and (first == a or b == a), (n, a, b, first, r.shape)
        rows.append(r)
        a = b
    sc.close(0)
    sc.step(0.1)                                        # the flush: Rt + R frames from history alone
    first, r = sc.fetch(0)
    assert (first, r.shape[0]) == (40 - Rt - R, Rt + R)
    assert NC.bits_equal(np.concatenate(rows + [r]), want[0])
    # closed with n = 0: nothing; closed with n <= Rt + R: everything at the flush
    sc.open_features(0, "raw")
    sc.open_features(1, "raw")
    sc.push_features(1, x[:Rt + R])
    sc.step(0.1)
    assert sc.fetch(1)[1].shape[0] == 0
    sc.close(0)
    sc.close(1)
    sc.step(0.1)
    assert sc.fetch(0)[1].shape[0] == 0
    first, r = sc.fetch(1)
    y, _ = batch_rows(am, spec, [x[:Rt + R]], pk.NormSpec("none"))
    assert first == 0 and NC.bits_equal(r, y[0])
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- deltas in front

def test_deltas_in_front_of_the_transform():
    """13 -> 39 -> +-3 -> 40, lengths around M + Rt + R."""
    Db, Lt, Rt, D, L, R = 13, 3, 3, 40, 2, 1
    deltas, M = pk.DeltaSpec(2, 2), 4
    spec = pk.TransformSpec(TC.matrix(3 * Db, Lt, Rt, D, True), Lt, Rt)
    am, _, _ = tiny(D, L, R)
    ts = ST.lengths(M, Lt, Rt, R, G)
    raw = [NC.features(T, Db, 17 + u) for u, T in enumerate(ts)]
    mats = [slot_matrix(D, True, 50 + u) for u in range(len(ts))]
    want, _ = batch_rows(am, spec, raw, pk.NormSpec("none"), deltas=deltas)
    want_m, _ = batch_rows(am, spec, raw, pk.NormSpec("none"), deltas=deltas, mats=mats)
    sc = pk.OnlineFeatureScorer.with_transform(am, len(ts), sum(ts) + 1, spec, deltas=deltas)
    assert (sc.in_dim(), sc.base_dim(), sc.feat_dim()) == (3 * Db, Db, D)
    sc.set_norm(pk.NormSpec("none"))
    rng = np.random.default_rng(4)
    for shift in (0, 1):
        jobs = [dict(slot=u, kind="raw", data=x, chunks=ST.chunks_of(x.shape[0], ST.CHUNKINGS[(u + shift) % 4], rng), start=(2 * u + shift) % 5,
                     close_delay=(u + shift) % 3) for u, x in enumerate(raw)]
        for u, (r, _) in enumerate(ST.run_jobs(sc, jobs)):
            assert rows_equal(r, want[u]), "T=%d pass %d chunks %s: rows differ" % (ts[u], shift, jobs[u]["chunks"][:6])
    # the same with every second slot's own (affine) matrix: those slots against the batch with per-utterance matrices
    jobs = [dict(slot=u, kind="raw", data=x, chunks=ST.chunks_of(x.shape[0], ST.CHUNKINGS[(u + 1) % 4], rng), start=u % 4, close_delay=u % 3,
                 mat=mats[u] if u % 2 == 0 else None) for u, x in enumerate(raw)]
    for u, (r, _) in enumerate(ST.run_jobs(sc, jobs)):
        assert rows_equal(r, (want_m if u % 2 == 0 else want)[u]), "T=%d slot matrix %s: rows differ" % (ts[u], u % 2 == 0)
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- every norm mode in front of the transform

NORMS = [("none", 13), ("speaker", 65), ("online", 13), ("sliding", 40), ("sliding", 41)]


@pytest.mark.parametrize("mode, Db", NORMS, ids=["%s-%d" % n for n in NORMS])
def test_every_norm_mode_in_front_of_the_transform(mode, Db):
    Lt, Rt, D, L, R = 3, 3, 40, 2, 1
    spec = pk.TransformSpec(TC.matrix(Db, Lt, Rt, D, True), Lt, Rt, in_dim=Db)
    frames = [0, 5, 130, 1, 33, 650]
    raw = [CA.features(T, Db, 30 + u) for u, T in enumerate(frames)]
    g = CA.stats_for(Db) if mode == "sliding" else None
    rec = [NC.accumulate(x) for x in raw]
    spk = [r + rec[2] for r in rec] if mode in ("speaker", "online") else None
    norm = {"none": pk.NormSpec("none"), "speaker": pk.NormSpec("speaker", True, True), "online": pk.OnlineCmvnSpec(8, 600, 0, True),
            "sliding": None}[mode]
    am, _, _ = tiny(D, L, R)
    records = mode in ("speaker", "online")
    want, recs = batch_rows(am, spec, raw, norm, g=g, spk=spk, stats=records)
    sc = pk.OnlineFeatureScorer.with_transform(am, len(raw), 700, spec, global_stats=g)
    if norm is not None:
        sc.set_norm(norm)
    rng = np.random.default_rng(5)
    jobs = [dict(slot=u, kind="raw", data=x, chunks=ST.chunks_of(x.shape[0], ("random", 7, "whole", 1)[u % 4], rng), start=u % 3,
                 close_delay=u % 3, spk=None if spk is None else spk[u], stats=records) for u, x in enumerate(raw)]
    for u, (rows, st) in enumerate(ST.run_jobs(sc, jobs)):
        assert rows_equal(rows, want[u]), "%s Db=%d utterance %d (%d frames): rows differ" % (mode, Db, u, frames[u])
        if records:
            assert st.shape == (2, Db + 1) and NC.bits_equal(st, recs[u]) and NC.bits_equal(st, rec[u]), (mode, u)
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- audio

def test_audio_through_an_mfcc_front_end_and_mixed_slots():
    fe = FA.SPECS[9]                                    # 13 of 23 MFCC
    Db, Lt, Rt, D, L, R = fe.dim, 3, 3, 40, 2, 1
    spec = pk.TransformSpec(TC.matrix(Db, Lt, Rt, D, True), Lt, Rt)
    am, _, _ = tiny(D, L, R)
    g = np.concatenate([np.full(Db, 10.0 * 2500.0), [2500.0]]).astype(np.float32)
    sizes = (399, 1237, 0, 14321, 159, 5000, 9000)
    rates = [16000, 16000, 16000, 16000, 8000, 8000, 16000]
    waves = [FA.wave_i16(n, 50 + u).astype(np.float32) for u, n in enumerate(sizes)]
    cap = 4 * sum(sizes)
    bs = pk.BatchScorer(am, g, len(waves), cap, frontend=fe, transform=spec)
    bs.set_waves(waves, rates)
    bs.score(0.1)
    want = fetch_rows(bs)
    base = [bs.fetch_fbank(u) for u in range(len(waves))]
    cmvn = [bs.fetch_cmvn(u) for u in range(len(waves))]
    bs.close()
    assert want[3].shape[0] == pk.num_frames(sizes[3]) and want[5].shape[0] > 0
    sc = pk.OnlineScorer.with_transform(am, g, len(waves) + 2, cap, spec, frontend=fe)
    assert (sc.in_dim(), sc.base_dim(), sc.feat_dim()) == (Db, Db, D)
    rng = np.random.default_rng(9)

    def wave_chunks(u, how):
        n = waves[u].size
        if how == "100ms":
            c = rates[u] // 10
            return [c] * (n // c) + ([n % c] if n % c else [])
        out, left = [], n
        while left > 0:
            c = int(min(left, rng.integers(1, 3001)))
            out += [c] + ([0] if rng.random() < 0.3 else [])
            left -= c
        return out

    for shift in (0, 1):
        jobs = [dict(slot=u, kind="audio", data=w, chunks=wave_chunks(u, ("100ms", "odd")[(u + shift) % 2]), rate=rates[u],
                     start=u % 3, close_delay=(u + shift) % 3) for u, w in enumerate(waves)]
        # the same steps: a RAW slot fed wave 3's front-end rows, a NORMALIZED slot fed its rows past the transform
        jobs.append(dict(slot=len(waves), kind="raw", data=base[3], chunks=ST.chunks_of(base[3].shape[0], 7, rng), start=1, close_delay=1))
        jobs.append(dict(slot=len(waves) + 1, kind="normalized", data=cmvn[3], chunks=ST.chunks_of(cmvn[3].shape[0], "random", rng), start=2))
        got = ST.run_jobs(sc, jobs)
        for u in range(len(waves)):
            assert rows_equal(got[u][0], want[u]), "wave %d (%d samples at %d Hz) pass %d: rows differ" % (u, sizes[u], rates[u], shift)
        assert NC.bits_equal(got[len(waves)][0], want[3]), "RAW slot beside audio"
        assert NC.bits_equal(got[len(waves) + 1][0], want[3]), "NORMALIZED slot beside audio"
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- the global matrix, the slots' own, both

@pytest.mark.parametrize("affine", [True, False], ids=["affine", "linear"])
def test_global_alone_per_slot_alone_both_and_mixed(affine):
    Dp, Lt, Rt, D, L, R = 13, 3, 3, 40, 2, 1
    am, _, _ = tiny(D, L, R)
    frames = [0, 3, G, 1, 2 * G + 1, 7, 33]
    rng = np.random.default_rng(6)
    mats = [slot_matrix(D, affine, 40 + u) for u in range(len(frames))]          # all different: a wrong index shows
    for spec, width in ((pk.TransformSpec(TC.matrix(Dp, Lt, Rt, D, True), Lt, Rt), Dp), (pk.TransformSpec(None, in_dim=D), D)):
        raw = [NC.features(T, width, 80 + u) for u, T in enumerate(frames)]
        raw[4][5, 2], raw[4][6, 0] = -0.0, np.nan        # (a matrix-less slot passes them on; see the module's docstring)
        plain, _ = batch_rows(am, spec, raw, pk.NormSpec("none"))
        own, _ = batch_rows(am, spec, raw, pk.NormSpec("none"), mats=mats)
        neighbour, _ = batch_rows(am, spec, raw, pk.NormSpec("none"), mats=mats[1:] + mats[:1])
        assert not NC.bits_equal(own[2], neighbour[2])
        sc = pk.OnlineFeatureScorer.with_transform(am, len(frames), sum(frames) + 1, spec)
        assert (sc.in_dim(), sc.feat_dim()) == (width, D)
        sc.set_norm(pk.NormSpec("none"))
        # no slot has a matrix; every slot has one; every second one has (the others in the same steps without)
        for which in (lambda u: False, lambda u: True, lambda u: u % 2 == 0, lambda u: u % 2 == 1):
            jobs = [dict(slot=u, kind="raw", data=x, chunks=ST.chunks_of(x.shape[0], ST.CHUNKINGS[u % 4], rng), start=u % 3, close_delay=u % 3,
                         mat=mats[u] if which(u) else None) for u, x in enumerate(raw)]
            for u, (r, _) in enumerate(ST.run_jobs(sc, jobs)):
                w = (own if which(u) else plain)[u]
                assert r.shape[0] == frames[u] and (frames[u] == 0 or TC.same_but_nan(r, w)), (width, u, which(u))
        sc.destroy()
    am.close()


# ---------------------------------------------------------------- isolation, reuse, edge values

def test_poisoned_neighbours_and_a_reopened_slot_change_no_bit():
    Dp, Lt, Rt, D, L, R = 41, 3, 3, 40, 2, 1
    C = Lt + Rt
    spec = pk.TransformSpec(TC.matrix(Dp, Lt, Rt, D, True), Lt, Rt)
    am, _, _ = tiny(D, L, R)
    feats = [NC.features(T, Dp, 60 + u) for u, T in enumerate((130, 9, 64))]
    mats = [slot_matrix(D, True, 70 + u) for u in range(3)]
    want, _ = batch_rows(am, spec, feats, pk.NormSpec("none"), mats=mats)
    rng = np.random.default_rng(2)
    sc = pk.OnlineFeatureScorer.with_transform(am, 5, 400, spec)
    sc.set_norm(pk.NormSpec("none"))
    nan = np.full((200, Dp), np.nan, np.float32)
    big = np.full((90, Dp), 1e30, np.float32)
    jobs = [dict(slot=0, kind="raw", data=feats[0], chunks=ST.chunks_of(130, 7, rng), mat=mats[0]),
            dict(slot=1, kind="raw", data=nan, chunks=ST.chunks_of(200, "random", rng), mat=mats[1]),
            dict(slot=2, kind="raw", data=feats[1], chunks=ST.chunks_of(9, 1, rng), start=2, mat=mats[1]),
            dict(slot=3, kind="raw", data=big, chunks=ST.chunks_of(90, 7, rng), close_delay=2),
            dict(slot=4, kind="raw", data=feats[2], chunks=ST.chunks_of(64, "random", rng), start=1, close_delay=1, mat=mats[2])]
    got = ST.run_jobs(sc, jobs)
    for i, u in ((0, 0), (2, 1), (4, 2)):
        assert NC.bits_equal(got[i][0], want[u]), i
    assert np.isnan(got[1][0]).all() and got[1][0].shape[0] == 200
    # a slot reopened after C + 5 NaN frames, in each parity of its ring: a fresh slot's bits (and its own matrix, not the last one's)
    for pushes in ([C + 5], [3, C + 2], [1, 1, C + 3]):
        jobs = [dict(slot=1, kind="raw", data=nan[:C + 5], chunks=pushes, mat=mats[2]),
                dict(slot=1, kind="raw", data=feats[0], chunks=ST.chunks_of(130, "random", rng), mat=mats[0]),
                dict(slot=1, kind="raw", data=feats[1], chunks=[9], close_delay=1, mat=mats[1])]
        got = ST.run_jobs(sc, jobs)
        assert np.isnan(got[0][0]).all()
        assert NC.bits_equal(got[1][0], want[0]) and NC.bits_equal(got[2][0], want[1]), pushes
    sc.destroy()
    am.close()


def test_nan_inf_at_a_zero_entry_and_minus_zero_across_a_ring_hand_over():
    Dp, Lt, Rt, D, L, R = 65, 3, 3, 40, 0, 0
    m = TC.matrix(Dp, Lt, Rt, D, True)
    m[:, 3 * Dp + 64] = 0.0                              # the centre tap of feature 64: a zero entry times an inf is NaN
    spec = pk.TransformSpec(m, Lt, Rt)
    am, _, _ = tiny(D, L, R)
    x = NC.features(60, Dp, 90)
    x[20, 64], x[21, 7], x[40, 5] = np.inf, -0.0, np.nan
    fs = pk.FeatureScorer(am, 1, 60, transform=spec)
    fs.set_norm(pk.NormSpec("none"))
    fs.set_features([x], "raw")
    fs.score(0.1)
    cm, want = fs.fetch_cmvn(0), fs.fetch(0).log_prob()
    fs.close()
    assert TC.same_but_nan(cm, TC.transform(x, m, Lt, Rt))
    # the inf reaches frames 17 .. 23: NaN where it meets the zero entry (frame 20, its centre tap), +-inf at the other six
    assert np.isnan(cm[20]).all() and np.isinf(cm[17:20]).all() and np.isinf(cm[21:24]).all() and np.isnan(cm[37:44]).all()
    assert np.isfinite(cm[:17]).all() and np.isfinite(cm[24:37]).all() and np.isfinite(cm[44:]).all()
    sc = pk.OnlineFeatureScorer.with_transform(am, 1, 64, spec)
    sc.set_norm(pk.NormSpec("none"))
    # the special frames are pushed last in a step, first in a step, and alone: each crosses the ring on its way to a transform frame
    for chunks in ([21, 1, 38], [20, 2, 18, 20], [19, 1, 1, 1, 17, 1, 1, 19], [60]):
        got = ST.run_jobs(sc, [dict(slot=0, kind="raw", data=x, chunks=chunks, close_delay=1)])[0][0]
        assert TC.same_but_nan(got, want) and (np.isnan(got) == np.isnan(want)).all(), chunks
    sc.destroy()
    am.close()


def test_scorers_of_the_existing_entries_still_give_their_bits():
    D, L, R = 39, 2, 1
    am, _, _ = tiny(D, L, R)
    g = CA.stats_for(D)
    x = CA.features(70, D, 4)
    base = x[:, :13].copy()
    deltas = pk.DeltaSpec(2, 2)
    rng = np.random.default_rng(3)

    def others_run():
        out = []
        for norm in (None, pk.NormSpec("none")):
            sc = pk.OnlineFeatureScorer(am, 2, 100, global_stats=g)
            assert sc.base_dim() == sc.feat_dim() == sc.in_dim() == D
            if norm is not None:
                sc.set_norm(norm)
            jobs = [dict(slot=0, kind="raw", data=x, chunks=SD.chunks_of(70, 7, rng)),
                    dict(slot=1, kind="normalized", data=x, chunks=SD.chunks_of(70, 1, rng), close_delay=1)]
            out += [r for r, _ in SD.run_jobs(sc, jobs)]
            assert code_of(lambda: sc.set_slot_transform(0, np.eye(D, dtype=np.float32)))[0] == E_STATE      # a stream of another entry
            sc.destroy()
        sc = pk.OnlineFeatureScorer(am, 1, 100, deltas=deltas)                # the same 39-dim model as 13 + deltas
        assert (sc.in_dim(), sc.base_dim()) == (D, 13)
        sc.set_norm(pk.NormSpec("none"))
        out.append(SD.run_jobs(sc, [dict(slot=0, kind="raw", data=base, chunks=SD.chunks_of(70, 7, rng))])[0][0])
        sc.destroy()
        return out

    before = others_run()
    fs = pk.FeatureScorer(am, 1, 70, global_stats=g)
    fs.set_features([x], "raw")
    fs.score(0.1)
    assert NC.bits_equal(before[0], fs.fetch(0).log_prob())
    fs.close()
    spec = pk.TransformSpec(TC.matrix(13, 3, 3, D, True), 3, 3)
    sc = pk.OnlineFeatureScorer.with_transform(am, 1, 100, spec)
    sc.set_norm(pk.NormSpec("none"))
    got = ST.run_jobs(sc, [dict(slot=0, kind="raw", data=base, chunks=ST.chunks_of(70, 7, rng), mat=slot_matrix(D))])[0][0]
    assert NC.bits_equal(got, batch_rows(am, spec, [base], pk.NormSpec("none"), mats=[slot_matrix(D)])[0][0])
    sc.destroy()
    after = others_run()
    assert all(NC.bits_equal(a, b) for a, b in zip(before, after))
    am.close()


# ---------------------------------------------------------------- failure codes

def test_failure_codes_and_the_same_healthy_job_afterwards():
    Db, Lt, Rt, D, L, R = 13, 3, 3, 40, 2, 1
    m = TC.matrix(Db, Lt, Rt, D, True)
    spec = pk.TransformSpec(m, Lt, Rt)
    am, _, _ = tiny(D, L, R)
    g = CA.stats_for(Db)
    x = CA.features(50, Db, 8)
    own = slot_matrix(D)
    want, _ = batch_rows(am, spec, [x], None, g=g, mats=[own])
    lib = pk.lib()

    def healthy(sc):
        got = ST.run_jobs(sc, [dict(slot=0, kind="raw", data=x, chunks=[20, 0, 30], close_delay=1, mat=own)])[0][0]
        assert NC.bits_equal(got, want[0])

    sc = pk.OnlineFeatureScorer.with_transform(am, 2, 60, spec, global_stats=g)
    healthy(sc)
    # a slot's own matrix: its shape, its entries, the slot's state and kind
    assert code_of(lambda: sc.set_slot_transform(0, own))[0] == E_STATE                     # not open
    sc.open_features(0, "raw")
    sc.open_features(1, "normalized")
    code, text = code_of(lambda: sc.set_slot_transform(0, np.zeros((39, 40), np.float32)))
    assert code == E_INVALID and "39 rows" in text
    code, text = code_of(lambda: sc.set_slot_transform(0, np.zeros((40, 42), np.float32)))
    assert code == E_INVALID and "42 columns" in text
    bad = own.copy()
    bad[3, 7] = np.nan
    code, text = code_of(lambda: sc.set_slot_transform(0, bad))
    assert code == E_INVALID and "row 3, column 7" in text
    assert code_of(lambda: sc.set_slot_transform(1, own))[0] == E_STATE                     # NORMALIZED: no transform applies
    assert code_of(lambda: sc.set_slot_transform(2, own))[0] == E_INVALID                   # no such slot
    # widths: RAW at Db, NORMALIZED at feat_dim, in Python and at the entry
    assert code_of(lambda: sc.push_features(0, np.zeros((2, 40), np.float32)))[0] == E_INVALID
    assert code_of(lambda: sc.push_features(1, np.zeros((2, 13), np.float32)))[0] == E_INVALID
    code, text = code_of(lambda: sc.push_features(0, np.zeros((61, 13), np.float32)))
    assert code == E_INVALID and "capacity" in text
    sc.push_features(0, x[:3])
    sc.step(0.1)                                         # three input frames: no transform frame yet, the matrix may still come
    assert sc.fetch(0)[1].shape[0] == 0
    sc.set_slot_transform(0, own)
    sc.push_features(0, x[3:30])
    assert code_of(lambda: sc.open(1))[0] == E_STATE                                        # audio on a features-only object
    sc.close(1)
    sc.step(0.1)
    assert sc.fetch(0)[1].shape[0] == 30 - Rt - R
    code, text = code_of(lambda: sc.set_slot_transform(0, own))                             # after the first transform frame
    assert code == E_STATE and "first transform frame" in text
    assert code_of(lambda: sc.set_norm(pk.NormSpec("none")))[0] == E_STATE
    sc.push_features(0, x[30:])
    sc.close(0)
    sc.step(0.1)
    first, r = sc.fetch(0)
    assert first == 30 - Rt - R and NC.bits_equal(r, want[0][first:])
    code, text = code_of(lambda: sc.set_norm(pk.NormSpec("utterance")))
    assert code == E_INVALID and "utterance" in text
    assert code_of(lambda: sc.step(0.1))[0] == E_STATE                                      # no open slot
    healthy(sc)
    sc.destroy()
    # RAW without statistics under the sliding rule
    bare = pk.OnlineFeatureScorer.with_transform(am, 1, 60, spec)
    code, text = code_of(lambda: bare.open_features(0, "raw"))
    assert code == E_INVALID and "statistics" in text
    bare.destroy()
    # the create entry, where it reads the finalized model: the batch entry's refusals, word for word
    fe, wide = FA.SPECS[9], FA.SPECS[1]
    d3, d2 = pk.DeltaSpec(2, 2), pk.DeltaSpec(1, 2)
    to39 = pk.TransformSpec(TC.matrix(Db, Lt, Rt, 39, True), Lt, Rt)
    OF, OS, F, B = pk.OnlineFeatureScorer.with_transform, pk.OnlineScorer.with_transform, pk.FeatureScorer, pk.BatchScorer
    for live, batch in ((lambda: OF(am, 2, 100, spec, deltas=d2), lambda: F(am, 2, 100, deltas=d2, transform=spec)),               # 13 is odd
                        (lambda: OS(am, g, 2, 16000, spec, frontend=wide), lambda: B(am, g, 2, 16000, frontend=wide, transform=spec)),
                        (lambda: OS(am, CA.stats_for(40), 2, 16000, spec, frontend=fe), lambda: B(am, CA.stats_for(40), 2, 16000, frontend=fe, transform=spec)),
                        (lambda: OF(am, 2, 100, spec, global_stats=CA.stats_for(40)), lambda: F(am, 2, 100, global_stats=CA.stats_for(40), transform=spec)),
                        (lambda: OF(am, 2, 100, to39), lambda: F(am, 2, 100, transform=to39)),
                        (lambda: OF(am, 2, 100, spec, deltas=d3), lambda: F(am, 2, 100, deltas=d3, transform=spec)),              # 13 / 3
                        (lambda: OS(am, g, 2, 16000, spec, frontend=pk.FrontendSpec(num_mel_bins=2)),
                         lambda: B(am, g, 2, 16000, frontend=pk.FrontendSpec(num_mel_bins=2), transform=spec))):
        code, text = code_of(live)
        assert (code, text) == code_of(batch) and code == E_INVALID, text
    assert "2 blocks" in code_of(lambda: OF(am, 2, 100, spec, deltas=d2))[1]
    assert "14" in code_of(lambda: OF(am, 2, 100, spec, global_stats=CA.stats_for(40)))[1]
    assert "39" in code_of(lambda: OF(am, 2, 100, to39))[1]
    half, _, _ = tiny(40, L, R, precision="f16x3")          # a finalized f16 model: refused as on every online scorer
    code, text = code_of(lambda: OF(half, 2, 100, spec))
    assert code == E_INVALID and "f32" in text
    half.close()
    for streams, cap in ((0, 100), (2, 0)):
        code, text = code_of(lambda: OF(am, streams, cap, spec))
        assert code == E_INVALID and "capacity" in text
    assert lib.pk_mi355_stream_in_dim(None) == E_INVALID
    # an audio object: a push past the capacity is refused and consumes nothing
    au = OS(am, g, 2, 1600, spec, frontend=fe)
    au.open(0)
    au.set_slot_transform(0, own)
    w = FA.wave_i16(1600, 1).astype(np.float32)
    au.push(0, w)
    code, text = code_of(lambda: au.push(0, w[:1]))
    assert code == E_INVALID and "capacity" in text
    au.close(0)
    au.step(0.1)
    bs = B(am, g, 1, 1600, frontend=fe, transform=spec)
    bs.set_waves([w])
    bs.set_utt_transforms([own])
    bs.score(0.1)
    assert NC.bits_equal(au.fetch(0)[1], bs.fetch(0).log_prob())
    bs.close()
    au.destroy()
    am.close()
