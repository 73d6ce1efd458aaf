"""Delta features on the online scorers: StreamDeltaKernel between the normaliser and
StreamFeatureLayoutKernel of a scorer made with deltas=.  The yardstick everywhere is the batch deltas scorer
(FeatureScorer / BatchScorer with deltas=, itself pinned to tests/delta_cases.py) on the whole input under the same
normalisation; every comparison is bitwise, each step's first_frame continues the last (stream_delta_cases.run_jobs).
  * Every base dimension, spec and context pairwise; slot lengths around M, M + R, 2M + R and the kernel's run of G
    frames, each in a slot of one object, opened at different steps; pushed whole, 1 and 7 frames a step and in seeded
    random pushes with empty ones; closed with the last push, a step later and after two empty steps; both softmax modes.
  * Every norm mode in front of the deltas, with norm_stats(slot) at Db; audio through two front-ends at two rates; audio,
    RAW and NORMALIZED slots in the same steps; NaN and 1e30 neighbours; a reopened slot; inf at a centre tap and -0.0
    across a ring hand-over; an existing-entry scorer in the same process; every failure code.  (The decoder and the
    recognizer behind such a scorer: tests/test_gpu_online_recognizer_deltas.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pocketkaldi_amd as pk

import cmvn_any_cases as CA
import delta_cases as DC
import frontend_any_cases as FA
import norm_cases as NC
import stream_delta_cases as SD
from test_gpu_cmvn_any import fetch_rows, tiny

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
DIMS = [1, 13, 63, 64, 65, 80]
SPECS = [(1, 1), (2, 2), (3, 1), (3, 8)]
CONTEXTS = [(0, 0), (2, 1), (5, 5)]
G = int(re.search(r"kDeltaFrames\s*=\s*(\d+)", open(os.path.join(REPO, "pocketkaldi_amd", "csrc", "pk_delta_kernel.h")).read()).group(1))


def code_of(call):
    with pytest.raises(pk.PkCodeError) as e:
        call()
    return e.value.code, str(e.value)


def rows_equal(got, want):
    """Bit for bit; a frameless input's batch rows have no columns either."""
    return got.shape[0] == 0 if want.shape[0] == 0 else NC.bits_equal(got, want)


def error_text():
    return pk.lib().pk_mi355_last_error().decode()


def batch_rows(am, spec, raw, norm=None, g=None, glob=None, spk=None, stats=False):
    """FeatureScorer(deltas=) on the whole matrices as RAW -> (rows per matrix, norm_stats per matrix or None)."""
    fs = pk.FeatureScorer(am, len(raw), max(sum(x.shape[0] for x in raw), 1), global_stats=g, deltas=spec)
    if isinstance(norm, pk.OnlineCmvnSpec):
        fs.set_norm(norm, glob)
    elif norm is not None:
        fs.set_norm(norm)
    if spk is not None:
        fs.set_speaker_stats(spk)
    fs.set_features(raw, "raw")
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


# ---------------------------------------------------------------- every shape, chunking and close

@pytest.mark.parametrize("Db", DIMS)
def test_every_shape_chunking_and_close_is_the_batch_scorer(Db):
    i = DIMS.index(Db)
    rng = np.random.default_rng(100 + Db)
    # All 24 (Db, spec) cells.  The context is (i + k) mod 3 and the softmax mode (i + k) mod 2: over a Db's four specs and
    # over a spec's six Db the sum takes four and six successive values, so every Db and every spec meets every context and
    # both modes, and i + k covers every residue mod 6, so every context meets both modes (test_the_cells_cover_every_pair).
    for k in range(len(SPECS)):
        order, window = SPECS[k]
        L, R = CONTEXTS[(i + k) % 3]
        spec = pk.DeltaSpec(order, window)
        M = order * window
        am, _, _ = tiny(spec.dim(Db), L, R, softmax=("stable", "reference")[(i + k) % 2])
        ts = SD.lengths(order, window, R, G)
        raw = [NC.features(T, Db, 7 + u) if u % 2 else DC.wide(T, Db, 7 + u) for u, T in enumerate(ts)]
        want, _ = batch_rows(am, spec, raw, pk.NormSpec("none"))
        sc = pk.OnlineFeatureScorer(am, len(ts), sum(ts) + 1, deltas=spec)
        assert (sc.base_dim(), sc.feat_dim()) == (Db, spec.dim(Db))
        sc.set_norm(pk.NormSpec("none"))
        for shift in (0, 1):                            # every length meets two chunkings and two ways to close
            jobs = [dict(slot=u, kind="raw", data=x, chunks=SD.chunks_of(x.shape[0], SD.CHUNKINGS[(u + k + 2 * shift) % 4], rng),
                         start=(3 * u + shift) % 5, close_delay=(u + k + shift) % 3) for u, x in enumerate(raw)]
            got = SD.run_jobs(sc, jobs)
            for u, (rows, _) in enumerate(got):
                assert rows.shape[0] == ts[u], (Db, order, window, L, R, ts[u], rows.shape)
                assert rows_equal(rows, want[u]), "Db=%d (%d,%d) L=%d R=%d T=%d M=%d chunks %s delay %d: rows differ" % (
                    Db, order, window, L, R, ts[u], M, jobs[u]["chunks"][:6], jobs[u]["close_delay"])
        sc.destroy()
        am.close()


def test_the_cells_cover_every_pair():
    cells = [(i, k, (i + k) % 3, (i + k) % 2) for i in range(len(DIMS)) for k in range(len(SPECS))]
    sizes = (len(DIMS), len(SPECS), len(CONTEXTS), 2)
    for x in range(4):
        for y in range(x + 1, 4):
            assert len({(c[x], c[y]) for c in cells}) == sizes[x] * sizes[y], (x, y)


def test_rows_arrive_with_a_lookahead_of_m_plus_r():
    Db, order, window, L, R = 13, 2, 2, 2, 1
    spec, M = pk.DeltaSpec(order, window), 4
    am, _, _ = tiny(spec.dim(Db), L, R)
    x = NC.features(40, Db, 3)
    want, _ = batch_rows(am, spec, [x], pk.NormSpec("none"))
    sc = pk.OnlineFeatureScorer(am, 2, 64, deltas=spec)
    sc.set_norm(pk.NormSpec("none"))
    sc.open_features(0, "raw")
    n = nd = a = 0
    rows = []
    for c in (3, 2, 1, 0, 10, 24):
        sc.push_features(0, x[n:n + c])
        sc.step(0.1)
        n += c
        nd, b = SD.advance(n, nd, a, M, R, False)
        first, r = sc.fetch(0)
        assert r.shape[0] == b - a == max(n - M - R, 0) - a and (first == a or b == a), (n, a, b, first, r.shape)
        rows.append(r)
        a = b
    sc.close(0)
    sc.step(0.1)                                        # the flush: M + R frames from history alone
    first, r = sc.fetch(0)
    assert (first, r.shape[0]) == (40 - M - R, M + R)
    assert NC.bits_equal(np.concatenate(rows + [r]), want[0])
    # closed with n = 0: nothing; closed with n <= M + R: everything at the flush
    sc.open_features(0, "raw")
    sc.open_features(1, "raw")
    sc.push_features(1, x[:M + R])
    sc.step(0.1)
    assert sc.fetch(1)[1].shape[0] == 0
    sc.close(0)
    sc.close(1)
    sc.step(0.1)
    assert sc.fetch(0)[1].shape[0] == 0
    first, r = sc.fetch(1)
    y, _ = batch_rows(am, spec, [x[:M + R]], pk.NormSpec("none"))
    assert first == 0 and NC.bits_equal(r, y[0])
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- every norm mode in front of the deltas

NORMS = [("none", 13), ("speaker", 65), ("online", 13), ("sliding", 40), ("sliding", 41)]


@pytest.mark.parametrize("mode, Db", NORMS, ids=["%s-%d" % n for n in NORMS])
def test_every_norm_mode_in_front_of_the_deltas(mode, Db):
    order, window, L, R = 2, 2, 2, 1
    spec = pk.DeltaSpec(order, window)
    frames = [0, 5, 130, 1, 33, 650]
    raw = [CA.features(T, Db, 30 + u) for u, T in enumerate(frames)]
    g = CA.stats_for(Db) if mode == "sliding" else None
    rec = [NC.accumulate(x) for x in raw]
    spk = [r + rec[2] for r in rec] if mode in ("speaker", "online") else None
    norm = {"none": pk.NormSpec("none"), "speaker": pk.NormSpec("speaker", True, True), "online": pk.OnlineCmvnSpec(8, 600, 0, True),
            "sliding": None}[mode]
    am, _, _ = tiny(spec.dim(Db), L, R)
    records = mode in ("speaker", "online")
    want, recs = batch_rows(am, spec, raw, norm, g=g, spk=spk, stats=records)
    sc = pk.OnlineFeatureScorer(am, len(raw), 700, global_stats=g, deltas=spec)
    if norm is not None:
        sc.set_norm(norm)
    rng = np.random.default_rng(5)
    jobs = [dict(slot=u, kind="raw", data=x, chunks=SD.chunks_of(x.shape[0], ("random", 7, "whole", 1)[u % 4], rng), start=u % 3,
                 close_delay=u % 3, spk=None if spk is None else spk[u], stats=records) for u, x in enumerate(raw)]
    for u, (rows, st) in enumerate(SD.run_jobs(sc, jobs)):
        assert rows_equal(rows, want[u]), "%s Db=%d utterance %d (%d frames): rows differ" % (mode, Db, u, frames[u])
        if records:
            assert st.shape == (2, Db + 1) and NC.bits_equal(st, recs[u]) and NC.bits_equal(st, rec[u]), (mode, u)
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- audio

AUDIO = [("mfcc13of23", FA.SPECS[9]), ("fbank80", FA.SPECS[1])]


@pytest.mark.parametrize("name, fe", AUDIO, ids=[a[0] for a in AUDIO])
def test_audio_through_a_front_end_and_mixed_slots(name, fe):
    Db = fe.dim
    spec = pk.DeltaSpec()
    L, R = 2, 1
    am, _, _ = tiny(spec.dim(Db), L, R)
    g = np.concatenate([np.full(Db, 10.0 * 2500.0), [2500.0]]).astype(np.float32)
    sizes = (399, 1237, 0, 14321, 159, 5000, 9000)
    rates = [16000, 16000, 16000, 16000, 8000, 8000, 16000]
    waves = [FA.wave_i16(n, 50 + u).astype(np.float32) for u, n in enumerate(sizes)]
    cap = 4 * sum(sizes)
    bs = pk.BatchScorer(am, g, len(waves), cap, frontend=fe, deltas=spec)
    bs.set_waves(waves, rates)
    bs.score(0.1)
    want = fetch_rows(bs)
    base = [bs.fetch_fbank(u) for u in range(len(waves))]
    cmvn = [bs.fetch_cmvn(u) for u in range(len(waves))]
    bs.close()
    assert want[3].shape[0] == pk.num_frames(sizes[3]) and want[5].shape[0] > 0
    sc = pk.OnlineScorer(am, g, len(waves) + 2, cap, frontend=fe, deltas=spec)
    assert (sc.base_dim(), sc.feat_dim()) == (Db, 3 * Db)
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
        # the same steps: a RAW slot fed wave 3's front-end rows, a NORMALIZED slot fed its rows past the deltas
        jobs.append(dict(slot=len(waves), kind="raw", data=base[3], chunks=SD.chunks_of(base[3].shape[0], 7, rng), start=1, close_delay=1))
        jobs.append(dict(slot=len(waves) + 1, kind="normalized", data=cmvn[3], chunks=SD.chunks_of(cmvn[3].shape[0], "random", rng), start=2))
        got = SD.run_jobs(sc, jobs)
        for u in range(len(waves)):
            assert rows_equal(got[u][0], want[u]), "%s wave %d (%d samples at %d Hz) pass %d: rows differ" % (name, u, sizes[u], rates[u], shift)
        assert NC.bits_equal(got[len(waves)][0], want[3]), "%s: RAW slot beside audio" % name
        assert NC.bits_equal(got[len(waves) + 1][0], want[3]), "%s: NORMALIZED slot beside audio" % name
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- isolation, reuse, edge values

def test_poisoned_neighbours_and_a_reopened_slot_change_no_bit():
    Db, order, window, L, R = 41, 2, 2, 2, 1
    spec, M = pk.DeltaSpec(order, window), 4
    am, _, _ = tiny(spec.dim(Db), L, R)
    feats = [NC.features(T, Db, 60 + u) for u, T in enumerate((130, 9, 64))]
    want, _ = batch_rows(am, spec, feats, pk.NormSpec("none"))
    rng = np.random.default_rng(2)
    sc = pk.OnlineFeatureScorer(am, 5, 400, deltas=spec)
    sc.set_norm(pk.NormSpec("none"))
    nan = np.full((200, Db), np.nan, np.float32)
    big = np.full((90, Db), 1e30, np.float32)
    jobs = [dict(slot=0, kind="raw", data=feats[0], chunks=SD.chunks_of(130, 7, rng)),
            dict(slot=1, kind="raw", data=nan, chunks=SD.chunks_of(200, "random", rng)),
            dict(slot=2, kind="raw", data=feats[1], chunks=SD.chunks_of(9, 1, rng), start=2),
            dict(slot=3, kind="raw", data=big, chunks=SD.chunks_of(90, 7, rng), close_delay=2),
            dict(slot=4, kind="raw", data=feats[2], chunks=SD.chunks_of(64, "random", rng), start=1, close_delay=1)]
    got = SD.run_jobs(sc, jobs)
    for i, u in ((0, 0), (2, 1), (4, 2)):
        assert NC.bits_equal(got[i][0], want[u]), i
    assert np.isnan(got[1][0]).all() and got[1][0].shape[0] == 200
    # a slot reopened after 2 M + 5 NaN frames, in each parity of its ring: a fresh slot's bits
    for pushes in ([2 * M + 5], [3, 2 * M + 2], [1, 1, 2 * M + 3]):
        jobs = [dict(slot=1, kind="raw", data=nan[:2 * M + 5], chunks=pushes),
                dict(slot=1, kind="raw", data=feats[0], chunks=SD.chunks_of(130, "random", rng)),
                dict(slot=1, kind="raw", data=feats[1], chunks=[9], close_delay=1)]
        got = SD.run_jobs(sc, jobs)
        assert np.isnan(got[0][0]).all()
        assert NC.bits_equal(got[1][0], want[0]) and NC.bits_equal(got[2][0], want[1]), pushes
    sc.destroy()
    am.close()


def test_inf_at_a_centre_tap_and_minus_zero_across_a_ring_hand_over():
    Db, order, window, L, R = 65, 2, 2, 0, 0
    spec, M = pk.DeltaSpec(order, window), 4
    am, _, _ = tiny(spec.dim(Db), L, R)
    x = NC.features(60, Db, 90)
    x[20, 64], x[21, 7], x[40, 5] = np.inf, -0.0, np.nan
    # the batch scorer's first-layer input says what the rule gives; the live rows are held to the batch rows
    fs = pk.FeatureScorer(am, 1, 60, deltas=spec)
    fs.set_norm(pk.NormSpec("none"))
    fs.set_features([x], "raw")
    fs.score(0.1)
    cm, want = fs.fetch_cmvn(0), fs.fetch(0).log_prob()
    fs.close()
    assert DC.same_but_nan(cm, DC.add_deltas(x, order, window))
    assert cm[20, 64] == np.inf and not np.isnan(cm[20, Db + 64]) and cm[21, 7].tobytes() == np.float32(0.0).tobytes()
    sc = pk.OnlineFeatureScorer(am, 1, 64, deltas=spec)
    sc.set_norm(pk.NormSpec("none"))
    # the special frames are pushed last in a step, first in a step, and alone: each crosses the ring on its way to a delta frame
    for chunks in ([21, 1, 38], [20, 2, 18, 20], [19, 1, 1, 1, 17, 1, 1, 19], [60]):
        got = SD.run_jobs(sc, [dict(slot=0, kind="raw", data=x, chunks=chunks, close_delay=1)])[0][0]
        assert DC.same_but_nan(got, want) and (np.isnan(got) == np.isnan(want)).all(), chunks
    sc.destroy()
    am.close()


def test_an_existing_entry_scorer_still_gives_its_bits():
    D, L, R = 39, 2, 1
    am, _, _ = tiny(D, L, R)
    g = CA.stats_for(D)
    x = CA.features(70, D, 4)
    rng = np.random.default_rng(3)

    def plain_run():
        out = []
        for norm in (None, pk.NormSpec("none")):
            sc = pk.OnlineFeatureScorer(am, 2, 100, global_stats=g)
            assert sc.base_dim() == sc.feat_dim() == D
            if norm is not None:
                sc.set_norm(norm)
            jobs = [dict(slot=0, kind="raw", data=x, chunks=SD.chunks_of(70, 7, rng)),
                    dict(slot=1, kind="normalized", data=x, chunks=SD.chunks_of(70, 1, rng), close_delay=1)]
            out += [r for r, _ in SD.run_jobs(sc, jobs)]
            sc.destroy()
        return out

    before = plain_run()
    fs = pk.FeatureScorer(am, 1, 70, global_stats=g)
    fs.set_features([x], "raw")
    fs.score(0.1)
    assert NC.bits_equal(before[0], fs.fetch(0).log_prob())
    fs.close()
    spec = pk.DeltaSpec(2, 2)
    sc = pk.OnlineFeatureScorer(am, 1, 100, deltas=spec)                      # the same 39-dim model as 13 + deltas
    sc.set_norm(pk.NormSpec("none"))
    base = x[:, :13].copy()
    got = SD.run_jobs(sc, [dict(slot=0, kind="raw", data=base, chunks=SD.chunks_of(70, 7, rng))])[0][0]
    assert NC.bits_equal(got, batch_rows(am, spec, [base], pk.NormSpec("none"))[0][0])
    sc.destroy()
    after = plain_run()
    assert all(NC.bits_equal(a, b) for a, b in zip(before, after))
    am.close()


# ---------------------------------------------------------------- failure codes

def test_failure_codes_and_the_same_healthy_job_afterwards():
    Db, L, R = 13, 2, 1
    spec = pk.DeltaSpec(2, 2)
    M = 4
    am, _, _ = tiny(39, L, R)
    g = CA.stats_for(Db)
    x = CA.features(50, Db, 8)
    want, _ = batch_rows(am, spec, [x], None, g=g)
    lib = pk.lib()

    def healthy(sc):
        got = SD.run_jobs(sc, [dict(slot=0, kind="raw", data=x, chunks=[20, 0, 30], close_delay=1)])[0][0]
        assert NC.bits_equal(got, want[0])

    sc = pk.OnlineFeatureScorer(am, 2, 60, global_stats=g, deltas=spec)
    healthy(sc)
    # widths: RAW at Db, NORMALIZED at feat_dim, in Python and at the entry
    sc.open_features(0, "raw")
    sc.open_features(1, "normalized")
    assert code_of(lambda: sc.push_features(0, np.zeros((2, 39), np.float32)))[0] == E_INVALID
    assert code_of(lambda: sc.push_features(1, np.zeros((2, 13), np.float32)))[0] == E_INVALID
    # the step capacity holds for both kinds and a refused push consumes nothing
    code, text = code_of(lambda: sc.push_features(0, np.zeros((61, 13), np.float32)))
    assert code == E_INVALID and "capacity" in text
    sc.push_features(0, x[:30])
    code, text = code_of(lambda: sc.push_features(1, np.zeros((31, 39), np.float32)))
    assert code == E_INVALID and "capacity" in text
    # audio on a features-only object
    assert code_of(lambda: sc.open(1))[0] == E_STATE
    assert code_of(lambda: sc.push(0, np.zeros(160, np.float32)))[0] == E_STATE
    sc.close(1)
    sc.step(0.1)
    assert sc.fetch(0)[1].shape[0] == 30 - M - R
    # utterance mode stays refused, the norm is set while no slot is open, records are at Db
    assert code_of(lambda: sc.set_norm(pk.NormSpec("none")))[0] == E_STATE
    sc.push_features(0, x[30:])
    sc.close(0)
    sc.step(0.1)
    first, r = sc.fetch(0)
    assert first == 30 - M - R and NC.bits_equal(r, want[0][first:])
    code, text = code_of(lambda: sc.set_norm(pk.NormSpec("utterance")))
    assert code == E_INVALID and "utterance" in text
    assert code_of(lambda: sc.norm_stats(0))[0] == E_STATE                       # sliding accumulates none
    sc.set_norm(pk.NormSpec("speaker", True, True))
    sc.open_features(0, "raw")
    assert code_of(lambda: sc.set_speaker_stats(0, np.ones((2, 40))))[0] == E_INVALID
    sc.push_features(0, x[:5])
    code, text = code_of(lambda: sc.step(0.1))
    assert code == E_STATE and "slot 0" in text                                  # no speaker record
    sc.set_speaker_stats(0, NC.accumulate(x))
    sc.close(0)
    sc.step(0.1)
    assert sc.fetch(0)[1].shape[0] == 5 and NC.bits_equal(sc.norm_stats(0), NC.accumulate(x[:5]))
    assert code_of(lambda: sc.set_norm(pk.OnlineCmvnSpec(8, 600, 200, False), np.ones((2, 40))))[0] == E_INVALID
    sc.set_norm(pk.NormSpec())
    assert code_of(lambda: sc.step(0.1))[0] == E_STATE                           # no open slot
    healthy(sc)
    sc.destroy()
    # RAW without statistics under the sliding rule
    bare = pk.OnlineFeatureScorer(am, 1, 60, deltas=spec)
    code, text = code_of(lambda: bare.open_features(0, "raw"))
    assert code == E_INVALID and "statistics" in text
    bare.destroy()
    # the create entry, where it reads the finalized model: the batch entry's refusals, word for word
    fe, wide = FA.SPECS[9], FA.SPECS[1]
    for live, batch in ((lambda: pk.OnlineFeatureScorer(am, 2, 100, deltas=pk.DeltaSpec(1, 2)), lambda: pk.FeatureScorer(am, 2, 100, deltas=pk.DeltaSpec(1, 2))),
                        (lambda: pk.OnlineScorer(am, g, 2, 16000, frontend=wide, deltas=spec), lambda: pk.BatchScorer(am, g, 2, 16000, frontend=wide, deltas=spec)),
                        (lambda: pk.OnlineScorer(am, CA.stats_for(39), 2, 16000, frontend=fe, deltas=spec),
                         lambda: pk.BatchScorer(am, CA.stats_for(39), 2, 16000, frontend=fe, deltas=spec)),
                        (lambda: pk.OnlineFeatureScorer(am, 2, 100, global_stats=CA.stats_for(39), deltas=spec),
                         lambda: pk.FeatureScorer(am, 2, 100, global_stats=CA.stats_for(39), deltas=spec)),
                        (lambda: pk.OnlineScorer(am, g, 2, 16000, frontend=pk.FrontendSpec(num_mel_bins=2), deltas=spec),
                         lambda: pk.BatchScorer(am, g, 2, 16000, frontend=pk.FrontendSpec(num_mel_bins=2), deltas=spec))):
        code, text = code_of(live)
        assert (code, text) == code_of(batch) and code == E_INVALID, text
    assert "2 blocks" in code_of(lambda: pk.OnlineFeatureScorer(am, 2, 100, deltas=pk.DeltaSpec(1, 2)))[1]
    assert "14" in code_of(lambda: pk.OnlineFeatureScorer(am, 2, 100, global_stats=CA.stats_for(39), deltas=spec))[1]
    half, _, _ = tiny(40, L, R, precision="f16x3")          # a finalized f16 model: refused as on every online scorer
    code, text = code_of(lambda: pk.OnlineFeatureScorer(half, 2, 100, deltas=pk.DeltaSpec(1, 2)))
    assert code == E_INVALID and "f32" in text
    half.close()
    # its capacities
    for streams, cap in ((0, 100), (2, 0)):
        code, text = code_of(lambda: pk.OnlineFeatureScorer(am, streams, cap, deltas=spec))
        assert code == E_INVALID and "capacity" in text
    assert lib.pk_mi355_stream_base_dim(None) == E_INVALID
    # an audio object: a step that cannot fit consumes nothing (the pushes are bounded by the capacity it was made with)
    fe = FA.SPECS[9]
    au = pk.OnlineScorer(am, g, 2, 1600, frontend=fe, deltas=spec)
    au.open(0)
    w = FA.wave_i16(1600, 1).astype(np.float32)
    au.push(0, w)
    code, text = code_of(lambda: au.push(0, w[:1]))
    assert code == E_INVALID and "capacity" in text
    au.close(0)
    au.step(0.1)
    bs = pk.BatchScorer(am, g, 1, 1600, frontend=fe, deltas=spec)
    bs.set_waves([w])
    bs.score(0.1)
    assert NC.bits_equal(au.fetch(0)[1], bs.fetch(0).log_prob())
    bs.close()
    au.destroy()
    am.close()
