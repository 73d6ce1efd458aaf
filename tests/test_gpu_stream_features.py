"""Live features at the online scorer: pk.OnlineFeatureScorer, OnlineScorer.open_features /
push_features, OnlineRecognizer.open_features / push_features.
  * A feature slot's rows, step after step, are pk.FeatureScorer's on the whole [T][D] matrix bit for bit, at every
    feature dimension and context StreamFeatureLayoutKernel takes another path for, at every chunking, with the slots
    of one object running out at different steps; each step's first_frame continues where the last step ended.
  * The kernel is a copy, held through the scores: frames of NaN payloads, +-Inf, -0.0 and subnormals pass through a
    history hand-over, and every row whose context holds no non-finite value has the batch scorer's bits (the batch
    layout is a copy by tests/test_gpu_features.py's read-back) next to rows that do hold them.
  * RAW features are the wave's fbank: rows equal the audio OnlineScorer's and BatchScorer's on the wave.
  * Audio, RAW and NORMALIZED slots in one step; poisoned neighbours, reopened slots; every failure code; the online
    decoder and the online recognizer downstream."""
import ctypes as C
import os

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth
from pocketkaldi_amd import synth_graph as SG

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_INVALID, E_STATE = -1, -4
DIMS = [1, 3, 39, 40, 63, 64, 65, 130]
CONTEXTS = [(0, 0), (1, 1), (2, 1), (5, 5), (0, 7), (70, 3)]
# (tests/test_gpu_features.py's) NaN payloads, +-Inf, -0.0, subnormals
SPECIALS = np.array([0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF,
                     0x00400000], np.uint32)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def finite(T, D, seed, sigma=1.0):
    return (np.random.default_rng([0x57F1, seed, T, D]).standard_normal((T, D)) * sigma).astype(np.float32)


def tiny(D=40, L=5, R=5, softmax="stable"):
    layers, prior, _, _ = synth.model("tiny", feat_dim=D, left=L, right=R)
    return pk.AcousticModel(layers, prior, L, R).set_softmax(softmax)


def chunks_of(n, how, rng):
    """Chunk sizes summing to n: "whole", an int (fixed size) or "random" (sizes in [1, 100], empty pushes in between)."""
    if how == "whole":
        return [n]
    if isinstance(how, int):
        return [how] * (n // how) + ([n % how] if n % how else [])
    out, left = [], n
    while left > 0:
        if rng.random() < 0.3:
            out.append(0)
        c = int(min(left, rng.integers(1, 101)))
        out.append(c)
        left -= c
    return out


def run_jobs(sc, jobs, prob_scale=0.1):
    """jobs: dicts {slot, kind ("audio", "normalized", "raw"), data (a wave, or [T][D] frames), chunks, start,
    close_with_last}.  A job opens its slot at step `start` or later (once the slot's earlier job has been flushed),
    pushes one chunk per step and closes with its last chunk or, by default, in the step after it (a step that brings the
    slot no new frames).  -> every job's rows [T][num_pdfs]; each step's rows must continue where the last ones ended."""
    n = len(jobs)
    rows, nxt, state, k, pos, busy, step = [[] for _ in range(n)], [0] * n, ["pending"] * n, [0] * n, [0] * n, {}, 0
    N = sc._am.num_pdfs()
    while any(s != "done" for s in state):
        for i, j in enumerate(jobs):
            audio = j["kind"] == "audio"
            if state[i] == "pending" and step >= j["start"] and j["slot"] not in busy:
                sc.open(j["slot"]) if audio else sc.open_features(j["slot"], j["kind"])
                assert sc.slot_kind(j["slot"]) == (None if audio else j["kind"])
                busy[j["slot"]] = i
                state[i] = "open"
            if state[i] == "open":
                if k[i] < len(j["chunks"]):
                    c = j["chunks"][k[i]]
                    (sc.push if audio else sc.push_features)(j["slot"], j["data"][pos[i]:pos[i] + c])
                    pos[i] += c
                    k[i] += 1
                    if k[i] == len(j["chunks"]) and j.get("close_with_last"):
                        sc.close(j["slot"])
                        state[i] = "closed"
                else:
                    sc.close(j["slot"])
                    state[i] = "closed"
        if any(s in ("open", "closed") for s in state):
            sc.step(prob_scale)
            for i, j in enumerate(jobs):
                if state[i] not in ("open", "closed"):
                    continue
                first, r = sc.fetch(j["slot"])
                if r.shape[0]:
                    assert first == nxt[i], (i, first, nxt[i])
                    rows[i].append(r)
                    nxt[i] += r.shape[0]
                if state[i] == "closed":
                    state[i] = "done"
                    del busy[j["slot"]]
        step += 1
    return [np.concatenate(r) if r else np.zeros((0, N), np.float32) for r in rows]


def feature_rows(am, feats, kind="normalized", g=None):
    """pk.FeatureScorer on the whole matrices: the reference of every feature slot."""
    fs = pk.FeatureScorer(am, len(feats), max(sum(f.shape[0] for f in feats), 1), global_stats=g)
    fs.set_features(feats, kind)
    fs.score(0.1)
    out = [fs.fetch(u).log_prob() for u in range(len(feats))]
    fs.close()
    return out


def wave_stages(am, g, waves):
    """BatchScorer on whole waves -> per wave (fbank, CMVN'd features, rows)."""
    bs = pk.BatchScorer(am, g, len(waves), max(sum(len(w) for w in waves), 1))
    bs.set_waves(waves)
    bs.score(0.1)
    out = [(bs.fetch_fbank(u), bs.fetch_cmvn(u), bs.fetch(u).log_prob()) for u in range(len(waves))]
    bs.close()
    return out


def job(slot, kind, data, chunks="whole", start=0, close_with_last=False, rng=None):
    return {"slot": slot, "kind": kind, "data": data, "chunks": chunks_of(len(data), chunks, rng), "start": start,
            "close_with_last": close_with_last}


def assert_jobs(sc, jobs, want, what):
    got = run_jobs(sc, jobs)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if b.shape[0] == 0:                                  # (an empty reference has no row length either)
            assert a.shape[0] == 0, (what, i, a.shape)
            continue
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        assert bits_equal(a, b), "%s job %d (%s, %d rows): differs from its reference" % (what, i, jobs[i]["kind"], b.shape[0])


# ---------------------------------------------------------------- the layout is a copy, across steps

@pytest.mark.parametrize("D", DIMS)
def test_rows_equal_the_feature_scorer_at_every_chunking(D):
    for k, (L, R) in enumerate(CONTEXTS):
        am = tiny(D, L, R, softmax=("stable", "reference")[k % 2])
        lengths = [0, 1, 2, R, R + 1, L + R + 1, 63, 64, 65, 129, 200]
        feats = [finite(T, D, u) for u, T in enumerate(lengths)]
        want = feature_rows(am, feats)
        assert all(np.isfinite(w).all() for w in want)
        sc = pk.OnlineFeatureScorer(am, len(lengths), sum(lengths))
        assert sc.feat_dim() == D and sc.slot_kind(0) is None
        rng = np.random.default_rng([D, L, R])
        # (how, close in the same step as the last push); without it the close comes a step later, and with R > 0 that
        # step's rows are served from the history alone
        for how, with_last in (("whole", False), ("whole", True), (1, False), (7, True), (7, False), (64, False), ("random", False),
                               ("random", True)):
            jobs = [job(u, "normalized", f, how, int(rng.integers(0, 4)), with_last, rng) for u, f in enumerate(feats)]
            assert_jobs(sc, jobs, want, "D=%d L=%d R=%d %s close_with_last=%s" % (D, L, R, how, with_last))
        sc.destroy()
        am.close()


# ---------------------------------------------------------------- bit patterns, through the scores

@pytest.mark.parametrize("D,L,R,chunk", [(65, 2, 1, 3), (40, 5, 5, 4), (130, 0, 7, 5), (3, 70, 3, 50)])
def test_special_values_pass_through_the_history_unchanged(D, L, R, chunk):
    """Frames that hold NaN payloads and infinities sit between frames that hold -0.0 and subnormals and plain ones,
    pushed `chunk` frames a step, so that every special frame is read from the history by a later step.  A row whose
    context [t - L, t + R] (clamped) holds no non-finite value must have the batch scorer's bits -- a neighbour's NaN
    that leaked into it, or a flushed subnormal, would change them -- and the rows that do hold one are non-finite
    exactly where the batch scorer's are."""
    T = 160
    am = tiny(D, L, R)
    x = finite(T, D, 77).view(np.uint32).copy()
    rng = np.random.default_rng([D, L, R])
    # (in the second half, so that a context of 74 frames leaves clean rows too) ... and the frame the right pad replicates
    hot = sorted(set(int(t) for t in T // 2 + rng.choice(T // 2, size=6, replace=False)) | {T - 1})
    for i, t in enumerate(hot):
        x[t, rng.integers(0, D)] = SPECIALS[i % 6]                   # non-finite
    for i in range(40):
        x[rng.integers(0, T), rng.integers(0, D)] = SPECIALS[6 + i % 4]   # -0.0, subnormals: finite
    x[hot, 0] = SPECIALS[2]
    feats = x.view(np.float32)
    dirty = np.zeros(T, bool)
    bad_frame = ~np.isfinite(feats).all(axis=1)
    for t in range(T):
        ctx = np.clip(np.arange(t - L, t + R + 1), 0, T - 1)
        dirty[t] = bad_frame[ctx].any()
    assert dirty.any() and (~dirty).sum() >= 8
    (want,) = feature_rows(am, [feats])
    sc = pk.OnlineFeatureScorer(am, 2, 2 * T)
    for how in (chunk, "whole"):
        got = run_jobs(sc, [job(1, "normalized", feats, how, 0, False)])[0]
        assert got.shape == want.shape
        assert np.isfinite(want[~dirty]).all()
        assert bits_equal(got[~dirty], want[~dirty]), how
        assert np.array_equal(np.isfinite(got[dirty]), np.isfinite(want[dirty])), how
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- RAW: the wave's fbank

@pytest.fixture(scope="module")
def raw_setup():
    """A 40-dim tiny model (L = R = 5), the statistics, and per wave: fbank, CMVN'd features and the batch scorer's rows
    (computed once)."""
    am = tiny()
    g = synth.global_cmvn_stats()
    hello = pk.read_wav(os.path.join(GOLDEN, "en-us-hello.wav"))
    long_wave = synth.utterance(3000, seconds=14.0)
    waves = {"hello": hello, "one": np.ascontiguousarray(long_wave[:400]), "705": np.ascontiguousarray(long_wave[:400 + 704 * 160]),
             "1307": np.ascontiguousarray(long_wave[:400 + 1306 * 160])}
    stages = dict(zip(waves, wave_stages(am, g, list(waves.values()))))
    assert [stages[k][0].shape[0] for k in waves] == [47, 1, 705, 1307]
    yield am, g, waves, stages
    am.close()


def test_raw_features_equal_the_audio_slot_and_the_batch_scorer(raw_setup):
    am, g, waves, stages = raw_setup
    names = ["hello", "one", "705"]
    fsc = pk.OnlineFeatureScorer(am, 3, 800, global_stats=g)
    osc = pk.OnlineScorer(am, g, 3, 800 * 160)
    audio = run_jobs(osc, [job(u, "audio", waves[k], 1600, u) for u, k in enumerate(names)])
    for u, k in enumerate(names):
        assert bits_equal(audio[u], stages[k][2]), k
    rng = np.random.default_rng(5)
    for sc in (fsc, osc):
        for how, with_last in (("whole", True), (10, False), ("random", False)):
            jobs = [job(u, "raw", stages[k][0], how, int(rng.integers(0, 3)), with_last, rng) for u, k in enumerate(names)]
            assert_jobs(sc, jobs, [stages[k][2] for k in names], "raw %s" % (how,))
    fsc.destroy()
    osc.destroy()


def test_raw_ring_wraps_twice(raw_setup):
    am, g, waves, stages = raw_setup
    fb, _, want = stages["1307"]
    sc = pk.OnlineFeatureScorer(am, 2, 1307, global_stats=g)
    assert_jobs(sc, [job(0, "raw", fb, "whole")], [want], "1307 whole")
    assert_jobs(sc, [job(0, "raw", fb, 10), job(1, "raw", stages["hello"][0], 10, 70)], [want, stages["hello"][2]], "1307 by 10")
    sc.destroy()


# ---------------------------------------------------------------- audio, RAW and NORMALIZED in one step

def test_mixed_step_audio_raw_and_normalized(raw_setup):
    am, g, waves, stages = raw_setup
    norm = finite(150, 40, 9)
    (norm_rows,) = feature_rows(am, [norm])
    cat = pk.read_wav(os.path.join(GOLDEN, "en-us-cat.wav"))
    ((cat_fb, _, cat_rows),) = wave_stages(am, g, [cat])
    sc = pk.OnlineScorer(am, g, 4, 4 * 1600)
    jobs = [job(0, "audio", waves["hello"], 1600, 1), job(1, "raw", cat_fb, 9, 0), job(2, "normalized", norm, 10, 2, True),
            job(3, "normalized", stages["hello"][1], 7, 0), job(1, "audio", cat, 1120, 3), job(0, "normalized", norm[:64], 10, 4),
            job(2, "raw", stages["hello"][0], 10, 5)]
    want = [stages["hello"][2], cat_rows, norm_rows, stages["hello"][2], cat_rows, feature_rows(am, [norm[:64]])[0], stages["hello"][2]]
    assert_jobs(sc, jobs, want, "mixed")
    sc.destroy()


# ---------------------------------------------------------------- isolation and reuse

def test_poisoned_neighbours_and_reopened_slots_change_no_bit(raw_setup):
    am, g, waves, stages = raw_setup
    nan705 = np.full((705, 40), np.nan, np.float32)
    loud = np.full((300, 40), 1e30, np.float32)
    loud[::3] = np.nan
    nan_wave = np.full(705 * 160 + 240, np.nan, np.float32)
    norm = finite(200, 40, 11)
    (norm_rows,) = feature_rows(am, [norm])
    hello_fb, hello_cmvn, hello_rows = stages["hello"]
    sc = pk.OnlineScorer(am, g, 4, 800 * 160)
    # neighbours stream NaN and 1e30 features and NaN audio
    jobs = [job(0, "normalized", loud, 10), job(1, "normalized", norm, 10), job(2, "audio", nan_wave, 1600), job(3, "raw", hello_fb, 10),
            job(0, "raw", loud, 10)]
    got = run_jobs(sc, jobs)
    assert bits_equal(got[1], norm_rows) and bits_equal(got[3], hello_rows)
    # every slot reopened after NaN frames, with the same kind and with the other one; slot 2 held NaN audio
    for slot in range(4):
        assert np.isnan(run_jobs(sc, [job(slot, "normalized", nan705, "whole")])[0]).all()
        assert_jobs(sc, [job(slot, "normalized", norm, 10)], [norm_rows], "reopened normalized %d" % slot)
        assert np.isnan(run_jobs(sc, [job(slot, "raw", nan705, "whole")])[0]).all()
        assert_jobs(sc, [job(slot, "raw", hello_fb, 10)], [hello_rows], "reopened raw %d" % slot)
        assert_jobs(sc, [job(slot, "normalized", hello_cmvn, 3)], [hello_rows], "other kind %d" % slot)
        assert_jobs(sc, [job(slot, "audio", waves["hello"], 1600)], [hello_rows], "audio again %d" % slot)
    sc.destroy()


def test_one_step_brings_625_frames_on_top_of_history():
    for D, L, R in ((65, 70, 3), (40, 5, 5)):
        am = tiny(D, L, R)
        feats = finite(9 + 625 + 30, D, 3)
        (want,) = feature_rows(am, [feats])
        sc = pk.OnlineFeatureScorer(am, 2, 700)
        j = job(1, "normalized", feats)
        j["chunks"] = [9, 625, 30]
        assert_jobs(sc, [j], [want], "625 on history D=%d" % D)
        sc.destroy()
        am.close()


# ---------------------------------------------------------------- failure codes

def code_of(call, *args):
    with pytest.raises(pk.PkCodeError) as e:
        call(*args)
    return e.value.code


def test_every_failure_code_and_the_object_stays_usable(raw_setup):
    am, g, waves, stages = raw_setup
    hello_fb, hello_cmvn, hello_rows = stages["hello"]
    L = pk.lib()
    healthy = lambda sc, kind: assert_jobs(sc, [job(0, kind, hello_fb if kind == "raw" else hello_cmvn, 10)], [hello_rows], kind)
    # create
    am65 = tiny(65, 2, 1)
    assert code_of(pk.OnlineFeatureScorer, am65, 2, 100, g) == E_INVALID             # statistics with feat_dim != 40
    assert "40-dim" in L.pk_mi355_last_error().decode()
    for streams, frames in ((0, 100), (2, 0), (-1, 100), (2, -5)):
        assert code_of(pk.OnlineFeatureScorer, am65, streams, frames) == E_INVALID   # capacity
    assert code_of(pk.OnlineScorer, am65, g, 2, 16000) == E_INVALID                  # the audio object stays 40-dim
    am65.close()
    plain = pk.OnlineFeatureScorer(am, 2, 100)                                       # no statistics
    with_stats = pk.OnlineFeatureScorer(am, 2, 100, global_stats=g)
    audio = pk.OnlineScorer(am, g, 2, 100 * 160)
    x = np.zeros((4, 40), np.float32)
    f32p = C.POINTER(C.c_float)
    for sc in (plain, with_stats, audio):
        assert sc.feat_dim() == 40
        assert L.pk_mi355_stream_open_features(sc._h, 0, 2) == E_INVALID and L.pk_mi355_stream_open_features(sc._h, 0, -1) == E_INVALID
        assert code_of(sc.open_features, 2, "normalized") == E_INVALID and code_of(sc.open_features, -1, "normalized") == E_INVALID
        assert code_of(sc.push_features, 0, x) == E_STATE                            # not open
        if sc is plain:
            assert code_of(sc.open_features, 0, "raw") == E_INVALID                  # RAW without statistics
            assert "statistics" in L.pk_mi355_last_error().decode()
            assert code_of(sc.push_features, 0, x) == E_STATE                        # ... opened nothing
        if sc is not audio:                                                          # no PCM buffers: the audio entries
            assert code_of(sc.open, 0) == E_STATE and code_of(sc.open, 0, 8000) == E_STATE
            assert code_of(sc.push, 0, np.zeros(16, np.float32)) == E_STATE and code_of(sc.push_i16, 0, np.zeros(16, np.int16)) == E_STATE
        sc.open_features(0, "normalized")
        assert code_of(sc.open_features, 0, "normalized") == E_STATE                 # open already
        assert sc.slot_kind(0) == "normalized" and sc.slot_kind(1) is None
        assert L.pk_mi355_stream_push_features(sc._h, 0, x.ctypes.data_as(f32p), -1) == E_INVALID
        assert L.pk_mi355_stream_push_features(sc._h, 0, None, 3) == E_INVALID
        assert L.pk_mi355_stream_push_features(sc._h, 1, x.ctypes.data_as(f32p), 4) == E_STATE
        assert L.pk_mi355_stream_push_features(sc._h, 2, x.ctypes.data_as(f32p), 4) == E_INVALID
        if sc is audio:
            assert code_of(sc.push, 0, np.zeros(16, np.float32)) == E_STATE          # audio into a feature slot
            sc.open(1)
            assert code_of(sc.push_features, 1, x) == E_STATE                        # features into an audio slot
            sc.close(1)
        # over capacity: refused whole, and what was pushed before stays
        sc.push_features(0, hello_cmvn[:40])
        assert code_of(sc.push_features, 0, np.zeros((61, 40), np.float32)) == E_INVALID
        assert "capacity" in L.pk_mi355_last_error().decode()
        sc.push_features(0, hello_cmvn[40:])
        sc.close(0)
        assert code_of(sc.push_features, 0, x) == E_STATE                            # closed, not yet flushed
        assert code_of(sc.open_features, 0, "normalized") == E_STATE
        sc.step(0.1)
        first, rows = sc.fetch(0)
        assert first == 0 and bits_equal(rows, hello_rows)
        healthy(sc, "normalized")
        if sc is not plain:
            healthy(sc, "raw")
        sc.destroy()


# ---------------------------------------------------------------- downstream: the online decoder, the online recognizer

def test_online_decoder_over_a_feature_scorer_equals_decode_batch(tmp_path):
    D, Lc, Rc = 65, 2, 1
    am = tiny(D, Lc, Rc)
    graph = SG.word_loop(30, 8, seed=3)
    assert graph["num_tids"] <= am.num_pdfs()
    path = str(tmp_path / "loop.fst")
    SG.write_fst(path, graph["start"], graph["final"], graph["arcs"])
    fst = pk.Fst(path)
    feats = [finite(T, D, 40 + u, sigma=3.0) for u, T in enumerate((120, 1, 0, 75, 200, 33))]
    n = len(feats)
    fs = pk.FeatureScorer(am, n, sum(f.shape[0] for f in feats))
    fs.set_features(feats)
    fs.score(0.1)
    whole = pk.Decoder(fst, am, n)
    whole.decode_batch(fs)
    want = [whole.result(u) for u in range(n)]
    sc = pk.OnlineFeatureScorer(am, n, n * 10)
    dec = pk.OnlineDecoder(fst, am, n)
    pos, state, got, step = [0] * n, ["pending"] * n, [None] * n, 0
    while any(s != "done" for s in state):
        for u in range(n):
            if state[u] == "pending" and step >= u % 3:
                sc.open_features(u)
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


def test_online_recognizer_from_features_equals_process_features():
    from test_gpu_align import TRACE
    from test_gpu_online_recognizer import CAT, CONF, HELLO, comparable
    waves = [pk.read_wav(HELLO), pk.read_wav(CAT), np.ascontiguousarray(pk.read_wav(HELLO)[:300])]
    rec = pk.Recognizer(CONF, max_utts=1, max_total_samples=max(len(w) for w in waves), trace_capacity=TRACE)
    fb, cmvn = [], []
    for w in waves:
        rec.process([w])
        fb.append(rec.batch.fetch_fbank(0))
        cmvn.append(rec.batch.fetch_cmvn(0))
    want = rec.process_features(fb, "raw")
    assert want[0].text and want[1].text and want[2].text == "" and fb[2].shape == (0, 40)
    online = pk.OnlineRecognizer(CONF, max_streams=3, max_step_samples=3 * 1600, trace_capacity=TRACE)
    for kind, src in (("raw", fb), ("normalized", cmvn)):
        pos, live = [0] * 3, set(range(3))
        for u in range(3):
            online.open_features(u, kind) if kind == "normalized" else online.open_features(u)     # (kind defaults to raw)
            assert online.scorer.slot_kind(u) == kind
        while live:
            closing = []
            for u in sorted(live):
                online.push_features(u, src[u][pos[u]:pos[u] + 10])
                pos[u] += 10
                if pos[u] >= src[u].shape[0]:
                    online.close(u)
                    closing.append(u)
            online.step()
            for u in closing:
                assert online.finished(u)
                live.discard(u)
        for u in range(3):
            assert comparable(online.result(u)) == comparable(want[u]), (kind, u)
    with pytest.raises(pk.PkCodeError) as e:
        online.push_features(0, fb[0][:2])                   # finished: not open
    assert e.value.code == E_STATE
    online.destroy()
    rec.close()


def test_commit_and_endpointing_split_a_feature_slot_as_the_audio_slot():
    """The joined wave of tests/test_gpu_online_utterances.py, with its silence set and rules, commit on: slot 0 takes
    the audio, slot 1 the wave's fbank as RAW features, each step the frames the step's samples completed, so that both
    slots decode the same frames in the same steps.  Every utterance of the feature slot -- where it was cut, by which
    rule, text, weight, segments and their acoustic costs -- is the audio slot's."""
    from test_gpu_align import TRACE
    from test_gpu_online_recognizer import CAT, CONF, HELLO, comparable
    from test_gpu_online_utterances import GAP, RULES, SILENCE
    wave = np.concatenate([pk.read_wav(HELLO), np.zeros(GAP, np.float32), pk.read_wav(CAT)]).astype(np.float32)
    rec = pk.Recognizer(CONF, max_utts=1, max_total_samples=len(wave), trace_capacity=TRACE)
    rec.process([wave])
    fb = rec.batch.fetch_fbank(0)
    rec.close()
    online = pk.OnlineRecognizer(CONF, max_streams=2, max_step_samples=2 * 1600, trace_capacity=TRACE)
    online.am.set_softmax("reference")
    online.set_endpointing(SILENCE, RULES)
    online.decoder.set_commit(True)
    online.open(0)
    online.open_features(1, "raw")
    pos = done = 0
    while pos < len(wave):
        online.push(0, wave[pos:pos + 1600])
        pos = min(pos + 1600, len(wave))
        online.push_features(1, fb[done:pk.num_frames(pos)])
        done = pk.num_frames(pos)
        if pos == len(wave):
            online.close(0)
            online.close(1)
        online.step()
        assert online.partial(0) == online.partial(1) and online.stable(0) == online.stable(1)
    assert done == fb.shape[0] and online.finished(0) and online.finished(1)
    a, b = online.utterances(0), online.utterances(1)
    assert len(a) >= 3 and {p.rule for p in a} >= {0, 1}
    assert [(p.first_frame, p.num_frames, p.rule) for p in b] == [(p.first_frame, p.num_frames, p.rule) for p in a]
    for p, q in zip(a, b):
        assert comparable(q.result) == comparable(p.result)
    assert comparable(online.result(1)) == comparable(online.result(0))
    online.destroy()
