"""The online scorer with a front-end spec: pk.OnlineScorer(am, stats, ..., frontend=spec).
Every frame's row equals pk.BatchScorer(am, stats, ..., frontend=spec) on the whole wave bit for bit -- the batch scorer
at a spec is what tests/test_gpu_frontend_any.py pins to the numpy restatement and the oracle -- at every chunking, while
the CMVN window slides and its ring wraps, over several slots that run out and are reopened, beside RAW and NORMALIZED
feature slots in the same steps, at other sample rates, with poisoned neighbours, in both softmax modes; at the default
spec the rows are pk.OnlineScorer's.  The specs are FA.BATCH_SPECS: D = 13, 64, 65, 80 take StreamCmvnChainKernel and
StreamFeatureLayoutKernel (one block of lanes, a full one, a second one-lane block), D = 40 takes StreamCmvnKernel.
No tolerance anywhere: every comparison is of bytes."""
import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth_graph as SG

import frontend_any_cases as FA
from test_gpu_frontend_any import tiny, bits_equal

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
DIMS = sorted(FA.BATCH_SPECS)
L, R = 2, 1
SHIFT = 160


def samples_for(frames):
    return 400 + SHIFT * (frames - 1)


_stats = {}


def stats_at(D):
    """Count 2500 and the means of one wave's features at the spec (what a model's statistics are to its features)."""
    if D not in _stats:
        fb = pk.Frontend(FA.BATCH_SPECS[D]).compute(FA.wave_i16(8000, 5))
        _stats[D] = np.concatenate([fb.astype(np.float64).mean(axis=0) * 2500.0, [2500.0]]).astype(np.float32)
    return _stats[D]


def batch_stages(am, g, spec, waves):
    """The reference: BatchScorer(frontend=spec) on the whole waves -> per wave (fbank rows, CMVN'd rows, log-likelihoods)."""
    bs = pk.BatchScorer(am, g, len(waves), max(sum(len(w) for w in waves), 1), frontend=spec)
    bs.set_waves(waves)
    bs.score(0.1)
    out = [(bs.fetch_fbank(u), bs.fetch_cmvn(u), bs.fetch(u).log_prob()) for u in range(len(waves))]
    bs.close()
    return out


def chunks_of(n, how, rng=None):
    """Chunk sizes summing to n: "whole", an int, or "random": sizes in [1, 3000] with empty pushes in between."""
    if how == "whole":
        return [n]
    if isinstance(how, int):
        return [how] * (n // how) + ([n % how] if n % how else [])
    out, left = [], n
    while left > 0:
        if rng.random() < 0.3:
            out.append(0)
        c = int(min(left, rng.integers(1, 3001)))
        out.append(c)
        left -= c
    return out


def run_jobs(sc, jobs):
    """jobs: dicts {slot, kind ("audio" / "raw" / "normalized"), data, chunks, start, rate}.  A job opens its slot at step
    `start` or later (once the slot's earlier job has been flushed), pushes one chunk a step and closes in the step after
    its last chunk.  -> every job's rows; each step's rows must continue where the slot's last ones ended."""
    n = len(jobs)
    rows, nxt, state, k, pos, busy, step = [[] for _ in range(n)], [0] * n, ["pending"] * n, [0] * n, [0] * n, {}, 0
    N = sc._am.num_pdfs()
    while any(s != "done" for s in state):
        for i, j in enumerate(jobs):
            audio = j["kind"] == "audio"
            if state[i] == "pending" and step >= j.get("start", 0) and j["slot"] not in busy:
                sc.open(j["slot"], j.get("rate", 16000)) if audio else sc.open_features(j["slot"], j["kind"])
                assert sc.slot_kind(j["slot"]) == (None if audio else j["kind"])
                busy[j["slot"]] = i
                state[i] = "open"
            if state[i] == "open":
                if k[i] < len(j["chunks"]):
                    c = j["chunks"][k[i]]
                    (sc.push if audio else sc.push_features)(j["slot"], j["data"][pos[i]:pos[i] + c])
                    pos[i] += c
                    k[i] += 1
                else:
                    sc.close(j["slot"])
                    state[i] = "closed"
        sc.step(0.1)
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


def job(slot, data, chunks="whole", kind="audio", start=0, rate=16000, rng=None):
    return {"slot": slot, "kind": kind, "data": data, "chunks": chunks_of(len(data), chunks, rng), "start": start, "rate": rate}


def assert_rows(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if b.shape[0] == 0:
            assert a.shape[0] == 0, (what, i, a.shape)
            continue
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        assert bits_equal(a, b), "%s, job %d: %d of %d rows differ, the first at %d" % (
            what, i, int(np.any(a != b, axis=1).sum()), a.shape[0], int(np.argmax(np.any(a != b, axis=1))))


# ---------------------------------------------------------------- chunkings

@pytest.mark.parametrize("D", DIMS)
def test_every_chunking_gives_the_batch_scorers_rows(D):
    spec, g, am = FA.BATCH_SPECS[D], stats_at(D), tiny(D, L, R)
    assert spec.dim == D
    lengths = (399, 400, 559, 560, 1200)                 # no frame; one (T <= R); one; two; six
    waves = [FA.wave_i16(n, 100 * D + n) for n in lengths]
    want = [s[2] for s in batch_stages(am, g, spec, waves)]
    assert [w.shape[0] for w in want] == [0, 1, 1, 2, 6] and all(np.isfinite(w).all() for w in want)
    sc = pk.OnlineScorer(am, g, 2, 8000, frontend=spec)
    assert sc.feat_dim() == D
    rng = np.random.default_rng(D)
    for how in ("whole", 159, 160, 161, 400, "random"):
        for w, ref in zip(waves, want):
            assert_rows(run_jobs(sc, [job(1, w, how, rng=rng)]), [ref], "D=%d, %d samples, chunks %s" % (D, w.size, how))
    long = FA.wave_float(20000, D)                        # 123 frames in random chunks, empty pushes included
    ref = batch_stages(am, g, spec, [long])[0][2]
    for seed in range(2):
        assert_rows(run_jobs(sc, [job(0, long, "random", rng=np.random.default_rng([D, seed]))]), [ref], "D=%d random %d" % (D, seed))
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- the window

@pytest.mark.parametrize("D", DIMS)
def test_the_window_slides(D):
    spec, g, am = FA.BATCH_SPECS[D], stats_at(D), tiny(D, L, R)
    w = FA.wave_i16(samples_for(640), 7 * D)              # 640 frames: the window slides from frame 600 on
    ref = batch_stages(am, g, spec, [w])[0][2]
    assert ref.shape[0] == 640
    sc = pk.OnlineScorer(am, g, 1, samples_for(640), frontend=spec)
    assert_rows(run_jobs(sc, [job(0, w, 4000)]), [ref], "D=%d, 250 ms chunks" % D)
    # one step of more than 600 new frames on top of history: 30 frames, then 610 at once
    first = samples_for(30)
    j = job(0, w)
    j["chunks"] = [first, w.size - first]
    assert_rows(run_jobs(sc, [j]), [ref], "D=%d, 610 frames in one step" % D)
    sc.destroy()
    am.close()


def test_the_ring_wraps_twice_at_80():
    D = 80
    spec, g, am = FA.BATCH_SPECS[D], stats_at(D), tiny(D, L, R)
    w = FA.wave_i16(samples_for(1307), 1307)
    ref = batch_stages(am, g, spec, [w])[0][2]
    assert ref.shape[0] == 1307
    sc = pk.OnlineScorer(am, g, 1, 1600, frontend=spec)
    assert_rows(run_jobs(sc, [job(0, w, 1600)]), [ref], "1307 frames in 100 ms chunks")
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- several slots

@pytest.mark.parametrize("D", DIMS)
def test_several_slots_run_out_and_reopen(D):
    spec, g, am = FA.BATCH_SPECS[D], stats_at(D), tiny(D, L, R)
    waves = [FA.wave_float(n, 11 * D + u) for u, n in enumerate((9000, 2400, 5000, 7300, 3100))]
    want = [s[2] for s in batch_stages(am, g, spec, waves)]
    sc = pk.OnlineScorer(am, g, 4, 4 * 1600, frontend=spec)
    gaps = job(2, waves[2])
    gaps["chunks"] = [1600, 0, 0, 1600, 0, 1800]          # no audio in some steps
    jobs = [job(0, waves[0], 1600), job(1, waves[1], 800), gaps, job(3, waves[3], 1000),
            job(1, waves[4], 1600, start=2)]              # slot 1 closes early and is reopened with another wave
    assert_rows(run_jobs(sc, jobs), want, "D=%d" % D)
    # after the shortest closes, a step of flushes only: both slots closed with nothing pushed since the last step
    two = [FA.wave_float(1500, 3), FA.wave_float(2100, 4)]
    ref = [s[2] for s in batch_stages(am, g, spec, two)]
    for s, w in enumerate(two):
        sc.open(s)
        sc.push(s, w)
    sc.step(0.1)
    got = [[sc.fetch(s)[1]] for s in range(2)]
    sc.close(0)
    sc.close(1)
    sc.step(0.1)
    for s in range(2):
        first, r = sc.fetch(s)
        assert r.shape[0] == R and first == ref[s].shape[0] - R
        got[s].append(r)
    assert_rows([np.concatenate(x) for x in got], ref, "D=%d flushes only" % D)
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- mixed kinds

@pytest.mark.parametrize("D", [80, 40])
def test_audio_raw_and_normalized_slots_in_the_same_steps(D):
    spec, g, am = FA.BATCH_SPECS[D], stats_at(D), tiny(D, L, R)
    w = FA.wave_i16(samples_for(57), 57 + D)
    fb, norm, ref = batch_stages(am, g, spec, [w])[0]
    assert fb.shape == (57, D)
    sc = pk.OnlineScorer(am, g, 3, 3 * 1600, frontend=spec)
    for order in ((0, 1, 2), (2, 0, 1)):
        jobs = [job(order[0], w, 1600), job(order[1], fb, 10, kind="raw"), job(order[2], norm, 10, kind="normalized")]
        assert_rows(run_jobs(sc, jobs), [ref, ref, ref], "D=%d slots %s" % (D, order))
    # the audio slot late, the feature slots of other lengths: records of every kind come and go
    jobs = [job(1, fb[:23], 7, kind="raw"), job(0, w, 1000, start=2), job(2, norm[:31], 9, kind="normalized", start=1)]
    got = run_jobs(sc, jobs)
    a = batch_stages(am, g, spec, [w[:samples_for(23)], w[:samples_for(31)]])
    assert_rows(got, [a[0][2], ref, a[1][2]], "D=%d staggered" % D)
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- rates

@pytest.mark.parametrize("D", [13, 80])
def test_other_rates_equal_resampling_first(D):
    spec, g, am = FA.BATCH_SPECS[D], stats_at(D), tiny(D, L, R)
    native = {8000: FA.wave_i16(4000, 8), 44100: FA.wave_i16(15000, 44)}
    at16 = {r: pk.resample(w, r) for r, w in native.items()}
    want = [s[2] for s in batch_stages(am, g, spec, [at16[8000], at16[44100]])]
    assert all(w.shape[0] > 20 for w in want)
    sc = pk.OnlineScorer(am, g, 2, 2 * 1700, frontend=spec)
    jobs = [job(0, native[8000], 800, rate=8000), job(1, native[44100], 4410, rate=44100)]
    assert_rows(run_jobs(sc, jobs), want, "D=%d" % D)
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- isolation

@pytest.mark.parametrize("D", DIMS)
def test_poisoned_neighbours_and_a_reopened_slot_change_no_bit(D):
    spec, g, am = FA.BATCH_SPECS[D], stats_at(D), tiny(D, L, R)
    w = FA.wave_float(6000, 17 * D)
    ref = batch_stages(am, g, spec, [w])[0][2]
    sc = pk.OnlineScorer(am, g, 3, 3 * 1600, frontend=spec)
    jobs = [job(0, np.full(6000, np.nan, np.float32), 1600), job(1, w, 1600), job(2, np.full(6000, 1e30, np.float32), 1600)]
    got = run_jobs(sc, jobs)
    assert_rows(got[1:2], [ref], "D=%d between a NaN and a 1e30 neighbour" % D)
    assert np.isnan(got[0]).all()
    sc.destroy()
    # a slot that held 705 NaN frames (sums, the whole ring and the history poisoned) and is opened again
    sc = pk.OnlineScorer(am, g, 1, samples_for(705), frontend=spec)
    bad = run_jobs(sc, [job(0, np.full(samples_for(705), np.nan, np.float32), samples_for(352))])
    assert bad[0].shape[0] == 705 and np.isnan(bad[0]).all()
    assert_rows(run_jobs(sc, [job(0, w, 1600)]), [ref], "D=%d reopened after 705 NaN frames" % D)
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- the default spec, both softmax modes

def test_the_default_spec_is_the_plain_online_scorer():
    from pocketkaldi_amd import synth
    g = synth.global_cmvn_stats()
    w = [FA.wave_i16(9000, 1), FA.wave_float(4000, 2)]
    for softmax in ("stable", "reference"):
        am = tiny(40, L, R, softmax=softmax)
        plain = pk.OnlineScorer(am, g, 2, 3200)
        spec = pk.OnlineScorer(am, g, 2, 3200, frontend=pk.frontend_default())
        jobs = [job(0, w[0], 1600), job(1, w[1], 900)]
        a, b = run_jobs(plain, jobs), run_jobs(spec, jobs)
        assert a[0].shape[0] == 54 and np.isfinite(a[0]).all()
        assert_rows(b, a, "default spec, %s softmax" % softmax)
        plain.destroy()
        spec.destroy()
        am.close()


def test_both_softmax_modes_at_80():
    D = 80
    spec, g = FA.BATCH_SPECS[D], stats_at(D)
    w = FA.wave_i16(8000, 5)
    for softmax in ("stable", "reference"):
        am = tiny(D, L, R, softmax=softmax)
        ref = batch_stages(am, g, spec, [w])[0][2]
        assert np.isfinite(ref).all()
        sc = pk.OnlineScorer(am, g, 1, 1600, frontend=spec)
        assert_rows(run_jobs(sc, [job(0, w, 1600)]), [ref], softmax)
        sc.destroy()
        am.close()


# ---------------------------------------------------------------- decoding

def test_online_decoding_equals_decode_batch(tmp_path):
    D = 80
    spec, g, am = FA.BATCH_SPECS[D], stats_at(D), tiny(D, L, R)
    graph = SG.word_loop(30, 8, seed=3)
    assert graph["num_tids"] <= am.num_pdfs()
    path = str(tmp_path / "loop.fst")
    SG.write_fst(path, graph["start"], graph["final"], graph["arcs"])
    fst = pk.Fst(path)
    waves = [FA.wave_float(8000, 40), FA.wave_float(16000, 41)]
    bs = pk.BatchScorer(am, g, 2, 24000, frontend=spec)
    bs.set_waves(waves)
    bs.score(0.1)
    dec = pk.Decoder(fst, am, 2)
    dec.decode_batch(bs)
    want = [dec.result(u) for u in range(2)]
    assert any(w[0] for w in want)
    sc = pk.OnlineScorer(am, g, 2, 3200, frontend=spec)
    od = pk.OnlineDecoder(fst, am, 2)
    pos = [0, 0]
    for s in range(2):
        sc.open(s)
        od.open(s)
    live = {0, 1}
    while live:
        for s in sorted(live):
            sc.push(s, waves[s][pos[s]:pos[s] + 1600])
            pos[s] += 1600
            if pos[s] >= waves[s].size:
                sc.close(s)
        sc.step(0.1, sync=False)
        od.advance(sc)
        live = {s for s in live if pos[s] < waves[s].size}
    for s in range(2):
        got = od.result(s)
        assert got[0] == want[s][0] and np.float32(got[1]).tobytes() == np.float32(want[s][1]).tobytes() and got[2] == want[s][2], s
    for o in (dec, bs):
        o.close()
    od.destroy()
    sc.destroy()
    am.close()


# ---------------------------------------------------------------- failure codes that need a device

def code_of(call, *args, **kw):
    with pytest.raises(pk.PkCodeError) as e:
        call(*args, **kw)
    return e.value.code, str(e.value)


def test_failure_codes():
    D = 80
    spec, g = FA.BATCH_SPECS[D], stats_at(D)
    half = tiny(D, L, R, precision="f16x3")
    code, msg = code_of(pk.OnlineScorer, half, g, 2, 3200, frontend=spec)
    assert code == E_INVALID and "f32" in msg, msg
    half.close()
    am = tiny(D, L, R)
    # the refusals of pk_mi355_frontend_stream_create that need a finalized model, by code and by word
    code, msg = code_of(pk.OnlineScorer, am, g, 2, 3200, frontend=FA.BATCH_SPECS[13])        # the spec's dimension, the model's
    assert code == E_INVALID and "produces 13-dim" in msg and "expects 80" in msg, msg
    code, msg = code_of(pk.OnlineScorer, am, stats_at(13), 2, 3200, frontend=FA.BATCH_SPECS[13])
    assert code == E_INVALID and "produces 13-dim" in msg and "expects 80" in msg, msg      # (before the statistics are looked at)
    code, msg = code_of(pk.OnlineScorer, am, g[:-1], 2, 3200, frontend=spec)                 # the statistics' length
    assert code == E_INVALID and "statistics have 80 entries" in msg and "80-dim model needs 81" in msg, msg
    code, msg = code_of(pk.OnlineScorer, am, np.zeros(41, np.float32), 2, 3200, frontend=spec)
    assert code == E_INVALID and "statistics have 41 entries" in msg and "80-dim model needs 81" in msg, msg
    code, msg = code_of(pk.OnlineScorer, am, stats_at(13), 2, 3200, frontend=spec)
    assert code == E_INVALID and "statistics have 14 entries" in msg and "needs 81" in msg, msg
    for streams, samples in ((0, 3200), (-1, 3200), (2, 0), (2, -1), (0, 0)):                # capacities <= 0
        code, msg = code_of(pk.OnlineScorer, am, g, streams, samples, frontend=spec)
        assert (code, msg) == (E_INVALID, "bad stream capacity"), (streams, samples, msg)
    code, msg = code_of(pk.OnlineScorer, am, g, 2, (1 << 30) + 1, frontend=spec)             # (and one beyond what a step may hold)
    assert (code, msg) == (E_INVALID, "bad stream capacity"), msg
    with pytest.raises(pk.PkError, match="41 entries"):                                      # without frontend=: the old constructor
        pk.OnlineScorer(am, g, 2, 3200)
    w = FA.wave_i16(4000, 9)
    ref = batch_stages(am, g, spec, [w])[0][2]
    sc = pk.OnlineScorer(am, g, 2, 2500, frontend=spec)
    sc.open(0)
    sc.push(0, w[:2000])
    code, msg = code_of(sc.push, 0, w[2000:2501])           # 2501 of 2500: refused, nothing consumed
    assert code == E_INVALID and "capacity" in msg, msg
    sc.open_features(1, "raw")
    code, msg = code_of(sc.push_features, 1, np.zeros((4, D), np.float32))       # a frame counts 160 samples
    assert code == E_INVALID and "capacity" in msg, msg
    sc.close(1)
    sc.step(0.1)
    rows = [sc.fetch(0)[1]]
    sc.push(0, w[2000:])
    sc.close(0)
    sc.step(0.1)
    rows.append(sc.fetch(0)[1])
    assert_rows([np.concatenate(rows)], [ref], "after the refused pushes")
    sc.destroy()
    am.close()
