"""The online scorer (csrc/capi_stream.hip, pk_mi355_stream_*): PCM pushed in chunks, scored step by step as frames become
final.  Every frame's log-likelihoods must equal the batch scorer's on the whole wave bit for bit, whatever the chunk
sizes, with many slots in one object opened and closed at different steps and reused."""
import os

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_INVALID, E_STATE = -1, -4


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def chunks_of(n, how, rng):
    """Chunk sizes summing to n: "whole", an int (fixed size), "random" (sizes in [1, 8000]) or "random0" (with
    empty pushes in between)."""
    if how == "whole":
        return [n]
    if isinstance(how, int):
        return [how] * (n // how) + ([n % how] if n % how else [])
    out, left = [], n
    while left > 0:
        if how == "random0" and rng.random() < 0.3:
            out.append(0)
        c = int(min(left, rng.integers(1, 8001)))
        out.append(c)
        left -= c
    return out


def run_jobs(sc, jobs, prob_scale=0.1, i16=False):
    """jobs: dicts {slot, wave, chunks, start}.  A job opens its slot at step `start` or later (once the slot's earlier
    job has been flushed), pushes one chunk per step, closes after its last chunk; the step after close flushes it.
    Returns every job's rows [T][num_pdfs], checking that each step's rows continue where the last ones ended."""
    n = len(jobs)
    rows = [[] for _ in range(n)]
    nxt = [0] * n
    state = ["pending"] * n
    k = [0] * n
    pos = [0] * n
    busy = {}
    step = 0
    while any(s != "done" for s in state):
        for i, j in enumerate(jobs):
            if state[i] == "pending" and step >= j["start"] and j["slot"] not in busy:
                sc.open(j["slot"])
                busy[j["slot"]] = i
                state[i] = "open"
            if state[i] == "open":
                if k[i] < len(j["chunks"]):
                    c = j["chunks"][k[i]]
                    w = j["wave"][pos[i]:pos[i] + c]
                    sc.push(j["slot"], w.astype(np.int16) if i16 else w)
                    pos[i] += c
                    k[i] += 1
                    if k[i] == len(j["chunks"]) and j.get("close_with_last"):
                        sc.close(j["slot"])           # the flushing step also computes new frames
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
    return [np.concatenate(r) if r else None for r in rows]


def waves_under_test():
    ws = [pk.read_wav(os.path.join(GOLDEN, f)) for f in ("en-us-hello.wav", "en-us-cat.wav")]
    ws += [synth.utterance(900 + i, seconds=1.0)[:n] for i, n in enumerate([0, 399, 400, 401, 559, 560, 1000])]
    ws.append(synth.utterance(950, seconds=7.3))          # 728 frames: the 600-frame window slides
    return ws


def make_jobs(waves, slots, seed):
    rng = np.random.default_rng(seed)
    hows = ["whole", 160, 399, "random", "random0"]
    jobs = []
    for i, w in enumerate(waves):
        how = 1 if 0 < len(w) <= 1000 and i % 2 else hows[i % len(hows)]
        jobs.append({"slot": i % slots, "wave": w, "chunks": chunks_of(len(w), how, rng), "start": int(rng.integers(0, 6)),
                     "close_with_last": i % 3 == 1})
    return jobs


def refmodel():
    from refmodel_text import load_text_model
    layers, prior, L, R, tid2pdf, cmvn41 = load_text_model()
    return layers, prior, L, R, tid2pdf, cmvn41


def model_s(**kw):
    layers, prior, L, R = synth.model("S", **kw)
    return layers, prior, L, R, None, synth.global_cmvn_stats()


def batch_rows(am, g, waves):
    bs = pk.BatchScorer(am, g, len(waves), max(sum(len(w) for w in waves), 1))
    bs.set_waves(waves)
    bs.score(0.1)
    return [bs.fetch(u).log_prob() for u in range(len(waves))]


# ---------------------------------------------------------------- 1. bit for bit the batch scorer

@pytest.mark.parametrize("softmax", ["stable", "reference"])
@pytest.mark.parametrize("which", ["refmodel", "S"])
def test_stream_equals_batch(which, softmax):
    layers, prior, L, R, tid2pdf, g = refmodel() if which == "refmodel" else model_s()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf).set_softmax(softmax)
    waves = waves_under_test()
    want = batch_rows(am, g, waves)
    sc = pk.OnlineScorer(am, g, 4, 200000)                 # 10 jobs on 4 slots: slots are reused
    got = run_jobs(sc, make_jobs(waves, 4, seed=11 if which == "S" else 12))
    for u, (w, r) in enumerate(zip(waves, want)):
        T = pk.num_frames(len(w))
        if T == 0:
            assert got[u] is None, u
            continue
        assert got[u].shape == r.shape == (T, am.num_pdfs()), (u, got[u].shape, r.shape)
        assert bits_equal(got[u], r), (u, len(w), np.max(np.abs(got[u] - r)))


def test_stream_int16_pushes_and_one_sample_chunks():
    """int16 ingestion, and a stream fed one sample per step across a frame boundary and past the look-ahead."""
    layers, prior, L, R, tid2pdf, g = refmodel()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    waves = [synth.utterance(960, seconds=0.1)[:1400], pk.read_wav(os.path.join(GOLDEN, "en-us-hello.wav"))]
    want = batch_rows(am, g, waves)
    sc = pk.OnlineScorer(am, g, 2, 10000)
    jobs = [{"slot": 0, "wave": waves[0], "chunks": [1] * len(waves[0]), "start": 0},
            {"slot": 1, "wave": waves[1], "chunks": chunks_of(len(waves[1]), 333, None), "start": 3}]
    got = run_jobs(sc, jobs, i16=True)
    for u in range(2):
        assert bits_equal(got[u], want[u]), u


@pytest.mark.parametrize("softmax", ["reference", "stable"])
def test_no_context_model_against_the_oracle(softmax):
    """L + R = 0 through the online scorer (its column shifts are non-negative by construction; the batch scorer lays
    models with L + R < 3 out with row = column, tests/test_gpu_reference_pin.py runs it): the oracle, bitwise with
    the reference softmax, within the 1e-4 contract with the stable one."""
    layers, prior, L, R, _, g = model_s(left=0, right=0)
    am = pk.AcousticModel(layers, prior, L, R).set_softmax(softmax)
    waves = [pk.read_wav(os.path.join(GOLDEN, "en-us-cat.wav")), synth.utterance(970, seconds=6.5),
             synth.utterance(971, seconds=0.03)]
    sc = pk.OnlineScorer(am, g, 2, 120000)
    rng = np.random.default_rng(5)
    jobs = [{"slot": i % 2, "wave": w, "chunks": chunks_of(len(w), "random", rng), "start": i} for i, w in enumerate(waves)]
    got = run_jobs(sc, jobs)
    nn = O.Nnet(layers)
    for u, w in enumerate(waves):
        ref = nn.am_compute(O.cmvn(g, O.Fbank().compute(w)), prior, L, R, 0.1)
        assert got[u].shape == ref.shape
        if softmax == "reference":
            assert bits_equal(got[u], ref), u
        else:
            err = np.abs(got[u].astype(np.float64) - ref)
            assert np.all(err <= 1e-4 * np.maximum(np.abs(ref), 1.0)), (u, err.max())


def test_many_streams_one_step_each():
    """32 streams of mixed lengths advanced together, 100 ms per step: the whole-batch answer."""
    layers, prior, L, R, tid2pdf, g = model_s()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    rng = np.random.default_rng(3)
    waves = [synth.utterance(1000 + i, seconds=float(rng.uniform(0.02, 3.0))) for i in range(32)]
    want = batch_rows(am, g, waves)
    sc = pk.OnlineScorer(am, g, 32, 32 * 1600)
    jobs = [{"slot": i, "wave": w, "chunks": chunks_of(len(w), 1600, None), "start": int(rng.integers(0, 4))}
            for i, w in enumerate(waves)]
    got = run_jobs(sc, jobs)
    assert any(pk.num_frames(len(w)) == 0 for w in waves)
    for u in range(32):
        if pk.num_frames(len(waves[u])) == 0:
            assert got[u] is None, u
        else:
            assert bits_equal(got[u], want[u]), u


def test_device_rows_are_the_fetched_rows():
    layers, prior, L, R, tid2pdf, g = refmodel()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    w = pk.read_wav(os.path.join(GOLDEN, "en-us-hello.wav"))
    sc = pk.OnlineScorer(am, g, 1, 10000)
    sc.open(0)
    sc.push(0, w[:4000])
    sc.step(0.1)
    ptr, first, count = sc.loglik_device(0)
    f2, rows = sc.fetch(0)
    assert first == f2 == 0 and count == rows.shape[0] == pk.num_frames(4000) - R and ptr
    host = np.zeros_like(rows)
    assert pk.lib().pk_mi355_memcpy(host.ctypes.data, ptr, host.nbytes, 2) == 0
    assert bits_equal(host, rows)


# ---------------------------------------------------------------- 2. state and argument errors are status codes

def test_state_errors():
    layers, prior, L, R, tid2pdf, g = refmodel()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    sc = pk.OnlineScorer(am, g, 2, 1000)
    w = synth.utterance(980, seconds=0.1)

    def code(f, *a):
        with pytest.raises(pk.PkCodeError) as e:
            f(*a)
        return e.value.code

    assert code(sc.step) == E_STATE                      # no open slot
    assert code(sc.push, 0, w[:10]) == E_STATE           # not open
    assert code(sc.open, 2) == E_INVALID                 # out of range
    sc.open(0)
    assert code(sc.open, 0) == E_STATE                   # already open
    sc.push(0, w[:600])
    assert code(sc.push, 0, w[:401]) == E_INVALID        # over the step capacity: nothing consumed
    sc.push(0, w[600:1000])                              # exactly the capacity
    sc.push(0, w[:0])                                    # empty push
    sc.close(0)
    assert code(sc.push, 0, w[:10]) == E_STATE           # closed
    assert code(sc.close, 0) == E_STATE
    assert code(sc.open, 0) == E_STATE                   # closed, not yet flushed
    sc.step(0.1)
    first, rows = sc.fetch(0)
    want = batch_rows(am, g, [w[:1000]])[0]
    assert first == 0 and bits_equal(rows, want)
    assert code(sc.step) == E_STATE                      # the flush freed the slot
    sc.open(0)                                           # reuse after close
    sc.close(0)
    sc.step(0.1)                                         # a stream of no samples: no frames
    assert sc.fetch(0)[1].shape == (0, am.num_pdfs())


def test_f16_models_are_refused():
    layers, prior, L, R, tid2pdf, g = refmodel()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf, precision="f16x3")
    with pytest.raises(pk.PkCodeError) as e:
        pk.OnlineScorer(am, g, 1, 1000)
    assert e.value.code == E_INVALID


# ---------------------------------------------------------------- 3. both scorers exactly at their capacity

FULL_LENGTHS = [0, 399, 400, 560, 720, 880, 1040, 1360, 1680]       # 0, 0, 1, 2, 3, 4, 5, 7 and 9 frames
_alone = {}


def scored_alone(which, softmax, am, g, n):
    """Utterance u of the full batch (FULL_LENGTHS in turn), scored alone in a fresh one-utterance BatchScorer: made
    once per model and softmax, shared by the cases below and left unchanged."""
    waves, rows = _alone.setdefault((which, softmax), ([], []))
    for u in range(len(waves), n):
        waves.append(synth.utterance(1100 + u, seconds=0.2)[:FULL_LENGTHS[u % len(FULL_LENGTHS)]])
        rows.append(batch_rows(am, g, [waves[u]])[0])
    return waves[:n], rows[:n]


@pytest.mark.parametrize("max_utts", [48, 96])
@pytest.mark.parametrize("lanes", ["1", "2"])
@pytest.mark.parametrize("softmax", ["stable", "reference"])
@pytest.mark.parametrize("which", ["refmodel", "S"])
def test_batch_exactly_full_equals_each_utterance_alone(which, softmax, lanes, max_utts, monkeypatch):
    """A batch scorer filled to both of its capacities (max_utts utterances, max_total_samples = the exact sum of the
    lengths) with empty, one-frame and not-a-multiple-of-four utterances, so that the column shift changes every few
    compact rows.  PK_MI355_CHUNK=128 is rounded up to the 256-row tile of the f16 kernels, and 48 utterances make 224
    compact rows: one pass, not full.  96 utterances make 456: two passes, the second not full, and with
    PK_MI355_LANES=2 one on each lane."""
    layers, prior, L, R, tid2pdf, g = refmodel() if which == "refmodel" else model_s()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf).set_softmax(softmax)
    waves, want = scored_alone(which, softmax, am, g, max_utts)
    monkeypatch.setenv("PK_MI355_CHUNK", "128")
    monkeypatch.setenv("PK_MI355_LANES", lanes)
    frames = [pk.num_frames(len(w)) for w in waves]
    assert sum((T + 3) // 4 * 4 for T in frames) == {48: 224, 96: 456}[max_utts]
    bs = pk.BatchScorer(am, g, max_utts, sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    for u in range(max_utts):
        got = bs.fetch(u).log_prob()
        assert got.shape == want[u].shape == (frames[u], am.num_pdfs() if frames[u] else 0), (u, got.shape)
        assert bits_equal(got, want[u]), (u, len(waves[u]))


@pytest.mark.parametrize("softmax", ["stable", "reference"])
@pytest.mark.parametrize("which", ["refmodel", "S"])
def test_stream_exactly_full_twice(which, softmax):
    """Five slots, max_step_samples = what one step pushes.  Step 1 pushes it all; step 2 pushes as much again and
    closes every slot, so every slot flushes its R held-back frames on top of its new ones: the max_frames +
    slots x (R + 3) row bound.  Every slot's second-step row count is 1 mod 4 (three padding rows each), except the
    slot that gets fewer than 400 samples in all and has no frames."""
    layers, prior, L, R, tid2pdf, g = refmodel() if which == "refmodel" else model_s()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf).set_softmax(softmax)

    def second_step_rows(p):
        return pk.num_frames(2 * p) - max(0, pk.num_frames(p) - R)

    per_step = [199]
    for base in (400, 1700, 3100, 5000):
        per_step.append(next(p for p in range(base, base + 1000) if second_step_rows(p) % 4 == 1))
    assert pk.num_frames(2 * per_step[0]) == 0 and all(second_step_rows(p) % 4 == 1 for p in per_step[1:])
    waves = [synth.utterance(1200 + i, seconds=1.0)[:2 * p] for i, p in enumerate(per_step)]
    assert [len(w) for w in waves] == [2 * p for p in per_step]
    want = batch_rows(am, g, waves)
    sc = pk.OnlineScorer(am, g, 5, sum(per_step))
    got = run_jobs(sc, [{"slot": i, "wave": w, "chunks": [p, p], "start": 0, "close_with_last": True}
                        for i, (w, p) in enumerate(zip(waves, per_step))])
    assert got[0] is None
    for u in range(1, 5):
        assert got[u].shape == want[u].shape == (pk.num_frames(len(waves[u])), am.num_pdfs()), u
        assert bits_equal(got[u], want[u]), u
