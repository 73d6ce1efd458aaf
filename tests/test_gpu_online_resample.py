"""Native-rate slots of the online scorer (pk_mi355_stream_open_rate): a slot at 44100 Hz and one at 48000 Hz beside a
16 kHz slot, fed whole and in chunks of 1, 7, Q and 441 samples and in seeded random chunks.  Every frame's
log-likelihood row must equal the batch scorer's on the whole wave -- converted by the numpy model over the library's
table (tests/resample_model.py) -- bit for bit.  Short slots, a slot reopened at another rate after NaN audio, an
over-budget push, and the online recognizer at 48000 Hz against Recognizer.process(waves, rates)."""
import os

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth

import resample_model as M
from refmodel_text import DIR
from test_gpu_resample import bits_equal, lib_table

pytestmark = pytest.mark.gpu

E_INVALID = -1
RATES = [44100, 48000, 16000]
CONF = os.path.join(DIR, "recognizer.conf")
HELLO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "en-us-hello.wav")


def convert(wave, rate):
    return np.asarray(wave, np.float32) if rate == 16000 else M.resample(lib_table(rate), wave)


@pytest.fixture(scope="module")
def setup():
    """The model, three half-second waves at 44100 / 48000 / 16000 Hz and the batch scorer's rows for each (once)."""
    layers, prior, L, R = synth.model("S")
    g = synth.global_cmvn_stats()
    am = pk.AcousticModel(layers, prior, L, R)
    rng = np.random.default_rng(31)
    waves = [np.round(2500 * rng.standard_normal(r // 2)).astype(np.float32) for r in RATES]
    want = batch_rows(am, g, [convert(w, r) for w, r in zip(waves, RATES)])
    assert all(w.shape[0] == 48 for w in want)             # 8000 samples at 16 kHz each
    return am, g, waves, want


def batch_rows(am, g, waves16k):
    bs = pk.BatchScorer(am, g, len(waves16k), max(sum(len(w) for w in waves16k), 1))
    bs.set_waves(waves16k)
    bs.score(0.1)
    return [bs.fetch(u).log_prob() for u in range(len(waves16k))]


def run(sc, waves, rates, chunks, slots=None):
    """Wave u into slot slots[u] opened at rates[u], its chunk sizes cycling through chunks[u]; a slot is closed with
    its last chunk.  A step after every round of pushes in which a chunk had 160 samples or more, else after 50 rounds
    (and once everything is closed).  -> every wave's rows (None without any), each step's rows checked to continue
    the last ones."""
    n = len(waves)
    slots = list(range(n)) if slots is None else slots
    for u in range(n):
        sc.open(slots[u], rates[u])
        assert sc.rate(slots[u]) == rates[u]
    pos, turn, nxt, rows = [0] * n, [0] * n, [0] * n, [[] for _ in range(n)]
    live, unflushed, rounds = set(range(n)), set(range(n)), 0
    while unflushed:
        largest = 0
        for u in sorted(live):
            c = chunks[u][turn[u] % len(chunks[u])]
            largest = max(largest, c)
            sc.push(slots[u], waves[u][pos[u]:pos[u] + c])
            pos[u] += c
            turn[u] += 1
            if pos[u] >= len(waves[u]):
                sc.close(slots[u])
                live.discard(u)
        rounds += 1
        if largest >= 160 or rounds == 50 or not live:
            rounds = 0
            sc.step(0.1)
            for u in sorted(unflushed):
                first, r = sc.fetch(slots[u])
                if r.shape[0]:
                    assert first == nxt[u], (u, first, nxt[u])
                    rows[u].append(r)
                    nxt[u] += r.shape[0]
                if u not in live:
                    unflushed.discard(u)
    return [np.concatenate(r) if r else None for r in rows]


def chunkings(waves):
    rng = np.random.default_rng(8)
    q = [lib_table(r).Q if r != 16000 else 1 for r in RATES]
    return {"whole": [[len(w)] for w in waves], "1": [[1]] * 3, "7": [[7]] * 3, "Q": [[x] for x in q], "441": [[441]] * 3,
            "random": [[int(c) for c in rng.integers(1, 3000, 64)] for _ in waves]}


@pytest.mark.parametrize("how", ["whole", "1", "7", "Q", "441", "random"])
def test_native_rate_slots_equal_the_batch_scorer(setup, how):
    am, g, waves, want = setup
    sc = pk.OnlineScorer(am, g, 3, 3 * 8100)
    got = run(sc, waves, RATES, chunkings(waves)[how])
    for u in range(3):
        assert got[u] is not None and got[u].shape == want[u].shape, (how, RATES[u])
        assert bits_equal(got[u], want[u]), (how, RATES[u])


def test_short_slots_reopening_and_the_budget(setup):
    am, g, waves, want = setup
    sc = pk.OnlineScorer(am, g, 3, 2000)
    # N_out = 399: no frame.  N_out = 400: the one frame of the batch scorer
    t = lib_table(44100)
    n399, n400 = -(-399 * t.Q // t.P), -(-400 * t.Q // t.P)
    assert (M.num_output(t, n399), M.num_output(t, n400)) == (399, 400)
    short = [waves[0][:n399], waves[0][:n400]]
    got = run(sc, short, [44100, 44100], [[500], [500]])
    assert got[0] is None
    (one,) = batch_rows(am, g, [convert(short[1], 44100)])
    assert one.shape[0] == 1 and bits_equal(got[1], one)

    # a slot that streamed NaN at 48000 Hz is reopened at 44100 Hz, then at 16000 Hz: fresh each time
    nan = np.full(6000, np.nan, np.float32)
    got = run(sc, [nan], [48000], [[1500]], slots=[1])
    assert got[0] is not None and np.isnan(got[0]).all()
    piece = [waves[0][:9000], waves[2][:3000]]
    fresh = batch_rows(am, g, [convert(piece[0], 44100), piece[1]])
    for wave, rate, rows in ((piece[0], 44100, fresh[0]), (piece[1], 16000, fresh[1])):
        got = run(sc, [wave], [rate], [[1000]], slots=[1])
        assert bits_equal(got[0], rows), rate

    # an over-budget push is refused and loses nothing: 2000 samples of capacity at 16 kHz are 6000 at 48000 Hz
    wave = waves[1][:12000]
    (rows,) = batch_rows(am, g, [convert(wave, 48000)])
    sc.open(0, 48000)
    sc.push(0, wave[:3000])
    with pytest.raises(pk.PkCodeError) as e:
        sc.push(0, wave[3000:6100])
    assert e.value.code == E_INVALID and "48000" in str(e.value)
    out, pos = [], 3000
    while True:
        sc.step(0.1)
        first, r = sc.fetch(0)
        if r.shape[0]:
            assert first == sum(x.shape[0] for x in out)
            out.append(r)
        if pos is None:
            break
        sc.push(0, wave[pos:pos + 3000])
        pos += 3000
        if pos >= len(wave):
            sc.close(0)
            pos = None
    assert bits_equal(np.concatenate(out), rows)
    for bad in (16001, 7999):
        with pytest.raises(pk.PkCodeError) as e:
            sc.open(0, bad)
        assert e.value.code == E_INVALID and str(bad) in str(e.value)
    sc.open(0)                                             # the refused opens left the slot free
    assert sc.rate(0) == 16000
    sc.close(0)
    sc.step(0.1)


def comparable(r):
    bits = lambda x: np.float32(x).view(np.uint32).item()
    return (r.text, r.words, bits(r.weight), r.ok, bits(r.loglikelihood_per_frame),
            [(s.word, s.start_frame, s.num_frames, bits(s.graph_cost), bits(s.acoustic_cost)) for s in r.segments])


def test_online_recognizer_at_48000(setup):
    """The reference's hello wave brought to 48 kHz by linear interpolation: the whole Result, segments included."""
    hello = pk.read_wav(HELLO)
    at = np.arange(3 * len(hello)) / 3.0
    wave = np.round(np.interp(at, np.arange(len(hello)), hello)).astype(np.float32)
    rec = pk.Recognizer(CONF, max_utts=1, max_total_samples=len(hello) + 16)
    (want,) = rec.process([wave], rates=[48000])
    rec.close()
    assert want.ok == 1 and want.text and want.segments
    online = pk.OnlineRecognizer(CONF, max_streams=2, max_step_samples=2 * 1700)
    online.open(1, 48000)
    for pos in range(0, len(wave), 4800):
        online.push(1, wave[pos:pos + 4800])
        if pos + 4800 >= len(wave):
            online.close(1)
        online.step()
    assert online.finished(1)
    assert comparable(online.result(1)) == comparable(want)
    online.destroy()
