"""ResampleKernel (csrc/resample.hip) through pk.resample and BatchScorer.set_waves(rates=...): bit for bit the numpy
model (tests/resample_model.py) run over the LIBRARY's table -- every rate, the lengths at which the output count or
the tiling changes, both zero-padded edges, full scale, 32-bit values, one NaN -- and a ragged batch mixing every rate
with 16 kHz against set_waves of the model-converted waves."""
import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth

import resample_model as M

pytestmark = pytest.mark.gpu

RATES = [8000, 11025, 22050, 32000, 44100, 48000, 96000]
E_INVALID = -1


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


_tables = {}


def lib_table(rate):
    """The model's table with the library's float32 weights (first / count are checked equal on the CPU)."""
    if rate not in _tables:
        lib = pk.resample_table(rate)
        t = M.table(rate)
        assert np.array_equal(lib.first, t.first) and np.array_equal(lib.count, t.count)
        _tables[rate] = M.with_weights(t, lib.weights)
    return _tables[rate]


def lengths_for(t):
    """N_in = 0, 1, Q - 1, Q, Q + 1, max_taps, the three lengths giving N_out = 399, 400, 401, and about 0.3 s (more
    than one tile of outputs, not a multiple of anything)."""
    def smallest_giving(n_out):                             # (8000 Hz gives even counts only: the first length reaching it)
        n = -(-n_out * t.Q // t.P)                          # ceil(n_out Q / P)
        assert n_out <= M.num_output(t, n) <= n_out + 1 and M.num_output(t, n - 1) < n_out
        return n
    return [0, 1, t.Q - 1, t.Q, t.Q + 1, t.max_taps] + [smallest_giving(n) for n in (399, 400, 401)] + [int(0.3 * t.rate) + 7]


def contents(n, rng):
    """name -> the signal of n samples"""
    out = {"noise": rng.integers(-32768, 32768, n).astype(np.float32)}
    if n >= 1:
        first, last = np.zeros(n, np.float32), np.zeros(n, np.float32)
        first[0], last[-1] = 12345.0, -23456.0
        out["impulse_first"], out["impulse_last"] = first, last
        out["full_scale"] = np.where(rng.integers(0, 2, n) == 1, np.float32(32767), np.float32(-32768)).astype(np.float32)
        out["int32_range"] = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.float32)
    return out


@pytest.mark.parametrize("rate", RATES)
def test_resample_equals_the_model_bit_for_bit(rate):
    t = lib_table(rate)
    rng = np.random.default_rng(rate)
    for n in lengths_for(t):
        for name, x in contents(n, rng).items():
            want = M.resample(t, x)
            got = pk.resample(x, rate)
            assert got.dtype == np.float32 and got.shape == (M.num_output(t, n),), (n, name)
            assert bits_equal(got, want), (n, name, int(np.sum(got.view(np.uint32) != want.view(np.uint32))))
    # the edges are not silent: an impulse at either end reaches the output
    n = t.Q + t.max_taps + 40
    x = contents(n, rng)
    assert np.any(pk.resample(x["impulse_first"], rate)[:4] != 0) and np.any(pk.resample(x["impulse_last"], rate)[-4:] != 0)


@pytest.mark.parametrize("rate", RATES)
def test_one_nan_sample(rate):
    """NaN exactly in the outputs whose window holds the sample; no other bit moves."""
    t = lib_table(rate)
    rng = np.random.default_rng(rate + 1)
    n = int(0.05 * rate) + 3
    x = rng.integers(-20000, 20000, n).astype(np.float32)
    clean = pk.resample(x, rate)
    for at in (0, n // 2, n - 1):
        bad = x.copy()
        bad[at] = np.nan
        got = pk.resample(bad, rate)
        j = np.arange(got.shape[0])
        base = t.first[j % t.P] + (j // t.P) * t.Q
        holds = (base <= at) & (at < base + t.count[j % t.P])
        assert holds.any() and not holds.all()
        assert np.array_equal(np.isnan(got), holds), at
        assert bits_equal(got[~holds], clean[~holds]), at
        assert bits_equal(got, M.resample(t, bad)), at


def test_a_rate_whose_table_and_span_pass_64_kib_of_lds():
    """8016 Hz: 1000 phases of 13 taps and a span of 1 500 samples are 66 060 bytes of LDS, more than a launch gets
    without asking -- the one size at which the launcher takes another path."""
    rate = 8016
    t = lib_table(rate)
    span = (1023 // t.P + 1) * t.Q + int((t.first + t.count).max() - t.first.min())
    assert 4 * (t.P * (t.max_taps | 1) + span) + 8 * t.P > 65536
    rng = np.random.default_rng(rate)
    for n in (t.Q + 1, 2 * t.Q + 77):                       # one tile, and all 1000 phases twice over (two tiles)
        x = rng.integers(-32768, 32768, n).astype(np.float32)
        assert bits_equal(pk.resample(x, rate), M.resample(t, x)), n


def test_identity_and_refusals():
    x = np.arange(-500, 500, dtype=np.float32)
    assert bits_equal(pk.resample(x, 16000), x)
    assert pk.resample(np.zeros(0, np.float32), 48000).shape == (0,)
    for bad in (16001, 7999):
        with pytest.raises(pk.PkError) as e:
            pk.resample(x, bad)
        assert e.value.code == E_INVALID and str(bad) in str(e.value)


# ---------------------------------------------------------------- the batch scorer

@pytest.fixture(scope="module")
def ragged():
    """Nine utterances: every rate and two at 16000, ragged lengths up to half a second, one too short for a frame.
    -> (model, cmvn stats, native waves, rates, the model-converted 16 kHz waves)"""
    layers, prior, L, R = synth.model("S")
    g = synth.global_cmvn_stats()
    am = pk.AcousticModel(layers, prior, L, R)
    rates = [44100, 16000, 8000, 96000, 11025, 16000, 48000, 22050, 32000]
    seconds = [0.5, 0.31, 0.2, 0.12, 0.45, 0.02, 0.33, 0.27, 0.4]
    rng = np.random.default_rng(77)
    native = [np.round(3000 * rng.standard_normal(int(s * r) + i)).astype(np.float32) for i, (s, r) in enumerate(zip(seconds, rates))]
    converted = [w if r == 16000 else M.resample(lib_table(r), w) for w, r in zip(native, rates)]
    return am, g, native, rates, converted


def stages(bs, n):
    return [(bs.fetch_fbank(u), bs.fetch_cmvn(u), bs.fetch(u).log_prob()) for u in range(n)]


def test_ragged_batch_of_all_rates(ragged):
    am, g, native, rates, converted = ragged
    n = len(native)
    total = sum(len(w) for w in converted)
    want_bs = pk.BatchScorer(am, g, n, total)
    want_bs.set_waves(converted)
    want_bs.score(0.1)
    want = stages(want_bs, n)
    assert sum(1 for w in converted if pk.num_frames(len(w)) == 0) == 1 and sum(1 for s in want if s[2].shape[0] > 10) >= 7

    bs = pk.BatchScorer(am, g, n, total)                  # capacity counts 16 kHz samples: an exact fit
    bs.set_waves(native, rates=rates)
    bs.score(0.1)
    got = stages(bs, n)
    for u in range(n):
        assert bs.num_frames(u) == pk.num_frames(len(converted[u]))
        for a, b in zip(got[u], want[u]):
            assert bits_equal(a, b), (u, rates[u])

    # a NaN neighbour (native and 16 kHz) changes nothing of the others
    poisoned = [w.copy() for w in native]
    poisoned[0][:] = np.nan
    poisoned[1][:] = np.nan
    bs.set_waves(poisoned, rates=rates)
    bs.score(0.1)
    after = stages(bs, n)
    assert np.isnan(after[0][2]).all() and np.isnan(after[1][2]).all()
    for u in range(2, n):
        for a, b in zip(after[u], want[u]):
            assert bits_equal(a, b), (u, rates[u])

    # the object is reusable for plain 16 kHz calls, and rates of 16000 throughout are today's call
    bs.set_waves(converted, rates=[16000] * n)
    bs.score(0.1)
    for u, s in enumerate(stages(bs, n)):
        for a, b in zip(s, want[u]):
            assert bits_equal(a, b), u

    # one sample over the capacity is refused
    small = pk.BatchScorer(am, g, n, total - 1)
    with pytest.raises(pk.PkError) as e:
        small.set_waves(native, rates=rates)
    assert e.value.code == E_INVALID and "samples" in str(e.value)
    with pytest.raises(pk.PkError) as e:
        bs.set_waves(native, rates=[16001] + rates[1:])
    assert e.value.code == E_INVALID and "16001" in str(e.value)
    with pytest.raises(pk.PkError):
        bs.set_waves(native, rates=rates[:-1])
