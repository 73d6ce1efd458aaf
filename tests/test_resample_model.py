"""CPU: the resampler's rule (tests/resample_model.py) pinned by properties, and the library's table held against it.
The table sizes and the filter figures are those of the numpy prototype the feature was specified with; the filter
tests allow twice its figures, for libm differences in the table."""
import numpy as np
import pytest

import pocketkaldi_amd as pk
import resample_model as M

RATES = [8000, 11025, 22050, 32000, 44100, 48000, 96000]
# rate -> (Q, P, fewest taps, most taps, table entries P x max_taps)
FACTS = {8000: (1, 2, 12, 13, 26), 11025: (441, 640, 12, 13, 8320), 22050: (441, 320, 16, 17, 5440), 32000: (2, 1, 25, 25, 25),
         44100: (441, 160, 33, 34, 5440), 48000: (3, 1, 37, 37, 37), 96000: (6, 1, 73, 73, 73)}


@pytest.fixture(scope="module")
def tables():
    return {r: M.table(r) for r in RATES}


@pytest.mark.parametrize("rate", RATES)
def test_plan_and_table_sizes(rate, tables):
    t = tables[rate]
    assert (t.Q, t.P, int(t.count.min()), int(t.count.max()), t.P * t.max_taps) == FACTS[rate]
    assert t.P * t.max_taps <= 16384
    sums = t.weights.sum(axis=1)
    assert 1.00003 < sums.min() and sums.max() < 1.001
    # phase 0 (u = 0) starts before the signal: the left edge really reads the zero padding
    assert -36 <= t.first[0] < 0 and t.first[0] == t.first.min() and np.all(np.diff(t.first) >= 0)
    assert int((t.first + t.count).max() - t.first.min()) <= t.Q + t.max_taps      # what a stream has to carry
    if rate == 96000:
        assert t.first[0] == -36


def test_largest_table_is_11025(tables):
    assert max(t.P * t.max_taps for t in tables.values()) == 8320 == tables[11025].P * tables[11025].max_taps


@pytest.mark.parametrize("rate", RATES)
def test_library_table_equals_the_model(rate, tables):
    t, lib = tables[rate], pk.resample_table(rate)
    assert (lib.Q, lib.P, lib.max_taps) == (t.Q, t.P, t.max_taps)
    assert np.array_equal(lib.first, t.first) and np.array_equal(lib.count, t.count)
    assert lib.weights.dtype == np.float32 and lib.weights.shape == t.weights.shape
    want = t.weights.astype(np.float32)                  # the rounded double
    same = lib.weights == want
    one_ulp = (lib.weights == np.nextafter(want, np.float32(np.inf))) | (lib.weights == np.nextafter(want, np.float32(-np.inf)))
    assert np.all(same | one_ulp)
    for p in range(t.P):                                 # rows are zero-padded behind their count
        assert np.all(lib.weights[p, t.count[p]:] == 0)


@pytest.mark.parametrize("rate", RATES)
def test_num_output_rule(rate, tables):
    t = tables[rate]
    for n in (0, 1, t.Q - 1, t.Q, t.Q + 1, 12345, 2 ** 31 - 1):
        assert M.num_output(t, n) == n * t.P // t.Q == pk.resample_num_output(rate, n)
    assert M.num_output(t, t.Q) == t.P and M.num_output(t, 0) == 0
    for n in (0, 1, t.Q - 1, t.Q, t.Q + 1):
        assert M.resample(t, np.ones(n, np.float32)).shape == (M.num_output(t, n),)


def test_identity_rate_and_refused_rates():
    t = pk.resample_table(16000)
    assert (t.Q, t.P, t.max_taps) == (1, 1, 1) and t.first[0] == 0 and t.count[0] == 1 and t.weights[0, 0] == 1.0
    assert pk.resample_num_output(16000, 777) == 777
    for bad in (16001, 7999, 0, -16000, 96001):
        with pytest.raises(pk.PkError) as e:
            pk.resample_table(bad)
        assert e.value.code == -1 and str(bad) in str(e.value)
        with pytest.raises(pk.PkError) as e:
            pk.resample_num_output(bad, 10)
        assert e.value.code == -1 and str(bad) in str(e.value)


@pytest.mark.parametrize("rate", RATES)
def test_chunked_equals_whole(rate, tables):
    t = tables[rate]
    rng = np.random.RandomState(rate)
    n = 3 * t.Q + 5 * t.max_taps + 17
    x = rng.randint(-3000, 3000, n).astype(np.float32)
    whole = M.resample(t, x)
    assert whole.shape == (M.num_output(t, n),)

    def split(size):
        return [min(size, n - at) for at in range(0, n, size)]
    cuts = sorted(rng.choice(np.arange(1, n), 9, replace=False))
    random_sizes = list(np.diff([0] + list(cuts) + [n]))
    for sizes in (split(1), split(7), split(t.Q), split(441), [n], random_sizes, [0, n, 0]):
        got = M.resample_chunked(t, x, sizes)
        assert got.shape == whole.shape and np.array_equal(got.view(np.uint32), whole.view(np.uint32))


def test_finality_rule(tables):
    for rate, t in tables.items():
        for n in (0, 1, t.max_taps, t.Q + 3, 2 * t.Q + t.max_taps):
            j = M.num_final(t, n)
            assert j <= M.num_output(t, n)
            ends = [int(t.first[k % t.P]) + (k // t.P) * t.Q + int(t.count[k % t.P]) - 1 for k in range(j + 1)]
            assert all(e < n for e in ends[:j]) and ends[j] >= n


def _tone(freq, rate, n, amp=8000.0):
    return (amp * np.sin(2 * np.pi * freq * np.arange(n) / rate)).astype(np.float32)


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


@pytest.mark.parametrize("rate", [44100, 48000])
def test_filter_against_the_ideal(rate, tables):
    t = tables[rate]
    n = rate // 10                                       # 0.1 s
    mid = slice(400, 1200)                               # middle samples of the 1600 out
    for freq, bound in ((1000, 2 * 2.3), (3000, 2 * 2.9)):
        y = M.resample(t, _tone(freq, rate, n))
        ideal = 8000.0 * np.sin(2 * np.pi * freq * np.arange(y.shape[0]) / 16000.0)
        err = _rms(y[mid] - ideal[mid])
        print("rate %d tone %d: rms error %.3f (bound %.1f)" % (rate, freq, err, bound))
        assert err <= bound
    x = _tone(12000, rate, n)                            # above the new Nyquist: gone
    y = M.resample(t, x)
    print("rate %d tone 12000: rms in %.1f out %.3f" % (rate, _rms(x), _rms(y[mid])))
    assert 5600 < _rms(x) < 5700 and _rms(y[mid]) <= 2 * 10.0


def test_upsampling_8000(tables):
    t = tables[8000]
    y = M.resample(t, _tone(1000, 8000, 800))
    ideal = 8000.0 * np.sin(2 * np.pi * 1000 * np.arange(y.shape[0]) / 16000.0)
    err = _rms(y[400:1200] - ideal[400:1200])
    print("8000 -> 16000, 1 kHz: rms error %.3f (bound 1.6)" % err)
    assert err <= 2 * 0.8
