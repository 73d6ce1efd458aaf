"""The cases of tests/test_gpu_grid_walks.py (tests/grid_walk_cases.py), checked without a GPU: the caps still stand in
the launchers' sources where the cases assume them, the pools' periods never bring a unit and its partner one cap
further to the same content or parameter, every case reaches past its cap, the comparison tells each of the three wrong
kernels from the expectation in every case, and no case needs 1 GiB of device memory."""
import os

import numpy as np
import pytest

import grid_walk_cases as GW

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pocketkaldi_amd", "csrc")
NAMES = sorted(GW.CASES)


def test_the_caps_stand_in_the_launchers_sources():
    for name, text, count in GW.SOURCE_PINS:
        src = open(os.path.join(CSRC, name)).read()
        assert src.count(text) == count, ("%s states %r %d times, not %d: a launch cap has moved -- update the caps and the shapes of "
                                          "tests/grid_walk_cases.py so that the second grid walk is still reached" % (name, text, src.count(text), count))


def test_the_memory_formulas_stand_in_the_create_path():
    for name, text, count in GW.FORMULA_PINS:
        src = open(os.path.join(CSRC, name)).read()
        assert src.count(text) == count, "%s no longer states %r: bring core_bytes of tests/grid_walk_cases.py in line with the create path" % (name, text)


def test_the_pool_periods_are_coprime_to_the_caps():
    # (the resample case has no per-item parameter: its periods are the 7 waves of the pool and the 6 of them that are items)
    for cap, periods in ((GW.UTT_CAP, (GW.POOL, GW.PARAMS)), (GW.RESAMPLE_ITEMS_CAP, (GW.POOL, GW.Resample.item_period))):
        for period in periods:
            assert cap % period != 0 and (cap + 1) % period != 0, (cap, period)
    assert GW.Resample.param_period == 0
    assert GW.LAYER_LINES_CAP % GW.ROWS_POOL != 0 and (GW.LAYER_LINES_CAP + 1) % GW.ROWS_POOL != 0
    # the lengths: 0, 1, 2, 3 and 5 frames, below and above the context; the unit at the cap is the empty one, so the
    # `continue` of an empty utterance is taken on the second turn, and a unit of several frames follows it
    assert {0, 1, 2, 3, 5} <= set(GW.LENGTHS) and min(GW.LENGTHS) < GW.LEFT + GW.RIGHT < max(GW.LENGTHS)
    assert GW.LENGTHS[GW.UTT_CAP % GW.POOL] == 0 and GW.LENGTHS[(GW.UTT_CAP + 1) % GW.POOL] > GW.LEFT + GW.RIGHT
    assert {0, 399, 400, 560} <= set(GW.AUDIO_SAMPLES) and GW.AUDIO_SAMPLES[GW.UTT_CAP % GW.POOL] == 0
    rates = {rate for rate, _ in GW.RESAMPLE_POOL}
    assert {8000, 16000, 44100} <= rates


@pytest.mark.parametrize("name", NAMES)
def test_every_case_reaches_past_its_cap(name):
    c = GW.case(name)
    T = c.unit_lengths()
    assert T.shape == (c.n_units,)
    late = c.late_units()
    assert len(late) >= 2 and all(0 <= u < c.n_units and 0 <= src < c.n_units and src != u for u, src in late)
    if name == "row_walk":
        assert 200000 < c.n_units <= GW.CHUNK and c.n_units > c.cap + c.cap // 4           # one pass, a third of it in the second turn
        assert sum(f.shape[0] for f in c.utterances()) == c.n_units
    elif name == "resample":
        items = [u for u in range(c.n_units) if GW.RESAMPLE_POOL[u % GW.POOL][0] != 16000]
        assert len(items) == GW.RESAMPLE_ITEMS_CAP + 2 and [u for u, _ in late] == items[GW.RESAMPLE_ITEMS_CAP:]
        assert all(T[u] in (1, 2) for u in range(GW.POOL))                                 # one or two frames after conversion
    elif name in GW.LIVE:
        # a step makes a record only for a slot with something new: every slot pushes, so both steps (the push, and the close
        # that releases the frames held back) have a record per slot, and the records past the cap are the first slots
        assert c.n_units == GW.UTT_CAP + 2 and T.min() >= 1 and c.records(T) > GW.UTT_CAP
        assert late == [(1, GW.UTT_CAP + 1), (0, GW.UTT_CAP)]
        assert all(u % GW.POOL != src % GW.POOL for u, src in late)                         # (another content, by record index too)
    else:
        assert c.n_units == GW.UTT_CAP + 2 and T[GW.UTT_CAP] == 0 and T[GW.UTT_CAP + 1] > 0
        assert T.sum() <= GW.CHUNK                                                         # one pass
    assert len(c.table()) <= 77 or name == "row_walk"


@pytest.mark.parametrize("name", NAMES)
def test_the_expectation_is_assembled_from_the_pairs(name):
    """Spot units on both sides of the cap: the rows at the unit's offset are its (content, parameter) pair's."""
    c = GW.case(name)
    rows, T = c.expected()
    assert rows.shape == (int(T.sum()), c.num_pdfs) and rows.dtype == np.float32
    first = np.concatenate([[0], np.cumsum(T)])
    cp, pp = c.periods()
    for u in (0, 1, cp, c.cap - 1, c.cap, c.cap + 1, c.n_units - 1):
        want = c.table()[u % GW.ROWS_POOL][None, :] if name == "row_walk" else c.table()[(u % cp) * pp + u % pp]
        assert GW.same(rows[first[u]:first[u + 1]], want), (name, u)
    if name != "row_walk":
        assert np.isfinite(rows).all()
    else:
        assert np.isnan(rows).any() and np.isfinite(rows).any()


@pytest.mark.parametrize("name", NAMES)
def test_every_wrong_kernel_is_told_from_the_expectation(name):
    c = GW.case(name)
    rows, T = c.expected()
    first = np.concatenate([[0], np.cumsum(T)])
    at = first[min(u for u, _ in c.late_units())]
    assert tuple(c.variants) == (("unprocessed", "wrapped", "twice") if name == "row_walk" else ("unprocessed", "wrapped"))
    for which in c.variants:
        wrong = c.variant(which)
        assert wrong.shape == rows.shape
        assert GW.same(wrong[:at], rows[:at]), (name, which)                  # (the first turn is the right one)
        differing = (wrong.view(np.uint32) != rows.view(np.uint32)) & ~(np.isnan(wrong) & np.isnan(rows))
        assert differing.any() and not GW.same(wrong, rows), "%s: the comparison cannot see the %s kernel" % (name, which)


@pytest.mark.parametrize("name", NAMES)
def test_every_case_fits_a_gibibyte(name):
    c = GW.case(name)
    for live in ((False, True) if name in GW.LIVE else (False,)):
        b = c.device_bytes(live=live)
        assert 0 < b < 2 ** 30, (name, live, b)


def test_each_kind_alone_is_a_case_too():
    for kind in GW.ELEMENTWISE:
        c = GW.RowWalk((kind,), pnorm=False)
        rows, _ = c.expected()
        assert rows.shape == (c.n_units, 6)
        for which in c.variants:
            assert not GW.same(c.variant(which), rows), (kind, which)
