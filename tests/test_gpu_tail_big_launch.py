"""The log-likelihood tail in launches the single-utterance entry cannot make (it walks an utterance in passes of 4 096
frames): designed logits (tests/tail_cases.py) through pk.FeatureScorer, which puts any number of rows into ONE launch.
With no splice context (L = R = 0) the feature dimension is the number of patterns, and frame t is one-hot at t mod P.

  * The stand-alone wave tail with iters >= 2: more than 8192 * per_wg rows in one launch (per_wg = 4 rows a workgroup,
    2 in the pair form above 4 096 columns), so a workgroup walks on to row r + 8192 * per_wg with the next rows
    prefetched into nv[] -- every row is compared with the predicted bits of its pattern, so row r and row r + step are
    both held.
  * The fused tail at 1 000 and 1 024 columns (C = 4: 8 column tiles need 48 row tiles = 6 144 rows in one launch), with
    the last row tile full and holding one row; neither width is eligible for the strip launch (8 column tiles, it needs
    more).  Bit-identical to the stand-alone wave tail on the same rows.

Still not covered: TailWaveKernel<..., LDS_PRIOR = true> needs more than 8 * 8192 * per_wg rows in one launch -- 262 144
for the four-row forms, which is the batch scorer's chunk size (a pass never holds more), and 131 072 rows of more than
4 096 columns for the pair form, over two gigabytes of log-likelihoods.  The fused route runs the same TailWaveLdsPrior
(test_gpu_tail_edges.py)."""
import numpy as np
import pytest

import pocketkaldi_amd as pk

import tail_cases as C
import tail_model as M

pytestmark = pytest.mark.gpu

STAND_ALONE = {"PK_MI355_FUSED_TAIL32": "1", "PK_MI355_FUSED_TAIL_MIN_TILES": "100000000"}
FUSED = {"PK_MI355_FUSED_TAIL32": "1", "PK_MI355_FUSED_TAIL_MIN_TILES": "384"}
WG_ROWS = 8192                                          # workgroups of a stand-alone launch at most


def per_wg(n):
    return 2 if M.wave_shape(n)[1] else 4


def model(monkeypatch, env, case, identity_first):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return pk.AcousticModel(C.layers(case, identity_first=identity_first), C.prior(case["n"], "varied"), 0, 0)


def one_launch(am, case, rows, scale=0.1):
    """`rows` one-hot frames as ONE utterance of a FeatureScorer: one pass of the layer stack, one launch of the tail."""
    fs = pk.FeatureScorer(am, 1, rows)
    assert rows <= 262144                                # the scorer's chunk: more rows would be several passes
    fs.set_features([C.features(case, rows)])
    fs.score(scale)
    out = fs.fetch(0).log_prob()
    fs.close()
    assert out.shape == (rows, case["n"])
    return out


# narrow and exact (C = 4), a clamped last chunk (6 of C = 8 chunks, the sixth partly filled), the pair form (C = 12, 17 chunks)
@pytest.mark.parametrize("n", [1024, 1501, 4097])
def test_stand_alone_wave_tail_second_iteration(n, monkeypatch):
    step = WG_ROWS * per_wg(n)
    rows = step + 5
    assert (M.wave_shape(n)[1], step) == ((True, 16384) if n > 4096 else (False, 32768))
    case = C.peaks_case(n)
    am = model(monkeypatch, STAND_ALONE, case, identity_first=False)
    got = one_launch(am, case, rows)
    am.close()
    where = "stand-alone TailWaveRows<C=%d, PAIR=%d, EXACT=%d>, %d rows in one launch" % (M.wave_shape(n) + (rows,))
    C.check(case, got, 0.1, "varied", "wave", where)    # every row: r < 5 and r + step are a workgroup's first and second iteration
    P = case["X"].shape[0]
    assert step % P != 0                                 # ... and hold different patterns


@pytest.mark.parametrize("rows", [6144, 6145])
@pytest.mark.parametrize("n", [1000, 1024])
def test_fused_tail_at_four_chunks(n, rows, monkeypatch):
    assert M.wave_shape(n) == (4, False, True)
    assert C.fused_route(rows, n) == "fused" and C.fused_route(6144 - 128, n) == "wave" and not C.strip_eligible(n)
    case = C.main_case(n)
    am = model(monkeypatch, FUSED, case, identity_first=True)
    got = one_launch(am, case, rows)
    am.close()
    where = "fused TailWaveRows<C=4>, n=%d, %d rows" % (n, rows)
    worst = C.check(case, got, 0.1, "varied", "wave", where)
    print("TAIL_BIG_LAUNCH_RATIO %s %.4f" % (where, worst))
    assert worst <= 1.0
    am = model(monkeypatch, STAND_ALONE, case, identity_first=True)
    alone = one_launch(am, case, rows)
    am.close()
    assert got.tobytes() == alone.tobytes(), where + ": differs from the stand-alone wave tail"
