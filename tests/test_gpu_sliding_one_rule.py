"""The four sliding-CMVN kernels against one expected value.  Raw rows of 700 frames -- past the
600-frame window, no multiple of 8 or 64 -- go to a FeatureScorer and, in uneven pushes of which the last straddles
frame 600, to an OnlineFeatureScorer.  At D = 40 these run CmvnKernel and StreamCmvnKernel, at D = 41 CmvnChainKernel and
StreamCmvnChainKernel.  The batch rows after CMVN must be the chunk rule's (tests/cmvn_any_cases.py: the oracle, 40
columns at a time) and every online log-likelihood row the batch row, bit for bit."""
import numpy as np
import pytest

import pocketkaldi_amd as pk

import cmvn_any_cases as CA
from test_cpp_ark_features import weight
from test_gpu_stream_features import run_jobs

pytestmark = pytest.mark.gpu

T, L, R, N = 700, 2, 1, 16
PUSHES = [1, 7, 64, 333, T - 405]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("D", [40, 41])
def test_batch_and_online_sliding_kernels_meet_the_chunk_rule(D):
    W = weight(np.arange(N * D * (L + R + 1))).reshape(N, D * (L + R + 1))
    am = pk.AcousticModel([("linear", W, weight(1000003 + np.arange(N))), ("softmax",)], np.full(N, 1.0 / N, np.float32), L, R)
    g, x = CA.stats_for(D), CA.features(T, D, 23)
    want = CA.cmvn_any(g, x)
    fs = pk.FeatureScorer(am, 1, T, global_stats=g)
    fs.set_features([x], "raw")
    fs.score(0.1)
    assert bits_equal(fs.fetch_cmvn(0), want), "D=%d: the batch kernel's rows are not the chunk rule's" % D
    rows = fs.fetch(0).log_prob()
    assert rows.shape == (T, N) and np.isfinite(rows).all()
    sc = pk.OnlineFeatureScorer(am, 1, T, global_stats=g)
    (got,) = run_jobs(sc, [{"slot": 0, "kind": "raw", "data": x, "chunks": PUSHES, "start": 0, "close_with_last": False}])
    assert bits_equal(got, rows), "D=%d: the online rows are not the batch rows" % D
    sc.destroy()
    fs.close()
    am.close()
