"""tests/cpp/frontend_example.cc: a wave through pocketkaldi::BatchScorer's front-end constructor -- an 80-bin
Povey-window fbank in front of an 80-dim model, with the 81 statistics of a Kaldi global CMVN file -- and through
pocketkaldi::Frontend (include/pocketkaldi_amd.hpp).  Its feature rows hash to the numpy restatement's and its
log-likelihood rows to pk.FeatureScorer's RAW rows on those features."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk
from oracle import oracle as O

import cmvn_any_cases as CA
import frontend_any_cases as FA
from test_cpp_ark_features import fnv, weight
from test_cpp_stream import build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frontend_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("frontend_example"), "--link-only"], text=True)


@pytest.mark.gpu
def test_frontend_example_equals_the_restatement_and_the_feature_scorer(tmp_path):
    D, L, R, N = 80, 2, 1, 16
    wav = os.path.join(REPO, "tests", "golden", "en-us-hello.wav")
    g = CA.stats_for(D)
    stats = str(tmp_path / "cmvn.stats")
    with open(stats, "wb") as f:                              # 2 x (D + 1) doubles: sums and count, then sums of squares
        m = np.zeros((2, D + 1))
        m[0] = g.astype(np.float64)
        f.write(b"\0BDM " + struct.pack("<BiBi", 4, 2, 4, D + 1) + m.astype("<f8").tobytes())
    got = subprocess.run([build("frontend_example"), wav, stats], capture_output=True, text=True)
    assert got.returncode == 0 and "frontend_example ok" in got.stdout, got.stdout + got.stderr
    spec = pk.FrontendSpec("fbank", 80, None, "povey", 20.0, 0.0)
    rows = FA.frontend_any(O.wav_read(wav), spec, pk.frontend_tables(spec))
    W = weight(np.arange(N * D * (L + R + 1))).reshape(N, D * (L + R + 1))
    b = weight(1000003 + np.arange(N))
    am = pk.AcousticModel([("linear", W, b), ("softmax",)], np.full(N, 1.0 / N, np.float32), L, R)
    fs = pk.FeatureScorer(am, 1, rows.shape[0], global_stats=g)
    fs.set_features([rows], "raw")
    fs.score(0.1)
    want = ["frames %d dim %d" % (rows.shape[0], D), "features %s" % fnv(rows.tobytes()), "loglik %s" % fnv(fs.fetch(0).log_prob().tobytes())]
    assert got.stdout.splitlines()[:3] == want
    fs.close()
    am.close()
