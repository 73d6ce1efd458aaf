"""tests/cpp/ark_features_example.cc: the entries of a Kaldi archive as raw 80-dim features, 10 frames a step, through a
features-only pocketkaldi::OnlineScorer made with the 81 statistics of a Kaldi global CMVN file, read by
pocketkaldi::ArkReader (include/pocketkaldi_amd.hpp).  Its rows hash to pk.FeatureScorer's RAW rows on the same model."""
import struct
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import cmvn_any_cases as CA
from test_cpp_stream import build


def test_ark_features_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("ark_features_example"), "--link-only"], text=True)


def fnv(data):
    h = 14695981039346656037
    for byte in bytes(data):
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def weight(k):
    k = np.asarray(k, np.uint64)
    return ((((k * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)).astype(np.float32) / np.float32(65536.0)
            - np.float32(0.5)) * np.float32(0.05)


@pytest.mark.gpu
def test_ark_features_example_equals_the_feature_scorer(tmp_path):
    D, L, R, N = 80, 2, 1, 16
    feats = {"short": CA.features(7, D, 900), "none": CA.features(0, D, 901), "long": CA.features(650, D, 902)}
    g = CA.stats_for(D)
    ark, stats = str(tmp_path / "feats.ark"), str(tmp_path / "cmvn.stats")
    with open(ark, "wb") as f:
        for key, x in feats.items():
            f.write(key.encode() + b" \0BFM " + struct.pack("<BiBi", 4, x.shape[0], 4, D) + x.astype("<f4").tobytes())
    with open(stats, "wb") as f:                              # 2 x (D + 1) doubles: sums and count, then sums of squares
        m = np.zeros((2, D + 1))
        m[0] = g.astype(np.float64)
        f.write(b"\0BDM " + struct.pack("<BiBi", 4, 2, 4, D + 1) + m.astype("<f8").tobytes())
    assert np.array_equal(pk.kaldi_global_stats(stats), g)
    got = subprocess.run([build("ark_features_example"), ark, stats], capture_output=True, text=True)
    assert got.returncode == 0 and "ark_features_example ok" in got.stdout, got.stdout + got.stderr
    W = weight(np.arange(N * D * (L + R + 1))).reshape(N, D * (L + R + 1))
    b = weight(1000003 + np.arange(N))
    am = pk.AcousticModel([("linear", W, b), ("softmax",)], np.full(N, 1.0 / N, np.float32), L, R)
    fs = pk.FeatureScorer(am, len(feats), sum(x.shape[0] for x in feats.values()), global_stats=g)
    fs.set_features(list(feats.values()), "raw")
    fs.score(0.1)
    want = ["entry %s frames %d loglik %s" % (key, x.shape[0], fnv(fs.fetch(u).log_prob().tobytes() if x.shape[0] else b""))
            for u, (key, x) in enumerate(feats.items())]
    assert got.stdout.splitlines()[:3] == want
    fs.close()
    am.close()
