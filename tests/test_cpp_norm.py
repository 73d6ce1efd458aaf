"""The normalisation spec in C++.
  * tests/cpp/norm_test.cc: csrc/pk_norm.cc in a process of its own, plain and under ASan + UBSan -- the spec's
    refusals, counts of 0, -1, NaN and inf, the variance floor, records for 1 and 200 utterances; the tables it
    finalises hash to the numpy restatement's (tests/norm_cases.py); and the sliding rule's two steps of pk_norm.h,
    which the CMVN kernels compile, walked over 700 frames at D = 40 and 41: the rows hash to the oracle's.
  * tests/cpp/norm_example.cc: an 80-bin front-end, pocketkaldi::BatchScorer::SetNorm(NormSpec::Utterance(true, true));
    its normalised rows, statistics and log-likelihood rows hash to Python's."""
import os
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import cmvn_any_cases as CA
import norm_cases as NC
from test_cpp_ark_features import fnv, weight
from oracle import oracle as O
from test_cpp_stream import build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pocketkaldi_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
D = 97


def h(k):
    return (np.asarray(k, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)


def records(U):
    """norm_test.cc's records, restated."""
    u, d = np.meshgrid(np.arange(U), np.arange(D), indexing="ij")
    k = 1000 * u + d
    n = 50.0 + 100.0 * (u % 7)
    m = (h(k) >> np.uint64(8)).astype(np.float64) / 65536.0 - 128.0
    v = 0.01 + (h(k + 7777) >> np.uint64(16)).astype(np.float64) / 4096.0
    rec = np.zeros((U, 2, D + 1))
    rec[:, 0, :D] = m * n
    rec[:, 1, :D] = (m * m + v) * n
    rec[:, 0, D] = n[:, 0]
    return rec


def sliding_input(dim, T=700):
    """norm_test.cc's sliding input, restated: values around 3, column dim // 2 around 1e4 (the two kinds of
    cmvn_any_cases.features), and cmvn_any_cases.stats_for's statistics."""
    t, d = np.meshgrid(np.arange(T), np.arange(dim), indexing="ij")
    x = (h(t * dim + d + 31337) >> np.uint64(8)).astype(np.float64) / 16777216.0 * 30.0 - 12.0
    x[:, dim // 2] += CA.BIG_COLUMN_MEAN
    return CA.stats_for(dim), x.astype(np.float32)


@pytest.mark.parametrize("dim", [40, 41])
def test_sliding_input_tells_a_float_only_sum_from_the_double_step(dim):
    """As test_cmvn_any_host.py shows for its input: the restated chain with the widen / narrow step IS the oracle on the
    program's input, and without it both kinds of column differ once the window slides."""
    g, x = sliding_input(dim)
    want = CA.cmvn_any(g, x)
    assert want.tobytes() == CA.restated_chain(g, x, True).tobytes()
    differs = CA.restated_chain(g, x, False).view(np.uint32) != want.view(np.uint32)
    assert not differs[:CA.WINDOW].any()
    per_column = differs.sum(axis=0)
    print("frames on which the float-only chain differs: big column %d, the others %d..%d"
          % (per_column[dim // 2], np.delete(per_column, dim // 2).min(), np.delete(per_column, dim // 2).max()))
    assert per_column[dim // 2] >= 10 and np.delete(per_column, dim // 2).min() >= 10


@pytest.mark.parametrize("flavour", [
    "plain",
    pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                       reason="a GPU is present: sanitizer builds run on CPU machines only")),
])
def test_host_side_stand_alone(flavour):
    binary_path = os.path.join(REPO, "tests", "cpp", "norm_test_%s.bin" % flavour)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off"] + (SANITIZE if flavour == "sanitized" else []) +
                          [os.path.join(REPO, "tests", "cpp", "norm_test.cc"), os.path.join(CSRC, "pk_norm.cc"), os.path.join(CSRC, "pk_files.cc"),
                           os.path.join(CSRC, "pk_tables.cc"), "-o", binary_path])
    run = subprocess.run([binary_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-4000:]
    assert run.stderr == ""                                  # a sanitizer reports there
    out = run.stdout.splitlines()
    assert out[-1] == "norm_test ok"
    want = []
    for U in (1, 200):
        rec = records(U)
        want.append("records %d %s" % (U, fnv(rec.tobytes())))
        for means, variances in NC.SWITCHES:
            table = np.stack([np.stack(NC.finalize(rec[u], means, variances)) for u in range(U)])
            assert table.shape == (U, 2, D) and table.dtype == np.float32 and np.isfinite(table).all()
            want.append("table %d %d %d %s" % (U, means, variances, fnv(table.tobytes())))
    x = ((h(np.arange(37 * 5) + 99) >> np.uint64(12)).astype(np.float64) / 1024.0 - 300.0).astype(np.float32).reshape(37, 5)
    y, rec = NC.normalize(x, "utterance", True, True)
    want += ["matrix %s" % fnv(x.tobytes()), "utterance %s %s" % (fnv(y.tobytes()), fnv(rec.tobytes()))]
    for dim in (40, 41):                                     # the sliding steps against the oracle
        g, x = sliding_input(dim)
        y = CA.cmvn_any(g, x)
        if dim == 40:
            assert y.tobytes() == O.cmvn(g, x).tobytes()
        want.append("sliding %d %s %s" % (dim, fnv(x.tobytes()), fnv(y.tobytes())))
    assert out[:len(want)] == want


def test_norm_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("norm_example"), "--link-only"], text=True)


@pytest.mark.gpu
def test_norm_example_equals_python():
    Dm, L, R, N = 80, 2, 1, 16
    wav = os.path.join(REPO, "tests", "golden", "en-us-hello.wav")
    got = subprocess.run([build("norm_example"), wav], capture_output=True, text=True)
    assert got.returncode == 0 and "norm_example ok" in got.stdout, got.stdout + got.stderr
    spec = pk.FrontendSpec("fbank", 80, None, "povey", 20.0, 0.0)
    W = weight(np.arange(N * Dm * (L + R + 1))).reshape(N, Dm * (L + R + 1))
    b = weight(1000003 + np.arange(N))
    am = pk.AcousticModel([("linear", W, b), ("softmax",)], np.full(N, 1.0 / N, np.float32), L, R)
    g = np.zeros(Dm + 1, np.float32)
    g[Dm] = 1.0
    wave = pk.read_wav(wav)
    bs = pk.BatchScorer(am, g, 1, wave.shape[0] + 1, frontend=spec)
    bs.set_norm(pk.NormSpec("utterance", True, True))
    bs.set_waves([wave])
    bs.score(0.1)
    rows = bs.fetch_fbank(0)
    want, rec = NC.normalize(rows, "utterance", True, True)
    assert NC.bits_equal(bs.fetch_cmvn(0), want) and NC.bits_equal(bs.norm_stats(0), rec)
    lines = ["frames %d dim %d" % (rows.shape[0], Dm), "normalized %s" % fnv(want.tobytes()), "stats %s" % fnv(rec.tobytes()),
             "loglik %s" % fnv(bs.fetch(0).log_prob().tobytes())]
    assert got.stdout.splitlines()[:4] == lines
    bs.close()
    am.close()
