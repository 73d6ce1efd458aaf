"""Delta features in C++.
  * tests/cpp/delta_test.cc: csrc/pk_delta.cc in a process of its own, plain and under ASan + UBSan -- the spec's
    refusals and range edges, T = 0 and T = 1, exactly sized buffers; the scale tables and delta rows it computes hash
    to the numpy restatement's (tests/delta_cases.py).
  * tests/cpp/deltas_example.cc: a 13-of-23 MFCC front-end, pocketkaldi::BatchScorer with a DeltaSpec in front of a 39-dim
    model; its front-end rows, first-layer rows and log-likelihood rows hash to Python's."""
import os
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import delta_cases as DC
import norm_cases as NC
from test_cpp_ark_features import fnv, weight
from test_cpp_stream import build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pocketkaldi_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
D = 97


def h(k):
    return (np.asarray(k, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)


@pytest.mark.parametrize("flavour", [
    "plain",
    pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                       reason="a GPU is present: sanitizer builds run on CPU machines only")),
])
def test_host_side_stand_alone(flavour):
    binary_path = os.path.join(REPO, "tests", "cpp", "delta_test_%s.bin" % flavour)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off"] + (SANITIZE if flavour == "sanitized" else []) +
                          [os.path.join(REPO, "tests", "cpp", "delta_test.cc"), os.path.join(CSRC, "pk_delta.cc"), os.path.join(CSRC, "pk_files.cc"),
                           "-o", binary_path])
    run = subprocess.run([binary_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-4000:]
    assert run.stderr == ""                                  # a sanitizer reports there
    out = run.stdout.splitlines()
    assert out[-1] == "delta_test ok"
    want = []
    for order, window in DC.SPECS:
        want.append("scales %d %d %s" % (order, window, fnv(DC.scale_table(order, window).tobytes())))
        for T in (0, 1, 2, 37, 130):
            x = ((h(np.arange(T * D) + 99) >> np.uint64(12)).astype(np.float64) / 1024.0 - 300.0).astype(np.float32).reshape(T, D)
            want.append("deltas %d %d %d %s" % (order, window, T, fnv(DC.add_deltas(x, order, window).tobytes())))
    assert out[:len(want)] == want


def test_deltas_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("deltas_example"), "--link-only"], text=True)


@pytest.mark.gpu
def test_deltas_example_equals_python():
    L, R, N = 2, 1, 16
    wav = os.path.join(REPO, "tests", "golden", "en-us-hello.wav")
    got = subprocess.run([build("deltas_example"), wav], capture_output=True, text=True)
    assert got.returncode == 0 and "deltas_example ok" in got.stdout, got.stdout + got.stderr
    fe = pk.FrontendSpec("mfcc", 23, 13, "povey", 20.0, 0.0, 22.0)
    deltas = pk.DeltaSpec()
    Db, Dm = fe.dim, deltas.dim(fe.dim)
    W = weight(np.arange(N * Dm * (L + R + 1))).reshape(N, Dm * (L + R + 1))
    b = weight(1000003 + np.arange(N))
    am = pk.AcousticModel([("linear", W, b), ("softmax",)], np.full(N, 1.0 / N, np.float32), L, R)
    g = np.zeros(Db + 1, np.float32)
    g[Db] = 1.0
    wave = pk.read_wav(wav)
    bs = pk.BatchScorer(am, g, 1, wave.shape[0] + 1, frontend=fe, deltas=deltas)
    bs.set_norm(pk.NormSpec("utterance", True, True))
    bs.set_waves([wave])
    bs.score(0.1)
    rows = bs.fetch_fbank(0)
    want = DC.add_deltas(NC.normalize(rows, "utterance", True, True)[0], 2, 2)
    assert NC.bits_equal(bs.fetch_cmvn(0), want)
    lines = ["frames %d base %d dim %d" % (rows.shape[0], Db, Dm), "features %s" % fnv(rows.tobytes()), "deltas %s" % fnv(want.tobytes()),
             "loglik %s" % fnv(bs.fetch(0).log_prob().tobytes())]
    assert got.stdout.splitlines()[:4] == lines
    bs.close()
    am.close()
