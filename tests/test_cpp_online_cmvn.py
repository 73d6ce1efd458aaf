"""Online CMVN in C++.
  * tests/cpp/online_cmvn_test.cc: csrc/pk_norm.cc in a process of its own, plain and under ASan + UBSan -- the spec's
    refusals, counts of 0, -1, NaN and inf, W = 1, windows that wrap and one that never fills; its outputs and window
    states hash to the numpy restatement's (tests/online_cmvn_cases.py).
  * tests/cpp/online_norm_example.cc: an 80-bin front-end, pocketkaldi::BatchScorer::SetNorm(OnlineCmvnSpec(8, 3, 2,
    true), global statistics), without and with a speaker record; its normalised rows and log-likelihood rows hash to
    Python's.  The program itself then feeds the wave to pocketkaldi::OnlineScorer under the same spec, 100 ms a step,
    and fails unless the live rows are the batch rows bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import online_cmvn_cases as OC
from test_cpp_ark_features import fnv, weight
from test_cpp_norm import CSRC, REPO, SANITIZE, h
from test_cpp_stream import build

D, T = 5, 37


def record(seed, n):
    """online_cmvn_test.cc's records, restated."""
    d = np.arange(D)
    m = (h(d + seed) >> np.uint64(8)).astype(np.float64) / 65536.0 - 128.0
    v = 0.01 + (h(d + seed + 7777) >> np.uint64(16)).astype(np.float64) / 4096.0
    rec = np.zeros((2, D + 1))
    rec[0, :D], rec[1, :D], rec[0, D] = m * n, (m * m + v) * n, n
    return rec


@pytest.mark.parametrize("flavour", [
    "plain",
    pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                       reason="a GPU is present: sanitizer builds run on CPU machines only")),
])
def test_host_side_stand_alone(flavour):
    binary_path = os.path.join(REPO, "tests", "cpp", "online_cmvn_test_%s.bin" % flavour)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off"] + (SANITIZE if flavour == "sanitized" else []) +
                          [os.path.join(REPO, "tests", "cpp", "online_cmvn_test.cc"), os.path.join(CSRC, "pk_norm.cc"), os.path.join(CSRC, "pk_files.cc"),
                           "-o", binary_path])
    run = subprocess.run([binary_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-4000:]
    assert run.stderr == ""                                  # a sanitizer reports there
    out = run.stdout.splitlines()
    assert out[-1] == "online_cmvn_test ok"
    x = ((h(np.arange(T * D) + 99) >> np.uint64(12)).astype(np.float64) / 1024.0 - 300.0).astype(np.float32).reshape(T, D)
    glob, spk = record(5000, 300.0), record(9000, 37.0)
    want = ["matrix %s" % fnv(x.tobytes()), "records %s %s" % (fnv(glob.tobytes()), fnv(spk.tobytes()))]
    for W in (1, 2, 8, 37, 50):
        for variances in (0, 1):
            for speaker in (0, 1):
                y, state = OC.online_cmvn(x, W, 3, 2, bool(variances), glob, spk if speaker else None)
                want.append("rule %d %d %d %s %s" % (W, variances, speaker, fnv(y.tobytes()), fnv(state.tobytes())))
    assert out[:len(want)] == want


def test_online_norm_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("online_norm_example"), "--link-only"], text=True)


@pytest.mark.gpu
def test_online_norm_example_equals_python():
    Dm, L, R, N = 80, 2, 1, 16
    wav = os.path.join(REPO, "tests", "golden", "en-us-hello.wav")
    got = subprocess.run([build("online_norm_example"), wav], capture_output=True, text=True)
    assert got.returncode == 0 and "online_norm_example ok" in got.stdout, got.stdout + got.stderr
    spec = pk.FrontendSpec("fbank", 80, None, "povey", 20.0, 0.0)
    W = weight(np.arange(N * Dm * (L + R + 1))).reshape(N, Dm * (L + R + 1))
    b = weight(1000003 + np.arange(N))
    am = pk.AcousticModel([("linear", W, b), ("softmax",)], np.full(N, 1.0 / N, np.float32), L, R)
    g = np.zeros(Dm + 1, np.float32)
    g[Dm] = 1.0

    def rec(mean, var, n):
        r = np.zeros((2, Dm + 1))
        r[0, :Dm], r[1, :Dm], r[0, Dm] = mean * n, (mean * mean + var) * n, n
        return r

    glob, spk = rec(10.0, 4.0, 300.0), rec(12.0, 2.0, 37.0)
    wave = pk.read_wav(wav)
    bs = pk.BatchScorer(am, g, 1, wave.shape[0] + 1, frontend=spec)
    bs.set_norm(pk.OnlineCmvnSpec(8, 3, 2, True), glob)
    lines = []
    for speaker in (0, 1):
        if speaker:
            bs.set_speaker_stats([spk])
        bs.set_waves([wave])
        bs.score(0.1)
        rows = bs.fetch_fbank(0)
        want, _ = OC.online_cmvn(rows, 8, 3, 2, True, glob, spk if speaker else None)
        assert bs.fetch_cmvn(0).tobytes() == want.tobytes()
        if not speaker:
            lines.append("frames %d dim %d" % (rows.shape[0], Dm))
        lines += ["normalized %d %s" % (speaker, fnv(want.tobytes())), "loglik %d %s" % (speaker, fnv(bs.fetch(0).log_prob().tobytes()))]
    assert got.stdout.splitlines()[:5] == lines
    bs.close()
    am.close()
