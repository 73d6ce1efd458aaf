"""Delta features on a live slot in C++.
  * tests/cpp/stream_delta_test.cc: the frame accounting, the fresh-or-ring choice and the host streaming apply of
    csrc/pk_delta.h in a process of its own, plain and under ASan + UBSan; the streaming apply is held there to
    pk_mi355_deltas_apply on the whole matrix at every chunking, with a ring of exactly 2 M frames.
  * tests/cpp/stream_deltas_plan_test.cc: the deltas rows of the stream plan (csrc/pk_plan.cc), printed and compared with
    the lines written out here from the table of DESIGN.md.
  * The numpy restatement (tests/stream_delta_cases.py) against the batch rule's (tests/delta_cases.py) and the library's.
  * tests/cpp/online_deltas_example.cc compiles and links against the header."""
import os
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import delta_cases as DC
import stream_delta_cases as SD
from test_cpp_ark_features import fnv, weight
from test_cpp_stream import build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pocketkaldi_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
MODES = ["sliding", "none", "utterance", "speaker", "online"]
FLAVOURS = ["plain", pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                                          reason="a GPU is present: sanitizer builds run on CPU machines only"))]


def run_stand_alone(name, sources, flavour, flags=()):
    binary_path = os.path.join(REPO, "tests", "cpp", "%s_%s.bin" % (name, flavour))
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + list(flags) + (SANITIZE if flavour == "sanitized" else []) +
                          [os.path.join(REPO, "tests", "cpp", name + ".cc")] + [os.path.join(CSRC, s) for s in sources] + ["-o", binary_path])
    run = subprocess.run([binary_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-4000:]
    assert run.stderr == ""                                  # a sanitizer reports there
    return run.stdout.splitlines()


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_accounting_pick_and_streaming_apply_stand_alone(flavour):
    out = run_stand_alone("stream_delta_test", ["pk_delta.cc", "pk_files.cc"], flavour, ["-ffp-contract=off"])
    assert out == ["stream deltas %d %d: 96 cases" % s for s in ((1, 1), (2, 2), (3, 8))] + ["stream_delta_test ok"]


def plan_line(area, mode, n_front, n_back, max_m, chain_pushed):
    """The deltas rows of the table: one block per step, normaliser -> StreamDelta -> StreamFeatureLayout, never fused, the
    rows in the upload staging; SLIDING is the chain at every base dimension."""
    normaliser = {"sliding": "StreamCmvnChain", "none": "-"}.get(mode, "StreamNorm")
    blocks = []
    if area:
        blocks.append("[first x%d d_upload %s StreamDelta StreamFeatureLayout]" % (n_front + n_back, normaliser if max_m > 0 or chain_pushed > 0 else "-"))
    elif n_back > 0:
        blocks.append("[back x%d d_upload %s StreamDelta StreamFeatureLayout]" % (n_back, normaliser if chain_pushed > 0 else "-"))
    return "stream deltas area=%d %s front=%d back=%d m=%d chain=%d: front=%d%s" % (
        area, mode, n_front, n_back, max_m, chain_pushed, int(n_front > 0), "".join(" " + b for b in blocks))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_deltas_rows_of_the_stream_plan(flavour):
    out = run_stand_alone("stream_deltas_plan_test", ["pk_plan.cc"], flavour)
    want = [plan_line(area, mode, nf, nb, m, chain) for area in (0, 1) for mode in MODES for nf in ((0, 2) if area else (0,)) for nb in (0, 2)
            for m in ((0, 3) if nf else (0,)) for chain in (0, 3)]
    assert out == want + ["stream_deltas_plan_test ok"]
    assert not any("StreamCmvn " in line or line.endswith("StreamCmvn]") for line in out)      # nothing is fused


def test_numpy_restatement_is_the_batch_rule_at_every_chunking():
    rng = np.random.default_rng(1)
    for order, window in ((1, 1), (2, 2), (3, 8)):
        M = order * window
        spec = pk.DeltaSpec(order, window)
        for T in (0, 1, 2, M, M + 1, 2 * M, 2 * M + 1, 70):
            x = DC.wide(T, 3, 5 + T) if T else np.zeros((0, 3), np.float32)
            want = DC.add_deltas(x, order, window)
            assert DC.bits_equal(pk.add_deltas(x, spec), want) or T == 0
            for how in SD.CHUNKINGS:
                for delay in (0, 1, 2):
                    chunks = SD.chunks_of(T, how, rng)
                    y, made = SD.stream_add_deltas(x, order, window, chunks, delay)
                    assert DC.bits_equal(y, want), (order, window, T, how, delay)
                    assert sum(made) == T and len(made) == max(len(chunks), 1) + delay


def test_accounting_restated():
    for M, R in ((1, 0), (4, 1), (24, 5)):
        n = nd = a = 0
        for _ in range(3 * M + R + 2):
            n += 1
            nd, b = SD.advance(n, nd, a, M, R, False)
            assert (nd, b) == (max(n - M, 0), max(n - M - R, 0))
            a = b
        assert SD.advance(n, nd, a, M, R, True) == (n, n) and n - a == M + R == SD.lookahead(M, 1, R)
        assert SD.advance(0, 0, 0, M, R, True) == (0, 0)


def test_online_deltas_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("online_deltas_example"), "--link-only"], text=True)


@pytest.mark.gpu
def test_online_deltas_example_equals_python():
    L, R, N = 2, 1, 16
    wav = os.path.join(REPO, "tests", "golden", "en-us-hello.wav")
    got = subprocess.run([build("online_deltas_example"), wav], capture_output=True, text=True)
    assert got.returncode == 0 and "online_deltas_example ok" in got.stdout, got.stdout + got.stderr
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
    bs.set_waves([wave])
    bs.score(0.1)
    rows = bs.fetch(0).log_prob()
    assert got.stdout.splitlines()[:2] == ["frames %d base %d dim %d" % (rows.shape[0], Db, Dm), "loglik %s" % fnv(rows.tobytes())]
    bs.close()
    am.close()
