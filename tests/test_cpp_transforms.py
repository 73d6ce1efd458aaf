"""Feature transforms in C++.
  * tests/cpp/transform_test.cc: csrc/pk_transform.cc in a process of its own, plain and under ASan + UBSan -- the spec's
    refusals and range edges, the widest matrix in a buffer of exactly its size, T = 0 and T = 1, the kernel's matrix
    layout, exactly sized inputs and outputs; the rows it computes hash to the numpy restatement's
    (tests/transform_cases.py).
  * tests/cpp/transform_plan_test.cc: csrc/pk_plan.cc the same two ways -- the batch plan of a transform object over
    source x deltas x global matrix or not x matrices handed over or not x mode, against lines written out here from the
    table of DESIGN.md section 25."""
import os
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import transform_cases as XC
from test_cpp_ark_features import fnv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pocketkaldi_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FLAVOURS = ["plain",
            pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                               reason="a GPU is present: sanitizer builds run on CPU machines only"))]


def h(k):
    return (np.asarray(k, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)


def cpp_input(n):
    return ((h(np.arange(n) + 99) >> np.uint64(12)).astype(np.float64) / 1024.0 - 300.0).astype(np.float32)


def cpp_matrix(n):
    return ((h(np.arange(n) + 7) >> np.uint64(12)).astype(np.float64) / 1048576.0 - 0.5).astype(np.float32)


def run_stand_alone(name, flavour, sources):
    binary_path = os.path.join(REPO, "tests", "cpp", "%s_%s.bin" % (name, flavour))
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off"] + (SANITIZE if flavour == "sanitized" else []) +
                          [os.path.join(REPO, "tests", "cpp", name + ".cc")] + [os.path.join(CSRC, s) for s in sources] + ["-o", binary_path])
    run = subprocess.run([binary_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-4000:]
    assert run.stderr == ""                                  # a sanitizer reports there
    out = run.stdout.splitlines()
    assert out[-1] == name + " ok"
    return out


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_host_side_stand_alone(flavour):
    out = run_stand_alone("transform_test", flavour, ["pk_transform.cc", "pk_files.cc"])
    Dp, L, R, T = 512, 7, 9, 3
    K = (L + R + 1) * Dp
    want = ["widest %s" % fnv(XC.transform(cpp_input(T * Dp).reshape(T, Dp), cpp_matrix(K + 1).reshape(1, K + 1), L, R).tobytes())]
    for Dp, L, R, rows, affine in XC.HOST_SPECS:
        cols = (L + R + 1) * Dp + (1 if affine else 0)
        m = cpp_matrix(rows * cols).reshape(rows, cols)
        for T in (0, 1, 2, 9, 33):
            y = XC.transform(cpp_input(T * Dp).reshape(T, Dp), m, L, R)
            want.append("transform %d %d %d %d %d %d %s" % (Dp, L, R, rows, affine, T, fnv(y.tobytes())))
    assert out[:len(want)] == want


# The table of DESIGN.md section 25, a transform object with statistics and a 13-dim front-end spec.  The normaliser at
# Db = 13 (what it is called, and whether it exists: mode none reads the raw rows as they are):
NORMALISER = {"sliding": "CmvnChain", "none": None, "utterance": "Norm", "speaker": "Norm", "online": "OnlineCmvn"}
BITS = {"d_raw": 1, "d_feats": 2, "d_delta": 4, "d_xform": 32, "d_uxform": 64}


def expected_plan_lines():
    lines = []
    for source in ("waves", "raw", "normalized"):
        for deltas in (0, 1):
            for glob in (0, 1):
                for utt in (0, 1):
                    for mode in ("sliding", "none", "utterance", "speaker", "online"):
                        into = 39 if deltas else 13
                        D = 40 if glob else into
                        steps, used = [], set()
                        if source == "normalized":                  # past every stage: the layout alone
                            steps.append("FeatureLayout(feats->Yt@%d)" % D)
                        else:
                            if source == "waves":
                                steps.append("front:FbankAny(-->d_raw@13)")
                            rows = "d_raw"
                            used.add(rows)
                            if NORMALISER[mode]:
                                steps.append("%s(d_raw->d_feats@13)" % NORMALISER[mode])
                                rows = "d_feats"
                                used.add(rows)
                            for present, stage, out, dim in ((deltas, "Delta", "d_delta", 13), (glob, "Transform", "d_xform", into),
                                                             (utt, "UttTransform", "d_uxform", D)):
                                if present:
                                    steps.append("%s(%s->%s@%d)" % (stage, rows, out, dim))
                                    rows = out
                                used.add(rows)
                            steps.append("FeatureLayout(%s->Yt@%d)" % (rows, D))
                        lines.append("batch %s deltas=%d global=%d utt=%d %s: %s | buffers=%d"
                                     % (source, deltas, glob, utt, mode, " ".join(steps), sum(BITS[r] for r in used)))
    lines.append("fused transform=0 plain=1")
    lines.append("plain utt=1: 2 steps, buffers=3")
    return lines


def test_transforms_example_compiles_and_links():
    """tests/cpp/transforms_example.cc over include/pocketkaldi_amd.hpp; tests/test_gpu_recognize_transforms.py runs it."""
    from test_cpp_stream import build
    assert "pk_mi355" in subprocess.check_output([build("transforms_example"), "--link-only"], text=True)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_transform_plan_stand_alone(flavour):
    out = run_stand_alone("transform_plan_test", flavour, ["pk_plan.cc"])
    want = expected_plan_lines()
    assert len(want) == 3 * 2 * 2 * 2 * 5 + 2
    assert out[:-1] == want
