"""tests/cpp/stream_example.cc: the WAV in 100 ms chunks through pocketkaldi::OnlineScorer and
pocketkaldi::OnlineDecoder (include/pocketkaldi_amd.hpp).  Its final lines equal tests/cpp/gpu_decode_example.cc's
for the whole utterance."""
import os
import subprocess

import pytest

import pocketkaldi_amd as pk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")


def build(name):
    pk.lib()
    libdir = os.path.dirname(pk.lib_path())
    out = os.path.join(REPO, "tests", "cpp", name + ".bin")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp", name + ".cc"), "-o", out,
                           "-L", libdir, "-l:libpk_mi355.so", "-Wl,-rpath," + libdir])
    return out


def test_stream_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("stream_example"), "--link-only"], text=True)


@pytest.mark.gpu
@pytest.mark.parametrize("wav", ["en-us-hello.wav", "en-us-cat.wav"])
def test_stream_example_equals_gpu_decode_example(wav):
    from refmodel_text import DIR
    args = [os.path.join(DIR, "refmodel.conf"), os.path.join(G, wav), os.path.join(DIR, "wordloop.fst")]
    got = subprocess.run([build("stream_example")] + args, capture_output=True, text=True)
    assert got.returncode == 0 and "stream_example ok" in got.stdout, got.stdout + got.stderr
    want = subprocess.run([build("gpu_decode_example")] + args, capture_output=True, text=True)
    assert want.returncode == 0 and "gpu_decode_example ok" in want.stdout, want.stdout + want.stderr
    assert got.stdout.count("partial ") >= 3

    def fields(out):
        return {k: v for k, v in (l.split(": ", 1) for l in out.splitlines() if ": " in l and not l.startswith("partial"))}
    g, w = fields(got.stdout), fields(want.stdout)
    for k in ("frames", "hyp", "weight", "loglikelihood_per_frame"):
        assert g[k] == w[k], (k, g[k], w[k])
