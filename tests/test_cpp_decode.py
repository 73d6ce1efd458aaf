"""tests/cpp/gpu_decode_example.cc: pk_process with both halves on the GPU through the C++ mirror
(pocketkaldi::Fst / pocketkaldi::Decoder, include/pocketkaldi_amd.hpp).  Its output equals
tests/cpp/process_example.cc's, which runs the reference's own decoder over the same log-likelihoods."""
import os
import subprocess

import pytest

import pocketkaldi_amd as pk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
DECLIB = os.path.join(REPO, "oracle", "_ref", "libpkref_decoder.so")


def build():
    pk.lib()
    libdir = os.path.dirname(pk.lib_path())
    out = os.path.join(REPO, "tests", "cpp", "gpu_decode_example.bin")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp", "gpu_decode_example.cc"), "-o", out,
                           "-L", libdir, "-l:libpk_mi355.so", "-Wl,-rpath," + libdir])
    return out


def test_gpu_decode_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build(), "--link-only"], text=True)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(DECLIB), reason="oracle/_ref/libpkref_decoder.so not built")
@pytest.mark.parametrize("wav", ["en-us-hello.wav", "en-us-cat.wav"])
@pytest.mark.parametrize("softmax", ["reference", "stable"])
def test_gpu_decode_example_equals_process_example(wav, softmax):
    from refmodel_text import DIR
    from test_gpu_decoder import build_example
    args = [os.path.join(DIR, "refmodel.conf"), os.path.join(G, wav), os.path.join(DIR, "wordloop.fst")]
    args += ["--reference-softmax"] if softmax == "reference" else []
    got = subprocess.run([build()] + args, capture_output=True, text=True)
    assert got.returncode == 0 and "gpu_decode_example ok" in got.stdout, got.stdout + got.stderr
    want = subprocess.run([build_example()] + args, capture_output=True, text=True)
    assert want.returncode == 0 and "process_example ok" in want.stdout, want.stdout + want.stderr

    def fields(out):
        return {k: v for k, v in (l.split(": ", 1) for l in out.splitlines() if ": " in l)}
    g, w = fields(got.stdout), fields(want.stdout)
    assert len(g["hyp"].split()) >= 1
    for k in ("frames", "hyp", "weight", "loglikelihood_per_frame"):
        assert g[k] == w[k], (k, g[k], w[k])
