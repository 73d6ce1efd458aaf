"""tests/cpp/online_features_example.cc: the WAV's fbank, 10 frames a step, as raw features through a features-only
pocketkaldi::OnlineScorer and pocketkaldi::OnlineDecoder, and through pocketkaldi::OnlineRecognizer::OpenFeatures /
PushFeatures (include/pocketkaldi_amd.hpp).  Its final lines equal tests/cpp/gpu_decode_example.cc's for the whole
utterance, and the recognizer's sentence is pk.Recognizer's on the wave."""
import os
import subprocess

import pytest

import pocketkaldi_amd as pk

from test_cpp_stream import G, build


def test_online_features_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("online_features_example"), "--link-only"], text=True)


@pytest.mark.gpu
@pytest.mark.parametrize("wav", ["en-us-hello.wav", "en-us-cat.wav"])
def test_online_features_example_equals_gpu_decode_example(wav):
    from refmodel_text import DIR
    args = [os.path.join(DIR, "refmodel.conf"), os.path.join(G, wav), os.path.join(DIR, "wordloop.fst")]
    conf = os.path.join(DIR, "recognizer.conf")
    got = subprocess.run([build("online_features_example")] + args + [conf], capture_output=True, text=True)
    assert got.returncode == 0 and "online_features_example ok" in got.stdout, got.stdout + got.stderr
    want = subprocess.run([build("gpu_decode_example")] + args, capture_output=True, text=True)
    assert want.returncode == 0 and "gpu_decode_example ok" in want.stdout, want.stdout + want.stderr
    assert got.stdout.count("partial ") >= 3

    def fields(out):
        return {k: v for k, v in (l.split(": ", 1) for l in out.splitlines() if ": " in l and not l.startswith("partial"))}
    g, w = fields(got.stdout), fields(want.stdout)
    for k in ("frames", "hyp", "weight", "loglikelihood_per_frame"):
        assert g[k] == w[k], (k, g[k], w[k])
    rec = pk.Recognizer(conf, max_utts=1, max_total_samples=200000)
    (whole,) = rec.process([pk.read_wav(os.path.join(G, wav))])
    rec.close()
    assert whole.text and g["recognizer_hyp"] == whole.text
    assert g["recognizer_loglikelihood_per_frame"] == "%.9g" % whole.loglikelihood_per_frame
