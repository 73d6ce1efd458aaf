#!/usr/bin/env python3
"""Extract the reference's own known-answer DATA into fixtures under tests/golden/.

Run in the build container (needs /root/reference).  Only numbers are taken:
  * test/srfft_test.cc:11-271  -- the 128-point real-FFT input/output pair
  * test/nnet_test.cc:25-109   -- the four layer micro-tests (restated by hand below)
  * test/data/*.wav, *.txt, cmvn_stats.bin are copied verbatim (data files).
And outputs of the REAL reference code that builds here (oracle/_ref: srfft.cc,
gemm.cc, gemm_haswell.cc) on our own seeded inputs:
  * ref_srfft512.npz  -- 8 frames in, packed spectra out
  * ref_sgemm.npz     -- small A, B and the reference GEMM<float>::Gemm product
And outputs of the reference's whole acoustic path (oracle/_ref/libpkref_am*.so: pcm_reader.cc, fbank.cc, cmvn.cc,
nnet.cc, am.cc, decodable.cc compiled from their own files) -- `make_ref_fixtures.py am` writes this one alone:
  * ref_am_path.npz   -- fbank and CMVN (test/data/cmvn_stats.bin) of both golden WAVs and of synth.utterance(950, 7.3 s)
                         (728 frames: the CMVN window slides); pk_decodable_init for tests/golden/refmodel on both WAVs
                         (CMVN with refmodel_cmvn.bin); for the synthetic models "S" and "W" on the hello WAV's CMVN'd
                         features a SHA-256 of the 47 x N matrix and rows 0, 23, 46; the overflowing softmax's 5 x 200
                         matrix from the -DNDEBUG flavour (with assertions on that input aborts, vector.cc:336).
"""
import json
import os
import re
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)


def parse_float_array(text, name):
    m = re.search(r"float\s+%s\s*\[[^\]]*\]\s*=\s*\{([^}]*)\}" % name, text, re.S)
    return [float(tok.rstrip("f")) for tok in re.findall(r"[-+0-9.eE]+f?", m.group(1)) if tok.strip("f")]


def make_am_fixture():
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from oracle import oracle as O
    from pocketkaldi_amd import synth
    from refmodel_files import overflow_model, sha256_rows, write_model
    assert O.have_ref_am()
    z = {}
    stats = O.read_vec(os.path.join(HERE, "cmvn_stats.bin"))
    rstats = O.read_vec(os.path.join(HERE, "refmodel", "refmodel_cmvn.bin"))
    refmodel = O.RefAm(os.path.join(HERE, "refmodel", "refmodel.conf"))
    waves = {"hello": O.ref_wav_read(os.path.join(HERE, "en-us-hello.wav")),
             "cat": O.ref_wav_read(os.path.join(HERE, "en-us-cat.wav")),
             "utt950": synth.utterance(950, seconds=7.3)}
    for name, w in waves.items():
        z["fbank_" + name] = O.ref_fbank(w)
        z["cmvn_" + name] = O.ref_cmvn(stats, z["fbank_" + name])
        if name != "utt950":
            z["ll_refmodel_" + name] = refmodel.decodable(O.ref_cmvn(rstats, z["fbank_" + name]), 0.1)
    assert z["fbank_utt950"].shape == (728, 40)
    for name in ("S", "W"):
        layers, prior, L, R = synth.model(name)
        with tempfile.TemporaryDirectory() as d:
            ll = O.RefAm(write_model(d, layers, prior, L, R)).decodable(z["cmvn_hello"], 0.1)
        z["ll_%s_hello_sha256" % name] = sha256_rows(ll)
        z["ll_%s_hello_rows" % name] = ll[[0, 23, 46]]
    layers, prior = overflow_model()
    with tempfile.TemporaryDirectory() as d:
        conf = write_model(d, layers, prior, 0, 0)
        z["ll_overflow"] = O.RefAm(conf, ndebug=True).decodable(np.zeros((5, 40), np.float32), 0.1)
    # float arrays are stored as their four byte planes (uint8 [4, ...], little-endian): sign / exponent bytes compress
    # far better apart from the mantissa bytes, which keeps the file under the size of the largest fixture so far;
    # tests/refmodel_files.py: load_ref_am_path() puts them together again
    z = {k: (np.moveaxis(np.ascontiguousarray(v, "<f4").view(np.uint8).reshape(v.shape + (4,)), -1, 0).copy()
             if v.dtype == np.float32 else v) for k, v in z.items()}
    np.savez_compressed(os.path.join(HERE, "ref_am_path.npz"), **z)
    print("ref_am_path.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "ref_am_path.npz")))


def main():
    if sys.argv[1:] == ["am"]:
        return make_am_fixture()
    src = open(os.path.join(REF, "test/srfft_test.cc")).read()
    data = parse_float_array(src, "data")
    fft = parse_float_array(src, "fft_data")
    assert len(data) == 128 and len(fft) == 128
    known = {
        "srfft128": {"input": data, "output": fft, "tol_abs": 1e-6,
                     "source": "test/srfft_test.cc:11-284"},
        # test/nnet_test.cc:23-110 (numbers restated; W is [out][in] like the model file)
        "linear": {"W": [[0.1, 0.8, 0.9], [0.4, 0.2, 0.7], [0.2, 0.1, 0.1], [0.4, 0.3, 0.2]],
                   "b": [0.1, -0.1, 0.2, -0.2], "x": [0.3, -0.1, 0.9],
                   "y": [0.86, 0.63, 0.34, 0.07], "tol_abs": 1e-6,
                   "source": "test/nnet_test.cc:23-55"},
        "softmax": {"x": [0.3, -0.1, 0.9, 0.2],
                    "y": [0.2274135, 0.15243983, 0.41437442, 0.20577225], "tol_abs": 1e-6,
                    "source": "test/nnet_test.cc:57-73"},
        "relu": {"x": [0.3, -0.1, 0.9, 0.2], "y": [0.3, 0.0, 0.9, 0.2], "tol_abs": 1e-6,
                 "source": "test/nnet_test.cc:75-92"},
        "normalize": {"x": [0.3, -0.1, 0.9, 0.2], "sum_sq": 4.0, "tol_abs": 1e-4,
                      "source": "test/nnet_test.cc:94-110"},
        "wav_hello": {"num_samples": 7802, "first": [12, 38, -8], "num_frames": 47,
                      "source": "test/fbank_test.cc:15-56, test/data/en-us-hello.wav"},
    }
    with open(os.path.join(HERE, "ref_known_answers.json"), "w") as f:
        json.dump(known, f, indent=1)

    for name in ("en-us-hello.wav", "en-us-cat.wav", "cmvn_stats.bin",
                 "fbankmat_en-us-hello.wav.txt", "fbankcmvnmat_en-us-hello.wav.txt"):
        dst = os.path.join(HERE, name)
        if not os.path.exists(dst):
            shutil.copyfile(os.path.join(REF, "test/data", name), dst)

    from oracle import oracle as O
    assert O.have_ref()
    rng = np.random.default_rng(0xF17)
    frames = (rng.standard_normal((8, 512)) * np.array([1, 10, 100, 1e3, 1e4, 3e4, 1e-3, 0])[:, None]
              ).astype(np.float32)
    spectra = np.stack([O.ref_srfft(fr) for fr in frames])
    np.savez(os.path.join(HERE, "ref_srfft512.npz"), frames=frames, spectra=spectra)

    gem = {}
    for i, (m, n, k) in enumerate([(7, 16, 440), (19, 12, 1024), (6, 10, 2048), (13, 5, 513)]):
        A = rng.standard_normal((m, k)).astype(np.float32)
        B = (rng.standard_normal((k, n)) * 0.05).astype(np.float32)
        gem["A%d" % i] = A
        gem["B%d" % i] = B
        gem["C%d" % i] = O.ref_sgemm(A, B)
    np.savez(os.path.join(HERE, "ref_sgemm.npz"), **gem)
    make_am_fixture()
    print("fixtures written to", HERE)


if __name__ == "__main__":
    main()
