"""The oracle against the REAL reference code that builds in this image
(oracle/_ref = srfft.cc + gemm.cc + gemm_haswell.cc compiled from /root/reference)
and against the committed outputs of that build (tests/golden/ref_*.npz).
Bit-exact.  CPU only."""
import os

import numpy as np
import pytest

from oracle import oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_srfft512_matches_committed_reference_output():
    z = np.load(os.path.join(G, "ref_srfft512.npz"))
    f = O.Srfft(512)
    for fr, sp in zip(z["frames"], z["spectra"]):
        assert np.array_equal(_bits(f.forward(fr)), _bits(sp))


def test_sgemm_matches_committed_reference_output():
    z = np.load(os.path.join(G, "ref_sgemm.npz"))
    for i in range(4):
        A, B, Cref = z["A%d" % i], z["B%d" % i], z["C%d" % i]
        assert np.array_equal(_bits(O.sgemm(A, B)), _bits(Cref))
        assert np.array_equal(_bits(O.sgemm_naive(A, B)), _bits(Cref))


needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")


@needs_ref
@pytest.mark.parametrize("n", [4, 8, 16, 32, 64, 128, 512, 1024])
def test_srfft_bitwise_vs_live_reference(n):
    rng = np.random.default_rng(n)
    f = O.Srfft(n)
    for scale in (1.0, 3e4, 1e-3):
        x = (rng.standard_normal(n) * scale).astype(np.float32)
        assert np.array_equal(_bits(f.forward(x)), _bits(O.ref_srfft(x)))


@needs_ref
@pytest.mark.parametrize("shape", [(7, 16, 440), (37, 50, 1024), (13, 33, 2048),
                                   (300, 20, 513), (6, 16, 512), (5, 4100, 30), (1, 1, 1)])
def test_sgemm_bitwise_vs_live_reference(shape):
    m, n, k = shape
    rng = np.random.default_rng(m * 131 + k)
    A = rng.standard_normal((m, k)).astype(np.float32)
    B = rng.standard_normal((k, n)).astype(np.float32)
    r = O.ref_sgemm(A, B)
    assert np.array_equal(_bits(O.sgemm(A, B)), _bits(r))
    assert np.array_equal(_bits(O.sgemm_naive(A, B)), _bits(r))


# ------------------------------------------------------------------ the reference's whole acoustic path, committed
# tests/golden/ref_am_path.npz holds outputs of the REAL reference (oracle/_ref/libpkref_am*.so, made by
# tests/golden/make_ref_fixtures.py): a pin that holds in a checkout without the reference tree.  The live library
# against the same fixture shows a drifting compiler or flag as such, not as an oracle or kernel bug.

def _same_bits_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, a.view(np.uint32)), np.where(both, 0, b.view(np.uint32)))


def _check_against_fixture(wav_read, fbank, cmvn, refmodel_ll, model_ll, overflow_ll):
    """Every array / hash of the fixture recomputed by one implementation (the oracle, or the live reference)."""
    from pocketkaldi_amd import synth
    from refmodel_files import load_ref_am_path, overflow_model, sha256_rows
    z = load_ref_am_path()
    stats = O.read_vec(os.path.join(G, "cmvn_stats.bin"))
    rstats = O.read_vec(os.path.join(G, "refmodel", "refmodel_cmvn.bin"))
    waves = {"hello": wav_read(os.path.join(G, "en-us-hello.wav")), "cat": wav_read(os.path.join(G, "en-us-cat.wav")),
             "utt950": synth.utterance(950, seconds=7.3)}
    for name, w in waves.items():
        fb = fbank(w)
        assert _same_bits_nan(fb, z["fbank_" + name]), name
        assert _same_bits_nan(cmvn(stats, fb), z["cmvn_" + name]), name
        if name != "utt950":
            assert _same_bits_nan(refmodel_ll(cmvn(rstats, fb)), z["ll_refmodel_" + name]), name
    assert z["fbank_utt950"].shape == (728, 40)                      # the 600-frame window slides
    for name in ("S", "W"):
        layers, prior, L, R = synth.model(name)
        ll = model_ll(layers, prior, L, R, z["cmvn_hello"])
        assert np.array_equal(sha256_rows(ll), z["ll_%s_hello_sha256" % name]), name
        assert _same_bits_nan(ll[[0, 23, 46]], z["ll_%s_hello_rows" % name]), name
    layers, prior = overflow_model()
    assert int(np.isnan(z["ll_overflow"]).sum()) == 30
    assert _same_bits_nan(overflow_ll(layers, prior, np.zeros((5, 40), np.float32)), z["ll_overflow"])


def test_oracle_matches_committed_reference_acoustic_path():
    from refmodel_text import load_text_model
    layers, prior, L, R, _, _ = load_text_model()
    nn = O.Nnet(layers)
    _check_against_fixture(O.wav_read, O.Fbank().compute, O.cmvn,
                           lambda f: nn.am_compute(f, prior, L, R, 0.1),
                           lambda ls, pr, l, r, f: O.Nnet(ls).am_compute(f, pr, l, r, 0.1),
                           lambda ls, pr, f: O.Nnet(ls).am_compute(f, pr, 0, 0, 0.1))


@pytest.mark.skipif(not O.have_ref_am(), reason="oracle/_ref/libpkref_am.so not built")
def test_live_reference_matches_its_committed_outputs(tmp_path):
    from refmodel_files import write_model
    refmodel = O.RefAm(os.path.join(G, "refmodel", "refmodel.conf"))
    n = [0]

    def model_ll(layers, prior, L, R, feats, ndebug=False):
        n[0] += 1
        d = tmp_path / str(n[0])
        d.mkdir()
        return O.RefAm(write_model(d, layers, prior, L, R), ndebug=ndebug).decodable(feats, 0.1)

    _check_against_fixture(O.ref_wav_read, O.ref_fbank, O.ref_cmvn, lambda f: refmodel.decodable(f, 0.1), model_ll,
                           lambda ls, pr, f: model_ll(ls, pr, 0, 0, f, ndebug=True))   # (aborts with assertions on)
