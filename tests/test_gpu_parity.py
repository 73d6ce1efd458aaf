"""GPU parity tests proper: the HIP path, called through the C ABI, against the CPU
oracle on the same seeded inputs, against the reference's own fixtures, and against
committed outputs of the real reference code (tests/golden/ref_*.npz).

Bars (stated per test):
  * fbank, CMVN, affine layers, ReLU, Normalize: bit-exact (the front-end's logf is the C
            library's algorithm restated, csrc/pk_logf.h).
  * log-likelihoods: |gpu - ref| <= 1e-4 * max(|ref|, 1)  (north_star: 1e-4 relative;
            "relative" is ill-conditioned near 0, hence the max(.,1)).
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth
from oracle import oracle as O


def fuzz_seeds(n):
    """Seeds of a fuzz test: 0..n-1 by default; a soak run on the GPU box widens and moves the range
    (PK_FUZZ_SEEDS=count, PK_FUZZ_BASE=first seed; tools/soak.sh)."""
    base = int(os.environ.get("PK_FUZZ_BASE", "0"))
    return range(base, base + int(os.environ.get("PK_FUZZ_SEEDS", n)))

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KNOWN = json.load(open(os.path.join(G, "ref_known_answers.json")))


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


def assert_fbank_close(gpu, ref):
    assert gpu.shape == ref.shape
    if ref.size == 0:
        return
    d = ulp_diff(gpu, ref)
    assert d.max() == 0, "max ULP %d, bit-identical fraction %.6f" % (d.max(), np.mean(d == 0))


def assert_loglik_close(gpu, ref):
    assert gpu.shape == ref.shape
    tol = 1e-4 * np.maximum(np.abs(ref), 1.0)
    err = np.abs(gpu.astype(np.float64) - ref.astype(np.float64))
    assert np.all(err <= tol), "max err %.3e (tol %.1e)" % (err.max(), tol.flat[err.argmax()])


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


# ------------------------------------------------------------------ front-end

def test_device_logf_is_the_c_librarys_logf():
    """fbank.cc:244-245 -> vector.cc:334-339 -> libm logf.  The kernel's restatement
    (csrc/pk_logf.h) against the oracle's libm calls: 4 M random positive normal bit patterns,
    a dense run around 1.0, the floor value, the range of mel energies, +inf."""
    rng = np.random.default_rng(11)
    bits = rng.integers(0x00800000, 0x7F800000, size=1 << 22, dtype=np.uint32)
    x = np.concatenate([
        bits.view(np.float32),
        (np.uint32(0x3F800000) + np.arange(-200000, 200000).astype(np.int64)).astype(np.uint32).view(np.float32),
        np.array([1.1920928955078125e-07, 1.0, 2.0, 0.5, 3.4028234663852886e38, np.inf], dtype=np.float32),
        np.exp(rng.uniform(-16, 30, size=1 << 20)).astype(np.float32),
    ])
    assert bits_equal(pk.device_logf(x), O.logf(x))
    assert np.isnan(pk.device_logf(np.array([np.nan], dtype=np.float32))[0])


def test_fbank_hello_wav_vs_oracle_and_kaldi_dump():
    w = O.wav_read(os.path.join(G, "en-us-hello.wav"))
    gpu = pk.Fbank().compute(w)
    assert_fbank_close(gpu, O.Fbank().compute(w))
    dump = np.loadtxt(os.path.join(G, "fbankmat_en-us-hello.wav.txt"))
    assert np.max(np.abs(gpu.reshape(-1) - dump)) < 3e-5      # see test_oracle_fixtures.py


def test_fbank_second_wav():
    w = O.wav_read(os.path.join(G, "en-us-cat.wav"))
    assert_fbank_close(pk.Fbank().compute(w), O.Fbank().compute(w))


@pytest.mark.parametrize("n", [0, 399, 400, 401, 559, 560, 16000])
def test_fbank_lengths(n):
    w = synth.utterance(3, seconds=1.0)[:n]
    gpu = pk.Fbank().compute(w)
    if O.num_frames(n) == 0:          # fbank.cc:272-273: resized to 0 x 0
        assert gpu.size == 0
        return
    assert gpu.shape == (O.num_frames(n), 40)
    assert_fbank_close(gpu, O.Fbank().compute(w))


def test_fbank_silence_hits_floor():
    w = synth.utterance(5, seconds=1.0)
    w[4000:9000] = 0.0                                       # all-zero stretch -> FLT_EPSILON floor
    gpu, ref = pk.Fbank().compute(w), O.Fbank().compute(w)
    assert np.isclose(ref.min(), np.log(np.float32(1.1920929e-07)), atol=1e-5)
    assert_fbank_close(gpu, ref)


def test_fbank_non_integer_samples_take_ordered_sum_path():
    rng = np.random.default_rng(11)
    w = (rng.standard_normal(8000) * 777.7).astype(np.float32)   # not integer valued
    assert_fbank_close(pk.Fbank().compute(w), O.Fbank().compute(w))
    w32 = (rng.integers(-2**31, 2**31 - 1, 4000)).astype(np.float32)   # 32-bit PCM range
    assert_fbank_close(pk.Fbank().compute(w32), O.Fbank().compute(w32))


@pytest.mark.parametrize("T", [1, 47, 200, 650, 998])
def test_cmvn_bit_exact(T):
    rng = np.random.default_rng(T)
    raw = (rng.standard_normal((T, 40)) * 3 + 12).astype(np.float32)
    g = synth.global_cmvn_stats()
    gpu = pk.CMVN(g, raw).get_frames()
    assert bits_equal(gpu, O.cmvn(g, raw))


def test_cmvn_reference_fixture():
    w = O.wav_read(os.path.join(G, "en-us-hello.wav"))
    stats = O.read_vec(os.path.join(G, "cmvn_stats.bin"))
    raw = O.Fbank().compute(w)
    gpu = pk.CMVN(stats, raw).get_frames()
    assert bits_equal(gpu, O.cmvn(stats, raw))
    dump = np.loadtxt(os.path.join(G, "fbankcmvnmat_en-us-hello.wav.txt"))
    assert np.max(np.abs(gpu.reshape(-1) - dump)) < 3e-5


# ------------------------------------------------------------------ layers

def test_layer_known_answers_from_nnet_test():
    k = KNOWN["linear"]
    am = pk.AcousticModel([("linear", np.array(k["W"]), np.array(k["b"]))], num_pdfs=4)
    y = am.propagate(np.array([k["x"]], dtype=np.float32))
    assert np.max(np.abs(y[0] - np.array(k["y"]))) < k["tol_abs"]
    for name in ("softmax", "relu"):
        k = KNOWN[name]
        y = pk.AcousticModel([(name,)], num_pdfs=4).propagate(np.array([k["x"]], dtype=np.float32))
        assert np.max(np.abs(y[0] - np.array(k["y"]))) < k["tol_abs"]
    k = KNOWN["normalize"]
    y = pk.AcousticModel([("normalize",)], num_pdfs=4).propagate(np.array([k["x"]], dtype=np.float32))
    assert abs(float(np.sum(y.astype(np.float64) ** 2)) - k["sum_sq"]) < k["tol_abs"]


def test_affine_bit_exact_vs_committed_reference_gemm():
    z = np.load(os.path.join(G, "ref_sgemm.npz"))
    for i in range(4):
        A, B, Cref = z["A%d" % i], z["B%d" % i], z["C%d" % i]   # C = A * B, B is [K][N]
        am = pk.AcousticModel([("linear", B.T.copy(), np.zeros(B.shape[1], np.float32))],
                              num_pdfs=B.shape[1])
        assert bits_equal(am.propagate(A), Cref)


@pytest.mark.parametrize("shape", [(1, 3, 4), (7, 440, 1024), (129, 1024, 1024), (300, 2048, 130),
                                   (5, 513, 3000), (257, 17, 9),
                                   # K = 2, 3, 4 chunks of 512 on a small launch: one k-group of waves
                                   # per chunk, added in chunk order (gemm.cc:95-123)
                                   (998, 1024, 1024), (200, 1536, 256), (64, 2048, 2048), (70, 2560, 64)])
def test_affine_relu_bit_exact_vs_oracle(shape):
    T, K, N = shape
    rng = np.random.default_rng(T * 7 + K)
    W = (rng.standard_normal((N, K)) * np.sqrt(2.0 / K)).astype(np.float32)
    b = (rng.standard_normal(N) * 0.1).astype(np.float32)
    x = rng.standard_normal((T, K)).astype(np.float32)
    layers = [("linear", W, b), ("relu",)]
    assert bits_equal(pk.AcousticModel(layers, num_pdfs=N).propagate(x), O.Nnet(layers).propagate(x))


def test_hidden_stack_bit_exact_and_normalize():
    rng = np.random.default_rng(5)
    dims = [60, 200, 136, 72]
    layers = []
    for i in range(3):
        W = (rng.standard_normal((dims[i + 1], dims[i])) * np.sqrt(2.0 / dims[i])).astype(np.float32)
        layers += [("linear", W, (rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32)),
                   ("relu",), ("normalize",)]
    x = rng.standard_normal((77, 60)).astype(np.float32)
    assert bits_equal(pk.AcousticModel(layers, num_pdfs=72).propagate(x), O.Nnet(layers).propagate(x))


def test_softmax_probabilities():
    rng = np.random.default_rng(9)
    W = (rng.standard_normal((3000, 64)) * 0.2).astype(np.float32)
    layers = [("linear", W, np.zeros(3000, np.float32)), ("softmax",)]
    x = rng.standard_normal((33, 64)).astype(np.float32)
    gpu, ref = pk.AcousticModel(layers, num_pdfs=3000).propagate(x), O.Nnet(layers).propagate(x)
    assert np.allclose(gpu.sum(axis=1), 1.0, atol=1e-5)
    assert np.max(np.abs(gpu - ref) / np.maximum(ref, 1e-30)) < 1e-5


# ------------------------------------------------------------------ the boundary

def tiny_model():
    layers, prior, L, R = synth.model("tiny")
    tid2pdf = np.concatenate([[0], np.arange(50), np.arange(50)[::-1]]).astype(np.int32)
    return layers, prior, L, R, tid2pdf


@pytest.mark.parametrize("T", [1, 3, 47, 300])
def test_decodable_tiny_net_vs_oracle(T):
    layers, prior, L, R, tid2pdf = tiny_model()
    rng = np.random.default_rng(T)
    feats = rng.standard_normal((T, 40)).astype(np.float32)
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    d = pk.Decodable(am, 0.1, feats)
    ref = O.Nnet(layers).am_compute(feats, prior, L, R, 0.1)
    lp = d.log_prob()
    assert_loglik_close(lp, ref)
    # decodable.cc:24-36 semantics
    assert d.is_last_frame(-1) is False or T == 0
    assert d.is_last_frame(T - 1) is True
    assert d.is_last_frame(0) is (T == 1)
    for frame, tid in [(0, 1), (T - 1, 50), (T // 2, 77)]:
        assert d.loglikelihood(frame, tid) == lp[frame, tid2pdf[tid]]
    d.destroy()


def test_decodable_without_softmax_layer_uses_plain_tail():
    rng = np.random.default_rng(2)
    W = np.abs(rng.standard_normal((20, 40 * 3))).astype(np.float32) * 0.05
    layers = [("linear", W, np.full(20, 0.01, np.float32)), ("relu",)]
    prior = np.full(20, 0.05, np.float32)
    feats = np.abs(rng.standard_normal((19, 40))).astype(np.float32)
    feats[3] = 0.0                                            # relu output 0.01 ... and floor cases
    am = pk.AcousticModel(layers, prior, 1, 1)
    lp = pk.Decodable(am, 1.0, feats).log_prob()
    assert_loglik_close(lp, O.Nnet(layers).am_compute(feats, prior, 1, 1, 1.0))


def test_full_path_single_utterance_S_model():
    layers, prior, L, R = synth.model("S")
    wave = synth.utterance(0, seconds=3.0)
    g = synth.global_cmvn_stats()
    am = pk.AcousticModel(layers, prior, L, R)
    bs = pk.BatchScorer(am, g, 1, wave.shape[0])
    bs.set_waves([wave])
    bs.score(0.1)
    fb_ref = O.Fbank().compute(wave)
    assert_fbank_close(bs.fetch_fbank(0), fb_ref)
    # stage-wise: CMVN of the GPU's own fbank must be bit-exact
    assert bits_equal(bs.fetch_cmvn(0), O.cmvn(g, bs.fetch_fbank(0)))
    ref = O.Nnet(layers).am_compute(O.cmvn(g, fb_ref), prior, L, R, 0.1)
    d = bs.fetch(0)
    assert_loglik_close(d.log_prob(), ref)
    assert d.is_last_frame(bs.num_frames(0) - 1)
    # and the reference-shaped entry point on the same CMVN'd features agrees with the batch path
    d2 = pk.Decodable(am, 0.1, bs.fetch_cmvn(0))
    assert bits_equal(d2.log_prob(), d.log_prob())


def test_batch_ragged_utterances_match_per_utterance_oracle():
    layers, prior, L, R, tid2pdf = tiny_model()
    g = synth.global_cmvn_stats()
    lens = [16000, 399, 5000, 400, 12345, 0, 104000, 7802]     # incl. too-short (0 frames) and >600 frames
    waves = [synth.utterance(10 + i, seconds=7.0)[:n] for i, n in enumerate(lens)]
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    bs = pk.BatchScorer(am, g, len(waves), sum(lens))
    bs.set_waves(waves)
    bs.score(0.1)
    assert bs.total_frames() == sum(O.num_frames(n) for n in lens)
    nn = O.Nnet(layers)
    for u, w in enumerate(waves):
        T = O.num_frames(len(w))
        assert bs.num_frames(u) == T
        d = bs.fetch(u)
        if T == 0:
            assert d.log_prob().shape[0] == 0
            continue
        fb = O.Fbank().compute(w)
        assert_fbank_close(bs.fetch_fbank(u), fb)
        assert_loglik_close(d.log_prob(), nn.am_compute(O.cmvn(g, fb), prior, L, R, 0.1))
    # int16 ingestion gives the same bits as float ingestion
    bs.set_waves_i16([w.astype(np.int16) for w in waves])
    bs.score(0.1)
    bs2 = pk.BatchScorer(am, g, len(waves), sum(lens))
    bs2.set_waves(waves)
    bs2.score(0.1)
    for u in range(len(waves)):
        assert bits_equal(bs.fetch(u).log_prob(), bs2.fetch(u).log_prob())


def test_chunking_is_invisible(monkeypatch):
    layers, prior, L, R, _ = tiny_model()
    g = synth.global_cmvn_stats()
    waves = [synth.utterance(40 + i, seconds=2.5) for i in range(6)]
    am = pk.AcousticModel(layers, prior, L, R)
    outs = []
    for chunk, lanes in (("128", "1"), ("8192", "1"), ("256", "2")):   # lanes = 2: odd chunks on a second stream
        monkeypatch.setenv("PK_MI355_CHUNK", chunk)
        monkeypatch.setenv("PK_MI355_LANES", lanes)
        bs = pk.BatchScorer(am, g, len(waves), sum(len(w) for w in waves))
        bs.set_waves(waves)
        for _ in range(2):                      # twice: the second pass must wait for both lanes of the first
            bs.score(0.1, sync=False)
        bs.synchronize()
        outs.append([bs.fetch(u).log_prob() for u in range(len(waves))])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert bits_equal(a, b)


def test_model_files_roundtrip(tmp_path):
    """NNT0/LAY0/MAT0/VEC0 reader (nnet.cc:80-147) against files written per convert_am.py:71-118."""
    from refmodel_files import write_model, write_vec
    layers, prior, L, R, tid2pdf = tiny_model()
    write_model(tmp_path, layers, prior, L, R, tid2pdf)
    nnet = tmp_path / "am.nnet"
    am_file = pk.AcousticModel.read(str(nnet), str(tmp_path / "am.prior"), str(tmp_path / "tid2pdf.bin"),
                                    L, R, 50)
    am_mem = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    feats = np.random.default_rng(0).standard_normal((21, 40)).astype(np.float32)
    assert bits_equal(pk.Decodable(am_file, 0.1, feats).log_prob(), pk.Decodable(am_mem, 0.1, feats).log_prob())
    assert am_file.transition_id_to_pdf_id(3) == tid2pdf[3]
    # the oracle's reader parses the same file the same way
    assert bits_equal(O.Nnet.read(str(nnet)).propagate(O.splice(feats, L, R)),
                      O.Nnet(layers).propagate(O.splice(feats, L, R)))
    with pytest.raises(pk.PkError):
        pk.AcousticModel.read(str(tmp_path / "am.prior"), str(tmp_path / "am.prior"), None, L, R, 50)
    # the same files through the reference's model config (pk_load, pocketkaldi.cc:72-144):
    # relative paths, mixed-case keys, comments, decoder keys ignored
    g = synth.global_cmvn_stats()
    with open(tmp_path / "cmvn.bin", "wb") as f:
        write_vec(f, g)
    (tmp_path / "pocketkaldi.conf").write_text(
        "# model\nfst = HCLG.pfst\nsymbol_table = words.bin\ncmvn_stats = cmvn.bin\n"
        "NNET = am.nnet\nprior=am.prior\n  tid2pdf = %s \nleft_context = %d\nright_context = %d\nnum_pdfs = 50\n"
        % (tmp_path / "tid2pdf.bin", L, R))
    am_conf, stats = pk.AcousticModel.load(str(tmp_path / "pocketkaldi.conf"))
    assert bits_equal(stats, g)
    assert bits_equal(pk.Decodable(am_conf, 0.1, feats).log_prob(), pk.Decodable(am_mem, 0.1, feats).log_prob())
    assert am_conf.transition_id_to_pdf_id(3) == tid2pdf[3] and am_conf.num_pdfs() == 50


# ------------------------------------------------------------------ f16x3 precision mode
# Split-fp16 arithmetic on the fp16 matrix cores (include/pk_mi355.h, PK_MI355_PRECISION_F16X3):
# not bit-exact by construction; the bar is the north_star tolerance, and the measured error
# is asserted an order of magnitude inside it.

@pytest.mark.parametrize("shape", [(1, 3, 4), (7, 440, 1024), (300, 1024, 1024), (257, 2048, 130),
                                   (5, 513, 3000)])
def test_f16x3_affine_close_to_fp32_chain(shape):
    T, K, N = shape
    rng = np.random.default_rng(T * 7 + K)
    W = (rng.standard_normal((N, K)) * np.sqrt(2.0 / K)).astype(np.float32)
    b = (rng.standard_normal(N) * 0.1).astype(np.float32)
    x = rng.standard_normal((T, K)).astype(np.float32)
    layers = [("linear", W, b), ("relu",)]
    gpu = pk.AcousticModel(layers, num_pdfs=N, precision="f16x3").propagate(x)
    ref = O.Nnet(layers).propagate(x)
    # error budget relative to the magnitude of the dot products: 2^-21 of sum |x||w|
    scale = (np.abs(x) @ np.abs(W.T)) + np.abs(b)
    assert np.max(np.abs(gpu - ref) / scale) < 2.0 ** -20


def test_f16x3_full_path_S_model_within_contract():
    layers, prior, L, R = synth.model("S")
    wave = synth.utterance(0, seconds=3.0)
    g = synth.global_cmvn_stats()
    am = pk.AcousticModel(layers, prior, L, R, precision="f16x3")
    bs = pk.BatchScorer(am, g, 1, wave.shape[0])
    bs.set_waves([wave])
    bs.score(0.1)
    ref = O.Nnet(layers).am_compute(O.cmvn(g, O.Fbank().compute(wave)), prior, L, R, 0.1)
    got = bs.fetch(0).log_prob()
    assert_loglik_close(got, ref)                              # the 1e-4 contract
    assert np.max(np.abs(got - ref)) < 2e-5                    # measured: ~1e-6
    # the reference-shaped entry point runs the same arithmetic
    d2 = pk.Decodable(am, 0.1, bs.fetch_cmvn(0))
    assert bits_equal(d2.log_prob(), got)


def test_f16x3_ragged_batch_and_chunking(monkeypatch):
    layers, prior, L, R, tid2pdf = tiny_model()
    g = synth.global_cmvn_stats()
    lens = [16000, 399, 5000, 400, 104000, 0, 7802]
    waves = [synth.utterance(60 + i, seconds=7.0)[:n] for i, n in enumerate(lens)]
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf, precision="f16x3")
    nn = O.Nnet(layers)
    outs = []
    for chunk in ("256", "65536"):
        monkeypatch.setenv("PK_MI355_CHUNK", chunk)
        bs = pk.BatchScorer(am, g, len(waves), sum(lens))
        bs.set_waves(waves)
        bs.score(0.1)
        outs.append([bs.fetch(u).log_prob() for u in range(len(waves))])
    for u, w in enumerate(waves):
        assert bits_equal(outs[0][u], outs[1][u])
        if O.num_frames(len(w)) == 0:
            assert outs[0][u].shape[0] == 0
            continue
        ref = nn.am_compute(O.cmvn(g, O.Fbank().compute(w)), prior, L, R, 0.1)
        assert_loglik_close(outs[0][u], ref)


def test_f16x3_rejects_unsupported_layer_patterns():
    eye = ("linear", np.eye(8, dtype=np.float32), np.zeros(8, np.float32))
    with pytest.raises(pk.PkError):                 # a Normalize must sit between two affine layers
        pk.AcousticModel([eye, ("normalize",)], num_pdfs=8, precision="f16x3")
    with pytest.raises(pk.PkError):
        pk.AcousticModel([eye, ("normalize",), ("normalize",), eye], num_pdfs=8, precision="f16x3")
    with pytest.raises(pk.PkError):
        pk.AcousticModel([("softmax",)], num_pdfs=8, precision="f16x3")
    pk.AcousticModel([eye, ("relu",), ("normalize",), eye, ("softmax",)], num_pdfs=8, precision="f16x3")    # accepted


def test_f16x3_normalize_layers_batch_path_within_contract():
    """The relu + renormalize stack through the BATCH scorer in f16x3 (NormalizeSplitKernel between the GEMMs):
    ragged utterances, every one inside the contract against the oracle, and measured an order below."""
    rng = np.random.default_rng(41)
    layers, prior = _random_net(rng, [440, 384, 520, 300, 700], normalize_p=1.0)
    assert [l[0] for l in layers].count("normalize") == 3
    g = synth.global_cmvn_stats()
    waves = [synth.utterance(300 + u, s) for u, s in enumerate([1.3, 0.05, 4.0, 2.2])]
    am = pk.AcousticModel(layers, prior, 5, 5, precision="f16x3")
    bs = pk.BatchScorer(am, g, len(waves), sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    nn = O.Nnet(layers)
    for u, w in enumerate(waves):
        ref = nn.am_compute(O.cmvn(g, O.Fbank().compute(w)), prior, 5, 5, 0.1)
        got = bs.fetch(u).log_prob()
        assert_loglik_close(got, ref)
        assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)) < 2e-5


def test_device_side_loglikelihood_gather():
    """decodable.cc:24-31 for many (frame, trans_id) pairs without leaving HBM."""
    import ctypes
    L_ = pk.lib()

    def to_device(arr):
        p = L_.pk_mi355_device_malloc(arr.nbytes)
        assert p
        assert L_.pk_mi355_memcpy(p, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes, 1) == 0   # H2D
        return p

    layers, prior, L, R, tid2pdf = tiny_model()
    g = synth.global_cmvn_stats()
    waves = [synth.utterance(80, 2.0), synth.utterance(81, 1.0)]
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    bs = pk.BatchScorer(am, g, 2, sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    for u in range(2):
        d = bs.fetch(u)
        T = bs.num_frames(u)
        rng = np.random.default_rng(u)
        frames = rng.integers(0, T, 1000).astype(np.int32)
        tids = rng.integers(1, len(tid2pdf), 1000).astype(np.int32)
        out = np.zeros(1000, dtype=np.float32)
        df, dt, do = to_device(frames), to_device(tids), to_device(out)
        bs.gather_loglik(u, df, dt, 1000, do)
        bs.synchronize()
        assert L_.pk_mi355_memcpy(out.ctypes.data_as(ctypes.c_void_p), do, out.nbytes, 2) == 0   # D2H
        want = np.array([d.loglikelihood(int(f), int(t)) for f, t in zip(frames, tids)], dtype=np.float32)
        assert bits_equal(out, want)
        for p in (df, dt, do):
            L_.pk_mi355_device_free(p)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("chunk", ["256", "262144"])
def test_compact_rows_equal_the_padded_layout(chunk, precision, monkeypatch):
    """Round 5: in f32 the layer stack's rows are compact (utterance after utterance, each padded to four rows, no rows for
    the L + R context pads that separate utterances in Yt; the first layer's spliced operand carries a per-lane column
    shift).  PK_MI355_COMPACT_ROWS=0 is the earlier layout (row = column of Yt).  Both must give every utterance the same
    bits -- lengths of 0, 1, 3, 4, 5 and 130 frames among them (runs that end inside, at and across groups of four rows
    and tiles), with one and with several layer-stack chunks -- through fetch, fetch_all and the device-side view."""
    monkeypatch.setenv("PK_MI355_CHUNK", chunk)
    layers, prior, L, R, tid2pdf = tiny_model()
    g = synth.global_cmvn_stats()
    frames = [7, 0, 1, 3, 4, 5, 130, 64, 2, 611, 33]
    waves = [synth.utterance(300 + i, 8.0)[:(400 + 160 * (t - 1)) if t > 0 else 123] for i, t in enumerate(frames)]
    got = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PK_MI355_COMPACT_ROWS", mode)
        am = pk.AcousticModel(layers, prior, L, R, tid2pdf, precision=precision)
        bs = pk.BatchScorer(am, g, len(waves), sum(len(w) for w in waves))
        bs.set_waves(waves)
        bs.score(0.1)
        assert [bs.num_frames(u) for u in range(len(waves))] == frames
        views = bs.fetch_all()
        one = []
        for u, v in enumerate(views):
            d = bs.fetch(u)
            assert bits_equal(d.log_prob(), v.log_prob())
            one.append(d.log_prob().copy())
        got[mode] = one
        # rows of d_ll: compact = sum of the lengths rounded up to four; padded = sum of (T + L + R)
        span = (bs.loglik_device(len(waves) - 1) - bs.loglik_device(0)) // (4 * am.num_pdfs())
        want = sum((t + 3) // 4 * 4 for t in frames[:-1]) if mode == "1" else sum(t + L + R for t in frames[:-1] if t > 0)
        assert span == want
        bs.close()
    nn, fb = O.Nnet(layers), O.Fbank()
    for u, (a, b) in enumerate(zip(got["0"], got["1"])):
        assert bits_equal(a, b), "utterance %d (%d frames)" % (u, frames[u])
        if frames[u] > 0:
            assert_loglik_close(b, nn.am_compute(O.cmvn(g, fb.compute(waves[u])), prior, L, R, 0.1))


def test_process_acoustic_matches_staged_path(capfd):
    """stages 1-3 of pk_process (pocketkaldi.cc:186-218) fused, with the
    reference's per-stage stderr lines."""
    layers, prior, L, R, tid2pdf = tiny_model()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    stats = O.read_vec(os.path.join(G, "cmvn_stats.bin"))
    wave = pk.read_wav(os.path.join(G, "en-us-hello.wav"))
    d = pk.process_acoustic(am, stats, wave, 0.1, verbose=True)
    err = capfd.readouterr().err
    assert "Fbank: " in err and "CMVN: " in err and "NNET: " in err
    ref = O.Nnet(layers).am_compute(O.cmvn(stats, O.Fbank().compute(wave)), prior, L, R, 0.1)
    assert_loglik_close(d.log_prob(), ref)
    assert d.is_last_frame(46) and not d.is_last_frame(-1)
    # staged path through the class mirror gives the same bits
    staged = pk.Decodable(am, 0.1, pk.CMVN(stats, pk.Fbank().compute(wave)).get_frames())
    assert bits_equal(staged.log_prob(), d.log_prob())
    # empty utterance (pocketkaldi.cc:180-184) and a longer second call (workspace regrowth)
    assert pk.process_acoustic(am, stats, np.zeros(0, np.float32)).log_prob().shape[0] == 0
    w2 = synth.utterance(7, 4.0)
    d2 = pk.process_acoustic(am, stats, w2)
    ref2 = O.Nnet(layers).am_compute(O.cmvn(stats, O.Fbank().compute(w2)), prior, L, R, 0.1)
    assert_loglik_close(d2.log_prob(), ref2)


# ------------------------------------------------------------------ BASELINE shapes at full size

def test_wide_model_both_precisions_vs_oracle():
    """BASELINE configs[4] shape: 440 -> 6 x 2048 ReLU -> 8000 softmax (K = 2048: four 512-chunks)."""
    layers, prior, L, R = synth.model("W")
    feats = np.random.default_rng(3).standard_normal((70, 40)).astype(np.float32)
    ref = O.Nnet(layers).am_compute(feats, prior, L, R, 0.1)
    for prec in ("f32", "f16x3"):
        lp = pk.Decodable(pk.AcousticModel(layers, prior, L, R, precision=prec), 0.1, feats).log_prob()
        assert_loglik_close(lp, ref)
        assert np.max(np.abs(lp - ref)) < 2e-5


def test_full_size_batch_properties():
    """BASELINE configs[2]: 256 utterances x 10 s, model S.  (i) every frame's likelihoods re-normalise
    (logsumexp(ll / scale + log prior) == 0), (ii) an utterance scored inside the batch has the
    same bits as the same utterance scored alone, (iii) ALL 256 utterances against the oracle under the
    contract: the oracle runs ~8.6 k frames/s a core and its C calls release the interpreter lock, so a pool of
    16 threads (a fixed number, not the machine's core count) does the 255 488 frames in seconds."""
    layers, prior, L, R = synth.model("S")
    g = synth.global_cmvn_stats()
    B = 256
    waves = [synth.utterance(u, 10.0) for u in range(B)]
    am = pk.AcousticModel(layers, prior, L, R)
    bs = pk.BatchScorer(am, g, B, sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    assert bs.total_frames() == B * 998
    logp = np.log(prior.astype(np.float64))
    solo = pk.BatchScorer(am, g, 1, 160000)
    for u in (0, 1, 127, 255):
        ll = bs.fetch(u).log_prob()
        assert ll.shape == (998, 3000)
        z = ll.astype(np.float64) / np.float64(np.float32(0.1)) + logp
        lse = np.log(np.sum(np.exp(z - z.max(axis=1, keepdims=True)), axis=1)) + z.max(axis=1)
        assert np.max(np.abs(lse)) < 2e-4                       # (i)
        solo.set_waves([waves[u]])
        solo.score(0.1)
        assert bits_equal(solo.fetch(0).log_prob(), ll)         # (ii)
    from concurrent.futures import ThreadPoolExecutor
    nn = O.Nnet(layers)

    def check(u):                                               # (iii)
        ref = nn.am_compute(O.cmvn(g, O.Fbank().compute(waves[u])), prior, L, R, 0.1)
        assert_loglik_close(bs.fetch(u).log_prob(), ref)
        return u

    with ThreadPoolExecutor(max_workers=16) as pool:
        assert sorted(pool.map(check, range(B))) == list(range(B))


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_full_size_batch_properties_wide_model(prec):
    """BASELINE configs[4] at the size the bench times: 256 utterances x 10 s through the wide model
    (440 -> 6 x 2048 -> 8000): the 256 x 256-tile fp16 kernel at K = 2048 / N = 8000, the 8000-wide tail,
    131 072-row chunks.  Same size-independent properties as configs[2] above -- (i) total frames,
    (ii) every frame's likelihoods re-normalise, (iii) an utterance inside the batch has the bits of the
    same utterance scored alone -- and (iv) one utterance against the oracle at the path's 1e-4 (sampled, unlike
    the "S" twin above, which checks all 256: at 38 M multiply-adds a frame the oracle needs ~3 core-minutes for the
    255 488 frames and the fetches move 8 GB, for each of the two precisions, and what a full check adds -- every
    position of an utterance in the batch -- is what the "S" test already covers with the same layout code)."""
    layers, prior, L, R = synth.model("W")
    g = synth.global_cmvn_stats()
    B = 256
    waves = [synth.utterance(u, 10.0) for u in range(B)]
    am = pk.AcousticModel(layers, prior, L, R, precision=prec)
    bs = pk.BatchScorer(am, g, B, sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    assert bs.total_frames() == B * 998                         # (i)
    logp = np.log(prior.astype(np.float64))
    solo = pk.BatchScorer(am, g, 1, 160000)
    for u in (0, 127, 255):
        ll = bs.fetch(u).log_prob()
        assert ll.shape == (998, 8000) and np.all(np.isfinite(ll))
        z = ll.astype(np.float64) / np.float64(np.float32(0.1)) + logp
        lse = np.log(np.sum(np.exp(z - z.max(axis=1, keepdims=True)), axis=1)) + z.max(axis=1)
        assert np.max(np.abs(lse)) < 2e-4                       # (ii)
        solo.set_waves([waves[u]])
        solo.score(0.1)
        assert bits_equal(solo.fetch(0).log_prob(), ll)         # (iii)
    ref = O.Nnet(layers).am_compute(O.cmvn(g, O.Fbank().compute(waves[127])), prior, L, R, 0.1)
    assert_loglik_close(bs.fetch(127).log_prob(), ref)          # (iv)
    solo.close()
    bs.close()


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_run_to_run_determinism_under_load(prec):
    """Race screen for the DMA-ring / barrier structure of the GEMM kernels: the same batch scored
    40 times back to back (no host sync in between) must give identical bits every time, and
    those bits must be the ones a freshly built scorer produces."""
    import zlib
    layers, prior, L, R = synth.model("S")
    g = synth.global_cmvn_stats()
    waves = [synth.utterance(200 + u, 10.0) for u in range(24)]
    am = pk.AcousticModel(layers, prior, L, R, precision=prec)
    bs = pk.BatchScorer(am, g, len(waves), sum(len(w) for w in waves))
    bs.set_waves(waves)
    sums = set()
    for rep in range(8):
        for _ in range(5):
            bs.score(0.1, sync=False)
        bs.synchronize()
        sums.add(tuple(zlib.crc32(bs.fetch(u).log_prob().tobytes()) for u in (0, 11, 23)))
    assert len(sums) == 1
    bs2 = pk.BatchScorer(am, g, len(waves), sum(len(w) for w in waves))
    bs2.set_waves(waves)
    bs2.score(0.1)
    assert tuple(zlib.crc32(bs2.fetch(u).log_prob().tobytes()) for u in (0, 11, 23)) in sums


def test_long_single_utterance_through_the_reference_entry_point():
    """pk_decodable_init on an utterance longer than the single-utterance pass (4096 frames) and
    longer than the CMVN window several times over: the internal row blocks are invisible."""
    layers, prior, L, R, tid2pdf = tiny_model()
    rng = np.random.default_rng(17)
    feats = rng.standard_normal((9001, 40)).astype(np.float32)
    ref = O.Nnet(layers).am_compute(feats, prior, L, R, 0.1)
    for prec in ("f32", "f16x3"):
        am = pk.AcousticModel(layers, prior, L, R, tid2pdf, precision=prec)
        d = pk.Decodable(am, 0.1, feats)
        assert_loglik_close(d.log_prob(), ref)
        assert d.is_last_frame(9000) and not d.is_last_frame(8999)
    # and the front-end on 95 s of audio (9498 frames, window slides for 8898 of them)
    w = synth.utterance(300, 95.0)
    g = synth.global_cmvn_stats()
    fb = pk.Fbank().compute(w)
    assert fb.shape == (9498, 40)
    assert_fbank_close(fb, O.Fbank().compute(w))
    assert bits_equal(pk.CMVN(g, fb).get_frames(), O.cmvn(g, fb))


def test_fetch_all_views_match_per_utterance_fetch():
    """pk_mi355_batch_fetch_all: one transfer into the page-locked arena; every view equals the
    malloc'd decodable pk_mi355_batch_fetch returns, destroy on a view frees nothing, and the
    arena is refilled by the next score."""
    layers, prior, L, R = synth.model("tiny")
    am = pk.AcousticModel(layers, prior, L, R)
    durs = [0.5, 0.02, 1.3, 0.031, 0.9]          # two utterances shorter than a frame -> T = 0
    waves = [synth.utterance(40 + u, d) for u, d in enumerate(durs)]
    bs = pk.BatchScorer(am, synth.global_cmvn_stats(), len(waves), sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1, sync=True)
    views = bs.fetch_all(sync=False)
    bs.synchronize()
    tid2pdf_n = am.num_pdfs()
    for u, v in enumerate(views):
        d = bs.fetch(u)
        a, b = v.log_prob(), d.log_prob()
        assert a.shape == b.shape == (bs.num_frames(u), tid2pdf_n if bs.num_frames(u) else 0)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        if bs.num_frames(u):
            assert v.is_last_frame(bs.num_frames(u) - 1) and not v.is_last_frame(-1)
        d.destroy()
        v.destroy()                                  # a view: nothing is freed
    # second round with other audio: the same arena now holds the new results
    waves2 = [synth.utterance(90 + u, 0.7) for u in range(3)]
    bs.set_waves(waves2)
    bs.score(0.1, sync=True)
    views2 = bs.fetch_all()
    for u, v in enumerate(views2):
        d = bs.fetch(u)
        assert np.array_equal(v.log_prob().view(np.uint32), d.log_prob().view(np.uint32))
        d.destroy()


# ------------------------------------------------------------------ reference softmax mode
# PK_MI355_SOFTMAX_REFERENCE: the reference's softmax / log operations one by one (libm expf and
# logf restated, csrc/pk_expf.h / pk_logf.h; float sum in column order; IEEE division).  With F32
# layers the whole path is then the reference's bit patterns.

def _bits_equal_nan(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both_nan, 0, a.view(np.uint32)),
                                                 np.where(both_nan, 0, b.view(np.uint32)))


@pytest.mark.parametrize("T,N", [(1, 50), (63, 64), (64, 65), (129, 3000), (33, 3008), (33, 3009), (70, 8000)])   # 3008 | 3009: register kernel | two-pass kernel
def test_reference_softmax_probabilities_bit_exact(T, N):
    rng = np.random.default_rng(T + N)
    W = (rng.standard_normal((N, 48)) * 0.4).astype(np.float32)
    layers = [("linear", W, (rng.standard_normal(N) * 0.5).astype(np.float32)), ("softmax",)]
    x = rng.standard_normal((T, 48)).astype(np.float32)
    am = pk.AcousticModel(layers, num_pdfs=N).set_softmax("reference")
    assert bits_equal(am.propagate(x), O.Nnet(layers).propagate(x))


@pytest.mark.parametrize("T", [1, 47, 300])
def test_reference_softmax_decodable_bit_exact(T):
    layers, prior, L, R, tid2pdf = tiny_model()
    feats = np.random.default_rng(T).standard_normal((T, 40)).astype(np.float32)
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf).set_softmax("reference")
    assert bits_equal(pk.Decodable(am, 0.1, feats).log_prob(), O.Nnet(layers).am_compute(feats, prior, L, R, 0.1))


def test_reference_softmax_overflow_like_the_reference():
    """Logits above 88.7: expf overflows, the sum is inf, that element becomes inf/inf = NaN and the
    rest of the row e/inf = 0 -> floor (vector.cc:265-277 has no max subtraction).  That is the reference's
    ARITHMETIC, i.e. what it computes with assertions compiled out (-DNDEBUG; pinned to that build of the real
    reference by tests/test_oracle_ref_am.py and tests/golden/ref_am_path.npz).  As its Makefile.am builds it,
    with assertions on, the reference aborts on this input at vector.cc:336 (assert(data_[i] >= 0.0) in ApplyLog:
    NaN fails it).  The product reproduces the arithmetic and does not abort."""
    N = 200
    W = np.zeros((N, 40), np.float32)
    b = np.linspace(-120.0, 95.0, N).astype(np.float32)        # some logits beyond 88.72, some below -103.97
    layers = [("linear", W, b), ("softmax",)]
    prior = np.full(N, 1.0 / N, np.float32)
    feats = np.zeros((5, 40), np.float32)
    ref = O.Nnet(layers).am_compute(feats, prior, 0, 0, 0.1)
    am = pk.AcousticModel(layers, prior, 0, 0).set_softmax("reference")
    gpu = pk.Decodable(am, 0.1, feats).log_prob()
    assert np.isnan(ref).any() and _bits_equal_nan(gpu, ref)
    # the default tail stays finite on the same input
    am2 = pk.AcousticModel(layers, prior, 0, 0)
    assert np.isfinite(pk.Decodable(am2, 0.1, feats).log_prob()).all()


def test_reference_softmax_whole_path_is_bit_identical_to_the_reference():
    """PCM -> fbank -> CMVN -> splice -> 4 x 1024 ReLU -> 3000 softmax -> log-likelihoods, model S,
    three ragged utterances in one batch: every float equals the CPU path's."""
    layers, prior, L, R = synth.model("S")
    g = synth.global_cmvn_stats()
    waves = [synth.utterance(70 + u, seconds=s) for u, s in enumerate([2.0, 0.7, 7.1])]   # 7.1 s: the window slides
    am = pk.AcousticModel(layers, prior, L, R).set_softmax("reference")
    bs = pk.BatchScorer(am, g, len(waves), sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    nn = O.Nnet(layers)
    for u, w in enumerate(waves):
        ref = nn.am_compute(O.cmvn(g, O.Fbank().compute(w)), prior, L, R, 0.1)
        assert bits_equal(bs.fetch(u).log_prob(), ref)


# ------------------------------------------------------------------ seeded fuzz
@pytest.mark.parametrize("seed", fuzz_seeds(6))
def test_fuzz_ragged_batches_every_stage(seed, monkeypatch):
    """Random ragged batches (lengths around the frame, CMVN-tile, window and chunk boundaries),
    random chunk size and lane count, int16 or float ingestion: features bit-exact per utterance,
    log-likelihoods bit-exact in reference-softmax mode and within the contract in the default mode."""
    rng = np.random.default_rng(1000 + seed)
    layers, prior, L, R, tid2pdf = tiny_model()
    g = synth.global_cmvn_stats()
    special = [0, 399, 400, 559, 560, 400 + 63 * 160, 400 + 64 * 160, 400 + 599 * 160, 400 + 600 * 160,
               400 + 601 * 160, 400 + 639 * 160, 400 + 640 * 160]
    lens = [int(special[rng.integers(len(special))] + rng.integers(0, 160) * rng.integers(0, 2)) for _ in range(5)]
    lens += [int(rng.integers(0, 120000)) for _ in range(4)]
    waves = [synth.utterance(500 + 16 * seed + i, seconds=8.0)[:n] for i, n in enumerate(lens)]
    monkeypatch.setenv("PK_MI355_CHUNK", str(int(rng.choice([128, 384, 1024, 4096]))))
    monkeypatch.setenv("PK_MI355_LANES", str(int(rng.choice([1, 2]))))
    nn, fb = O.Nnet(layers), O.Fbank()
    refs = []
    for w in waves:
        f = fb.compute(w)
        c = O.cmvn(g, f)
        refs.append((f, c, nn.am_compute(c, prior, L, R, 0.1) if len(f) else None))
    for mode in ("reference", "stable"):
        am = pk.AcousticModel(layers, prior, L, R, tid2pdf).set_softmax(mode)
        bs = pk.BatchScorer(am, g, len(waves), max(sum(lens), 1))
        if seed % 2:
            bs.set_waves_i16([w.astype(np.int16) for w in waves])
        else:
            bs.set_waves(waves)
        bs.score(0.1)
        for u, (f, c, ll) in enumerate(refs):
            assert bs.num_frames(u) == len(f)
            if len(f) == 0:
                continue
            assert bits_equal(bs.fetch_fbank(u), f) and bits_equal(bs.fetch_cmvn(u), c)
            got = bs.fetch(u).log_prob()
            if mode == "reference":
                assert bits_equal(got, ll)
            else:
                assert_loglik_close(got, ll)


# ------------------------------------------------------------------ round-2 additions

def test_device_fft_bit_exact_vs_committed_real_reference_output():
    """The kernel's 512-point real FFT alone (pk_mi355_test_srfft512: the FFT passes + real
    post-pass FbankKernel runs) on tests/golden/ref_srfft512.npz["frames"] == ["spectra"], which
    are outputs of the REAL pk_srfft_compute (srfft.cc:371-461) built from the reference's own
    file in the build container (tests/golden/make_ref_fixtures.py).  A direct pin, bitwise."""
    z = np.load(os.path.join(G, "ref_srfft512.npz"))
    got = pk.device_srfft512(z["frames"])
    assert bits_equal(got, z["spectra"])
    # and against the oracle's restatement on more frames (incl. magnitudes of real PCM windows)
    rng = np.random.default_rng(21)
    frames = (rng.standard_normal((300, 512)) * rng.choice([1e-3, 1.0, 3e3, 3e4], size=(300, 1))).astype(np.float32)
    fft = O.Srfft(512)
    assert bits_equal(pk.device_srfft512(frames), np.stack([fft.forward(f) for f in frames]))


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_outputs_wider_than_the_tail_register_cache(prec):
    """More than 8192 pdfs: the three-pass tail (tail.hip TailWideKernel) takes over -- every column
    takes part in the softmax and is written (f16x3 used to drop columns >= 8192)."""
    N, D = 8200, 40
    rng = np.random.default_rng(8200)
    W = (rng.standard_normal((N, D)) * 0.3).astype(np.float32)
    b = (rng.standard_normal(N) * 0.5).astype(np.float32)
    layers = [("linear", W, b), ("softmax",)]
    prior = rng.uniform(0.5, 1.5, N)
    prior = (prior / prior.sum()).astype(np.float32)
    feats = rng.standard_normal((37, D)).astype(np.float32)
    am = pk.AcousticModel(layers, prior, 0, 0, precision=prec)
    lp = pk.Decodable(am, 0.1, feats).log_prob()
    ref = O.Nnet(layers).am_compute(feats, prior, 0, 0, 0.1)
    assert_loglik_close(lp, ref)
    p = am.propagate(feats)                       # probabilities, the kTailSoftmaxProb form
    assert np.allclose(p.sum(axis=1), 1.0, atol=1e-5) and np.all(p[:, 8192:] > 0)
    # no softmax layer: the plain floor / log / prior tail on a wide output
    layers2 = [("linear", np.abs(W), np.abs(b)), ("relu",)]
    lp2 = pk.Decodable(pk.AcousticModel(layers2, prior, 0, 0, precision=prec), 1.0, np.abs(feats)).log_prob()
    assert_loglik_close(lp2, O.Nnet(layers2).am_compute(np.abs(feats), prior, 0, 0, 1.0))


def test_f16x3_spliced_entry_needs_feature_dim_multiple_of_8():
    """the interleaved (hi, lo) frame row exists only for feat_dim % 8 == 0; other widths
    must fail loudly in pk_decodable_init instead of writing out of bounds."""
    rng = np.random.default_rng(3)
    W = rng.standard_normal((16, 60)).astype(np.float32)
    am = pk.AcousticModel([("linear", W, np.zeros(16, np.float32)), ("softmax",)],
                          np.full(16, 1 / 16, np.float32), 1, 1, precision="f16x3")     # feat_dim = 20
    with pytest.raises(pk.PkError, match="multiple of 8"):
        pk.Decodable(am, 0.1, rng.standard_normal((9, 20)).astype(np.float32))
    # the plain (non-spliced) entry pads rows itself and stays usable; f32 takes any width
    assert am.propagate(rng.standard_normal((9, 60)).astype(np.float32)).shape == (9, 16)
    am32 = pk.AcousticModel([("linear", W, np.zeros(16, np.float32)), ("softmax",)],
                            np.full(16, 1 / 16, np.float32), 1, 1)
    assert pk.Decodable(am32, 0.1, rng.standard_normal((9, 20)).astype(np.float32)).log_prob().shape == (9, 16)


def test_view_destroyed_after_its_batch_is_safe():
    """VERDICT r1 #10 (gpurun_out/seg.log): the reference's caller destroys its decodable
    unconditionally at the end (pocketkaldi.cc:247), possibly after pk_mi355_batch_destroy.  The
    arena lives until the batch AND the views of its last fetch_all are gone: reading such a view
    after the batch is destroyed is still valid, destroying the last one frees the arena, once.
    (include/pk_mi355.h promises less -- contents valid until the batch is scored again or destroyed --
    the longer lifetime is what makes the reference's unconditional destroy order safe.)"""
    import ctypes as C
    L_ = pk.lib()
    layers, prior, L, R = synth.model("tiny")
    am = pk.AcousticModel(layers, prior, L, R)
    waves = [synth.utterance(50 + u, 0.6) for u in range(3)] + [np.zeros(10, np.float32)]   # last: T = 0
    bs = pk.BatchScorer(am, synth.global_cmvn_stats(), len(waves), sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    want = [bs.fetch(u).log_prob() for u in range(len(waves))]
    arr = (pk.pk_decodable_t * len(waves))()
    assert L_.pk_mi355_batch_fetch_all(bs._h, arr, len(waves), 1) == 0
    L_.pk_mi355_batch_destroy(bs._h)            # the batch goes first ...
    bs._h = None
    for u in range(len(waves)):                 # ... the views are still readable ...
        lp = arr[u].log_prob
        if lp.ncol:
            got = np.ctypeslib.as_array(lp.data, shape=(lp.ncol, lp.nrow)).copy()
            assert bits_equal(got, want[u])
            assert L_.pk_decodable_islastframe(C.byref(arr[u]), lp.ncol - 1)
    for u in range(len(waves)):                 # ... and destroying them is safe (the last one releases the arena)
        L_.pk_decodable_destroy(C.byref(arr[u]))
        assert not arr[u].log_prob.data and arr[u].log_prob.ncol == 0
    # the heap is intact: malloc-backed decodables still work
    d = pk.Decodable(am, 0.1, np.zeros((5, 40), np.float32))
    assert d.log_prob().shape == (5, 50)
    d.destroy()
    # the nastiest order: the views of an EARLIER fetch_all are destroyed while the views of
    # the current one are outstanding, then the batch goes -- every view counts against its OWN generation,
    # so the current views must stay readable until the last of THEM is destroyed
    bs3 = pk.BatchScorer(am, synth.global_cmvn_stats(), 3, sum(len(w) for w in waves[:3]))
    bs3.set_waves(waves[:3])
    bs3.score(0.1)
    stale = (pk.pk_decodable_t * 3)()
    fresh = (pk.pk_decodable_t * 3)()
    assert L_.pk_mi355_batch_fetch_all(bs3._h, stale, 3, 1) == 0
    bs3.score(0.1)
    assert L_.pk_mi355_batch_fetch_all(bs3._h, fresh, 3, 1) == 0
    assert stale[0].am != fresh[0].am and fresh[0].am == fresh[2].am      # one (opaque) generation handle per fetch_all
    for u in range(3):
        L_.pk_decodable_destroy(C.byref(stale[u]))      # three stale destroys: the current generation still counts 3
    L_.pk_mi355_batch_destroy(bs3._h)
    bs3._h = None
    for u in range(3):
        lp = fresh[u].log_prob
        assert bits_equal(np.ctypeslib.as_array(lp.data, shape=(lp.ncol, lp.nrow)), want[u])
        assert L_.pk_decodable_loglikelihood(C.byref(fresh[u]), 0, 7) == want[u][0, 7]
    keep = [(fresh[u].log_prob.ncol, fresh[u].log_prob.nrow, fresh[u].log_prob.data, fresh[u].am) for u in range(3)]
    late = (pk.pk_decodable_t * 3)()
    for u in range(3):                                   # bitwise copies, destroyed after the originals
        late[u].log_prob.ncol, late[u].log_prob.nrow, late[u].log_prob.data, late[u].am = keep[u]
        L_.pk_decodable_destroy(C.byref(fresh[u]))       # the last of these releases the arena
    for u in range(3):
        L_.pk_decodable_destroy(C.byref(late[u]))        # views of a generation that is gone: a no-op, not a free()
    # the copy of a destroyed view is destroyed only after the generation's record has been
    # recycled for a LATER fetch_all (records are reused once 64 more have been retired): it must not count
    # against the generation that now lives in that record
    bs4 = pk.BatchScorer(am, synth.global_cmvn_stats(), 3, sum(len(w) for w in waves[:3]))
    bs4.set_waves(waves[:3])
    bs4.score(0.1)
    first = (pk.pk_decodable_t * 3)()
    assert L_.pk_mi355_batch_fetch_all(bs4._h, first, 3, 1) == 0
    ghosts = (pk.pk_decodable_t * 3)()
    for u in range(3):
        ghosts[u].log_prob.ncol, ghosts[u].log_prob.nrow, ghosts[u].log_prob.data, ghosts[u].am = (
            first[u].log_prob.ncol, first[u].log_prob.nrow, first[u].log_prob.data, first[u].am)
        L_.pk_decodable_destroy(C.byref(first[u]))
    handles = set()
    cur = (pk.pk_decodable_t * 3)()
    for i in range(200):
        assert L_.pk_mi355_batch_fetch_all(bs4._h, cur, 3, 1) == 0
        handles.add(cur[0].am & ~63)
        if i < 199:
            for u in range(3):
                L_.pk_decodable_destroy(C.byref(cur[u]))
    assert (ghosts[0].am & ~63) in handles and ghosts[0].am != cur[0].am      # the record WAS recycled; the serial moved on
    for u in range(3):
        L_.pk_decodable_destroy(C.byref(ghosts[u]))      # three ghost destroys: ignored
    L_.pk_mi355_batch_destroy(bs4._h)
    bs4._h = None
    for u in range(3):                                   # the current generation still owns the arena
        lp = cur[u].log_prob
        assert bits_equal(np.ctypeslib.as_array(lp.data, shape=(lp.ncol, lp.nrow)), want[u])
    for u in range(3):
        L_.pk_decodable_destroy(C.byref(cur[u]))
    # Python mirror: closing the scorer while views are alive, views die later
    bs2 = pk.BatchScorer(am, synth.global_cmvn_stats(), 3, sum(len(w) for w in waves[:3]))
    bs2.set_waves(waves[:3])
    bs2.score(0.1)
    views = bs2.fetch_all()
    bs2.close()
    assert bits_equal(views[1].log_prob(), want[1])
    del views


def test_one_model_shared_by_host_threads():
    """the reference's pk_decodable_init is re-entrant for a shared model (nnet.cc:149-163
    allocates per call); ours serialises on a per-model lock -- concurrent callers get their own,
    correct results."""
    import threading
    layers, prior, L, R, tid2pdf = tiny_model()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    rng = np.random.default_rng(99)
    feats = [rng.standard_normal((40 + 37 * i, 40)).astype(np.float32) for i in range(6)]
    want = [pk.Decodable(am, 0.1, f).log_prob() for f in feats]
    got = [None] * len(feats)
    errs = []

    def work(i):
        try:
            for _ in range(5):
                got[i] = pk.Decodable(am, 0.1, feats[i]).log_prob()
        except Exception as e:      # noqa
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(feats))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    for a, b in zip(got, want):
        assert bits_equal(a, b)


def test_more_utterances_than_cus():
    """300 short utterances: the CMVN kernel (one workgroup per utterance, 117 KiB of LDS: one per CU)
    needs more than one round of workgroups; features and log-likelihoods per utterance as alone."""
    layers, prior, L, R, tid2pdf = tiny_model()
    g = synth.global_cmvn_stats()
    rng = np.random.default_rng(300)
    lens = [int(rng.integers(400, 12000)) for _ in range(300)]
    waves = [synth.utterance(2000 + i, 0.75)[:n] for i, n in enumerate(lens)]
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf).set_softmax("reference")
    bs = pk.BatchScorer(am, g, len(waves), sum(lens))
    bs.set_waves(waves)
    bs.score(0.1)
    nn, fb = O.Nnet(layers), O.Fbank()
    for u in (0, 1, 127, 255, 256, 257, 299):
        f = fb.compute(waves[u])
        c = O.cmvn(g, f)
        assert bits_equal(bs.fetch_fbank(u), f) and bits_equal(bs.fetch_cmvn(u), c)
        assert bits_equal(bs.fetch(u).log_prob(), nn.am_compute(c, prior, L, R, 0.1))


# ------------------------------------------------------------------ plain fp16 mode (PK_MI355_PRECISION_F16)
# ONE fp16 MFMA per product on the hi halves only: the throughput ceiling of the fp16 matrix cores at a
# STATED tolerance of its own -- outside the path's 1e-4 contract, so the
# test states the looser bar and prints what was measured.

def test_plain_f16_mode_states_its_own_tolerance(capsys):
    layers, prior, L, R = synth.model("S")
    wave = synth.utterance(0, seconds=3.0)
    g = synth.global_cmvn_stats()
    ref = O.Nnet(layers).am_compute(O.cmvn(g, O.Fbank().compute(wave)), prior, L, R, 0.1)
    errs, agree = {}, {}
    for prec in ("f16x3", "f16"):
        am = pk.AcousticModel(layers, prior, L, R, precision=prec)
        bs = pk.BatchScorer(am, g, 1, wave.shape[0])
        bs.set_waves([wave])
        bs.score(0.1)
        got = bs.fetch(0).log_prob()
        errs[prec] = float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)))
        agree[prec] = float(np.mean(np.argmax(got, axis=1) == np.argmax(ref, axis=1)))
    with capsys.disabled():
        print("\n  max |err| / max(|ref|, 1) on log-likelihoods, model S: f16x3 %.2e, plain f16 %.2e; "
              "top-1 pdf agreement %.4f / %.4f" % (errs["f16x3"], errs["f16"], agree["f16x3"], agree["f16"]))
    assert errs["f16x3"] < 1e-4                     # the contract
    assert 1e-5 < errs["f16"] < 2e-2                # plain fp16: its own, looser, stated bar (measured ~1e-3)
    assert agree["f16"] > 0.97                      # the frame-level decision is barely affected


@pytest.mark.parametrize("D,L,R", [(40, 5, 5), (8, 3, 2), (6, 4, 4), (7, 2, 1)])
def test_spliced_first_layer_big_tiles_any_feature_dimension(D, L, R):
    """The 128 x 128-tile kernel's spliced operand (am.cc:65-88 as an address function) for even and odd
    feature dimensions; dimensions below the 16-row k-slab wrap more than once per slab (round 1 wrapped
    at most once: wrong addresses for feature dimensions below 16 in the big-tile variant).  4096-row passes x 1536 outputs = 384 tiles of 128: the big-tile variant."""
    rng = np.random.default_rng(D * 100 + L)
    K, N, T = D * (L + R + 1), 1536, 9000
    W = (rng.standard_normal((N, K)) * np.sqrt(2.0 / K)).astype(np.float32)
    layers = [("linear", W, (rng.standard_normal(N) * 0.1).astype(np.float32)), ("relu",),
              ("linear", (rng.standard_normal((30, N)) * 0.1).astype(np.float32), np.zeros(30, np.float32)), ("softmax",)]
    prior = np.full(30, 1 / 30, np.float32)
    feats = rng.standard_normal((T, D)).astype(np.float32)
    am = pk.AcousticModel(layers, prior, L, R).set_softmax("reference")
    got = pk.Decodable(am, 0.1, feats).log_prob()
    rows = np.r_[0:300, T // 2:T // 2 + 300, T - 300:T]
    ref = O.Nnet(layers).am_compute(feats, prior, L, R, 0.1)
    assert bits_equal(got[rows], ref[rows]) and bits_equal(got, ref)


@pytest.mark.parametrize("seed", fuzz_seeds(24))
def test_fuzz_layer_stacks_bit_exact(seed):
    """Random layer stacks through Nnet::Propagate (nnet.cc:149-163): random widths (not multiples of
    anything), depths, ReLU / Normalize in any position, optional softmax (reference arithmetic), random
    frame counts -- every output bit equal to the oracle's."""
    from refmodel_files import random_stack
    layers, x, dims = random_stack(seed)
    T = x.shape[0]
    am = pk.AcousticModel(layers, num_pdfs=dims[-1]).set_softmax("reference")
    got, ref = am.propagate(x), O.Nnet(layers).propagate(x)
    assert _bits_equal_nan(got, ref), "layers %s T %d dims %s" % ([l[0] for l in layers], T, dims)


@pytest.mark.parametrize("seed", fuzz_seeds(16))
def test_fuzz_decodable_contexts_and_dimensions(seed):
    """pk_decodable_init (decodable.cc:8-17) with random feature dimension, left / right context, widths
    and frame counts (one frame up to several 4096-frame passes): bit-identical to AcousticModel::Compute
    in the oracle with the reference softmax, and the lookup semantics of decodable.cc:24-36."""
    rng = np.random.default_rng(777 + seed)
    D = int(rng.integers(1, 49))
    L, R = int(rng.integers(0, 7)), int(rng.integers(0, 7))
    H, N = int(rng.integers(1, 300)), int(rng.integers(2, 400))
    K = D * (L + R + 1)
    layers = [("linear", (rng.standard_normal((H, K)) * np.sqrt(2.0 / K)).astype(np.float32),
               (rng.standard_normal(H) * 0.1).astype(np.float32)), ("relu",),
              ("linear", (rng.standard_normal((N, H)) * np.sqrt(2.0 / H)).astype(np.float32),
               (rng.standard_normal(N) * 0.1).astype(np.float32)), ("softmax",)]
    prior = rng.uniform(0.5, 1.5, N)
    prior = (prior / prior.sum()).astype(np.float32)
    T = int(rng.choice([1, 2, 5, 64, 500, 4096, 4097, 9000]))
    feats = rng.standard_normal((T, D)).astype(np.float32)
    tid2pdf = np.concatenate([[0], rng.integers(0, N, 40)]).astype(np.int32)
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf).set_softmax("reference")
    d = pk.Decodable(am, 0.1, feats)
    ref = O.Nnet(layers).am_compute(feats, prior, L, R, 0.1)
    assert bits_equal(d.log_prob(), ref), "D %d L %d R %d H %d N %d T %d" % (D, L, R, H, N, T)
    assert d.is_last_frame(T - 1) and not d.is_last_frame(T - 2 if T > 1 else -1)
    assert d.loglikelihood(T - 1, 7) == ref[T - 1, tid2pdf[7]]


@pytest.mark.parametrize("seed", fuzz_seeds(10))
def test_fuzz_f16x3_decodable_within_contract(seed):
    """f16x3 through pk_decodable_init with random (multiple-of-8) feature dimensions, contexts, widths,
    depths and frame counts: inside the 1e-4 contract everywhere, measured error an order below."""
    rng = np.random.default_rng(999 + seed)
    D = 8 * int(rng.integers(1, 7))
    L, R = int(rng.integers(0, 6)), int(rng.integers(0, 6))
    dims = [D * (L + R + 1)] + [int(rng.integers(8, 600)) for _ in range(int(rng.integers(1, 4)))] + [int(rng.integers(2, 700))]
    layers = []
    for i in range(len(dims) - 1):
        layers.append(("linear", (rng.standard_normal((dims[i + 1], dims[i])) * np.sqrt(2.0 / dims[i])).astype(np.float32),
                       (rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32)))
        layers.append(("relu",) if i < len(dims) - 2 else ("softmax",))
        # round 3: NormalizeLayer (nnet.cc:62-75) between two affine layers -- the relu + renormalize stacks
        # tool/convert_am.py writes -- with or without the ReLU in front of it
        if i < len(dims) - 2 and rng.random() < 0.4:
            if rng.random() < 0.25:
                layers.pop()
            layers.append(("normalize",))
    prior = rng.uniform(0.5, 1.5, dims[-1])
    prior = (prior / prior.sum()).astype(np.float32)
    T = int(rng.choice([1, 3, 255, 256, 257, 1000, 4500]))
    feats = rng.standard_normal((T, D)).astype(np.float32)
    got = pk.Decodable(pk.AcousticModel(layers, prior, L, R, precision="f16x3"), 0.1, feats).log_prob()
    ref = O.Nnet(layers).am_compute(feats, prior, L, R, 0.1)
    # a frame whose activations are all zero in front of a Normalize is NaN in the reference (0 * inf, nnet.cc:62-75;
    # seeds 20266, 20306, 21638 of the round-3 soak: tiny random nets); f16x3 operands saturate instead of carrying
    # NaN (include/pk_mi355.h), so those frames are outside this mode's contract -- and finite here
    bad = np.isnan(ref).any(axis=1)
    assert np.all(np.isfinite(got))
    assert bad.mean() < 0.5
    got, ref = got[~bad], ref[~bad]
    assert_loglik_close(got, ref)
    assert got.size == 0 or np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)) < 2e-5, "dims %s L %d R %d T %d" % (dims, L, R, T)


def _random_net(rng, dims, normalize_p=0.0):
    layers = []
    for i in range(len(dims) - 1):
        layers.append(("linear", (rng.standard_normal((dims[i + 1], dims[i])) * np.sqrt(2.0 / dims[i])).astype(np.float32),
                       (rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32)))
        if i < len(dims) - 2:
            layers.append(("relu",))
            if rng.random() < normalize_p:
                layers.append(("normalize",))
        else:
            layers.append(("softmax",))
    prior = rng.uniform(0.5, 1.5, dims[-1])
    return layers, (prior / prior.sum()).astype(np.float32)


@pytest.mark.parametrize("seed", fuzz_seeds(6))
def test_fuzz_big_tile_decodable(seed):
    """The 128 x 128-tile GEMM variants (gemm.hip LaunchGeo<2>: spliced first layer, accumulation over
    several 512-chunks, swapped roles for the last layer) through pk_decodable_init: widths 1400-2300 that
    are multiples of nothing, any feature dimension and context, 4096-frame passes -- bit-identical to
    the oracle's AcousticModel::Compute with the reference softmax."""
    rng = np.random.default_rng(31337 + seed)
    D = int(rng.integers(1, 49))
    L, R = int(rng.integers(0, 7)), int(rng.integers(0, 7))
    hidden = [int(rng.integers(1537, 2300)) for _ in range(int(rng.integers(1, 3)))]
    dims = [D * (L + R + 1)] + hidden + [int(rng.integers(1410, 3100))]
    layers, prior = _random_net(rng, dims, normalize_p=0.25)
    T = int(rng.choice([4096, 4100, 6000, 8200]))
    feats = rng.standard_normal((T, D)).astype(np.float32)
    am = pk.AcousticModel(layers, prior, L, R).set_softmax("reference")
    got = pk.Decodable(am, 0.1, feats).log_prob()
    ref = O.Nnet(layers).am_compute(feats, prior, L, R, 0.1)
    assert bits_equal(got, ref), "dims %s L %d R %d T %d layers %s" % (dims, L, R, T, [l[0] for l in layers])


@pytest.mark.parametrize("seed", fuzz_seeds(4))
def test_fuzz_batches_wide_model_both_precisions(seed, monkeypatch):
    """Ragged batches through the batched scorer with a model wide enough for the big-tile kernels of
    both precisions, random layer-stack chunk: f32 bit-identical with the reference softmax and within
    the contract with the default tail; f16x3 within the contract."""
    rng = np.random.default_rng(90210 + seed)
    dims = [440] + [int(rng.integers(520, 1300)) for _ in range(int(rng.integers(2, 4)))] + [int(rng.integers(900, 2100))]
    layers, prior = _random_net(rng, dims)
    g = synth.global_cmvn_stats()
    lens = [int(rng.integers(400, 64000)) for _ in range(int(rng.integers(12, 30)))]
    waves = [synth.utterance(9000 + 64 * seed + i, seconds=4.0)[:n] for i, n in enumerate(lens)]
    monkeypatch.setenv("PK_MI355_CHUNK", str(int(rng.choice([1024, 4096, 8192, 131072]))))
    nn, fb = O.Nnet(layers), O.Fbank()
    refs = [nn.am_compute(O.cmvn(g, fb.compute(w)), prior, 5, 5, 0.1) for w in waves]
    for prec, mode in (("f32", "reference"), ("f32", "stable"), ("f16x3", "stable")):
        am = pk.AcousticModel(layers, prior, 5, 5, precision=prec).set_softmax(mode)
        bs = pk.BatchScorer(am, g, len(waves), sum(lens))
        bs.set_waves_i16([w.astype(np.int16) for w in waves])
        bs.score(0.1)
        for u, ll in enumerate(refs):
            got = bs.fetch(u).log_prob()
            if mode == "reference":
                assert bits_equal(got, ll), "dims %s utt %d" % (dims, u)
            else:
                assert_loglik_close(got, ll)



@pytest.mark.parametrize("N", [700, 1000, 1501, 3000, 4090, 5000, 6100, 8000])
def test_fp32_fused_tail_equals_the_stand_alone_wave_tail(N, monkeypatch):
    """PK_MI355_FUSED_TAIL32=1 (round-4 experiment switch): in fp32 mode the last affine layer's big-tile launch
    finishes the log-softmax tail itself (gemm.hip, TAIL variant: the workgroup that completes a 128-row tile of
    logits turns its rows into log-likelihoods), everything else takes TailWaveKernel; both run pk_tail_wave.h, so
    the two must agree bit for bit at every register-cache width, over several chunks and a ragged last tile; the
    fused run launches no tail kernel; and the wave arithmetic (hardware exp2, DPP trees) sits inside the contract
    against the oracle and within 1e-5 of the shipped TailKernel."""
    rng = np.random.default_rng(N)
    layers, prior = _random_net(rng, [440, 264, N])
    g = synth.global_cmvn_stats()
    lens = [int(rng.integers(8000, 64000)) for _ in range(40)]
    waves = [synth.utterance(7300 + i, seconds=4.0)[:n].astype(np.int16) for i, n in enumerate(lens)]
    monkeypatch.setenv("PK_MI355_CHUNK", "16384")
    got = {}
    for name, env in (("kernel", {"PK_MI355_FUSED_TAIL32": "0"}),
                      ("wave", {"PK_MI355_FUSED_TAIL32": "1", "PK_MI355_FUSED_TAIL_MIN_TILES": "100000000"}),
                      ("fused", {"PK_MI355_FUSED_TAIL32": "1", "PK_MI355_FUSED_TAIL_MIN_TILES": "384"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        am = pk.AcousticModel(layers, prior, 5, 5)
        bs = pk.BatchScorer(am, g, len(waves), sum(lens))
        bs.set_waves_i16(waves)
        bs.enable_timing(True)
        for _ in range(2):                      # twice: the arrival counters must be back at zero
            bs.score(0.1)
        exact = (N + 255) // 256 in (4, 8, 12, 16, 24, 32)       # the row widths that have a fused form (pk_tail_wave.h)
        assert (bs.timing()["tail"][1] == 0) == (name == "fused" and exact), "only the fused run launches no tail kernel"
        got[name] = [bs.fetch(u).log_prob().copy() for u in range(len(waves))]
    for a, b in zip(got["wave"], got["fused"]):
        assert bits_equal(a, b)
    for a, b in zip(got["kernel"], got["fused"]):
        assert np.max(np.abs(a - b) / np.maximum(np.abs(a), 1.0)) < 1e-5
    nn, fb = O.Nnet(layers), O.Fbank()
    for u in (0, 17, 39):
        ref = nn.am_compute(O.cmvn(g, fb.compute(waves[u].astype(np.float32))), prior, 5, 5, 0.1)
        assert_loglik_close(got["fused"][u], ref)


@pytest.mark.parametrize("path", ["kernel", "wave", "fused"])
def test_stable_tail_keeps_nan_rows_nan(path, monkeypatch):
    """with the DEFAULT (stable) softmax a row with a NaN logit must come out NaN, as the reference's
    does (am.cc:109: `x < 1e-20` is false for NaN, so log(NaN) follows) -- v_max_f32(NaN, floor) returned the floor
    and turned such rows into plausible log-likelihoods with rc 0.  NaN features in a few frames make the rows within
    the splice context of those frames NaN and no others; all three tails: TailKernel (PK_MI355_FUSED_TAIL32=0), the
    stand-alone wave tail, and the tail fused into the last layer's launch (4 096-row chunk x 24 column tiles; the
    404-row remainder takes the wave tail)."""
    for k, v in {"kernel": {"PK_MI355_FUSED_TAIL32": "0"},
                 "wave": {"PK_MI355_FUSED_TAIL32": "1", "PK_MI355_FUSED_TAIL_MIN_TILES": "100000000"},
                 "fused": {"PK_MI355_FUSED_TAIL32": "1", "PK_MI355_FUSED_TAIL_MIN_TILES": "384"}}[path].items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(77)
    layers, prior = _random_net(rng, [440, 264, 3000])
    T = 4500
    feats = rng.standard_normal((T, 40)).astype(np.float32)
    bad_frames = [7, 2000, 4094, 4400]
    for t in bad_frames:
        feats[t, int(rng.integers(0, 40))] = np.nan
    am = pk.AcousticModel(layers, prior, 5, 5)
    got = pk.Decodable(am, 0.1, feats).log_prob()
    ref = O.Nnet(layers).am_compute(feats, prior, 5, 5, 0.1)
    nan_rows = np.isnan(ref).all(axis=1)
    want_rows = np.zeros(T, bool)
    for t in bad_frames:
        want_rows[max(0, t - 5):t + 6] = True
    assert np.array_equal(nan_rows, want_rows) and not np.isnan(ref[~nan_rows]).any()      # what the reference does
    gn, rn = np.isnan(got), np.isnan(ref)
    bad = np.flatnonzero((gn != rn).any(axis=1))
    assert bad.size == 0, ("NaN placement differs from the reference's in %d rows, first %s: NaN columns there -- here %s, reference %s"
                           % (bad.size, bad[:12].tolist(), gn[bad[:12]].sum(axis=1).tolist(), rn[bad[:12]].sum(axis=1).tolist()))
    assert_loglik_close(got[~nan_rows], ref[~nan_rows])


@pytest.mark.parametrize("T", [1930, 2048, 2049, 2177])
def test_fused_tail_at_the_smallest_launches_that_fuse(T):
    """The fused tail exists for big-tile launches (>= 384 tiles of 128 x 128); the strip launch takes one column tile
    away from the big-tile launch.  16 row tiles x 24 column tiles = 384 is the smallest launch that fuses: with the
    strip it would be 16 x 23 = 368 -- small-tile kernels, which carry no tail -- so there the strip must not be taken
    (round 5: it was, and no log-likelihoods were made: found by review, this is its test).  3 000 pdfs, T around
    16 x 128 rows and just past it (17 row tiles: 17 x 23 = 391, strip and fusion both)."""
    rng = np.random.default_rng(T)
    layers, prior = _random_net(rng, [440, 96, 3000])
    feats = rng.standard_normal((T, 40)).astype(np.float32)
    am = pk.AcousticModel(layers, prior, 5, 5)
    got = pk.Decodable(am, 0.1, feats).log_prob()
    assert_loglik_close(got, O.Nnet(layers).am_compute(feats, prior, 5, 5, 0.1))


def test_fused_tail_hand_off_repeats_bit_for_bit_at_the_benchmark_size():
    """The fused tail's owner reads logits other workgroups stored behind other XCDs' L2s (sc1 stores, an arrival
    counter, sc1 loads): a visibility bug there would be rare and would only show at sizes the fuzz tests do not
    reach.  tools/fused_tail_stress.py scores the full 256 x 10 s batch with the tail as its own launch, then N times
    fused, and compares every byte of [frames][pdfs] each time (soak: 2 000 passes of S, 300 of W; here 40 and 6)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fused_tail_stress", os.path.join(os.path.dirname(G), "..", "tools", "fused_tail_stress.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run("S", 256, 10.0, 40) == 0
    assert mod.run("W", 256, 10.0, 6) == 0
