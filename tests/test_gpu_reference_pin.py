"""The device against the REAL reference, bit for bit -- not against the oracle restatement alone.

With the reference softmax (set_softmax("reference")) and f32 layers the product claims the reference's bit patterns.
Two witnesses: tests/golden/ref_am_path.npz, committed outputs of the reference's own pcm_reader.cc / fbank.cc /
cmvn.cc / nnet.cc / am.cc / decodable.cc (always run), and the live library oracle/_ref/libpkref_am.so built from those
files (host code only; travels with the tree; skipped where absent).  The assertions-on flavour of that library aborts
on a NaN (vector.cc:336), so it is given finite cases only."""
import os

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth
from oracle import oracle as O
from refmodel_files import fuzz_seeds, load_ref_am_path, overflow_model, sha256_rows, write_model
from refmodel_text import DIR, load_text_model

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HELLO, CAT = os.path.join(G, "en-us-hello.wav"), os.path.join(G, "en-us-cat.wav")
needs_live = pytest.mark.skipif(not O.have_ref_am(), reason="oracle/_ref/libpkref_am.so not built")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, a.view(np.uint32)), np.where(both, 0, b.view(np.uint32)))


def within_contract(got, ref):
    """The project's log-likelihood contract, unchanged: |got - ref| <= 1e-4 * max(|ref|, 1).  -> (ok, max relative)"""
    assert got.shape == ref.shape
    rel = np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref.astype(np.float64)), 1.0)
    return bool(np.all(rel <= 1e-4)), float(rel.max()) if rel.size else 0.0


def batch(am, g, waves):
    bs = pk.BatchScorer(am, g, len(waves), max(sum(len(w) for w in waves), 1))
    bs.set_waves(waves)
    bs.score(0.1)
    return bs


# ------------------------------------------------------------------ against the committed outputs of the reference

def test_front_end_reproduces_the_reference_fixture():
    z = load_ref_am_path()
    stats = O.read_vec(os.path.join(G, "cmvn_stats.bin"))
    waves = {"hello": pk.read_wav(HELLO), "cat": pk.read_wav(CAT), "utt950": synth.utterance(950, seconds=7.3)}
    layers, prior, L, R = synth.model("tiny")
    bs = batch(pk.AcousticModel(layers, prior, L, R), stats, list(waves.values()))
    for u, (name, w) in enumerate(waves.items()):
        fb = pk.Fbank().compute(w)
        assert same_bits(fb, z["fbank_" + name]), name
        assert same_bits(pk.CMVN(stats, fb).get_frames(), z["cmvn_" + name]), name
        assert same_bits(bs.fetch_fbank(u), z["fbank_" + name]) and same_bits(bs.fetch_cmvn(u), z["cmvn_" + name]), name


def test_refmodel_log_likelihoods_reproduce_the_reference_fixture():
    """pk_mi355_load(refmodel.conf) -> process_acoustic, pk_decodable_init, the batch scorer and the online scorer
    (160-sample chunks): all the reference's pk_decodable_init bits."""
    z = load_ref_am_path()
    am, stats = pk.AcousticModel.load(os.path.join(DIR, "refmodel.conf"))
    am.set_softmax("reference")
    waves = [pk.read_wav(HELLO), pk.read_wav(CAT)]
    want = [z["ll_refmodel_hello"], z["ll_refmodel_cat"]]
    bs = batch(am, stats, waves)
    sc = pk.OnlineScorer(am, stats, 2, 4000)
    for u, (w, ref) in enumerate(zip(waves, want)):
        assert same_bits(pk.process_acoustic(am, stats, w, 0.1).log_prob(), ref)
        feats = pk.CMVN(stats, pk.Fbank().compute(w)).get_frames()
        assert same_bits(pk.Decodable(am, 0.1, feats).log_prob(), ref)
        assert same_bits(bs.fetch(u).log_prob(), ref)
        sc.open(u)
        rows = []
        for i in range(0, len(w) + 160, 160):
            if i < len(w):
                sc.push(u, w[i:i + 160])
            else:
                sc.close(u)
            sc.step(0.1)
            first, r = sc.fetch(u)
            if r.shape[0]:
                assert first == sum(x.shape[0] for x in rows)
                rows.append(r)
        assert same_bits(np.concatenate(rows), ref)


@pytest.mark.parametrize("name", ["S", "W"])
def test_synthetic_models_reproduce_the_reference_fixture(name):
    """47 x 3000 / 47 x 8000 log-likelihoods: the SHA-256 of the reference's matrix and three of its rows in full.
    f16x3 is not bit-exact by design: within the contract of the REFERENCE's rows."""
    z = load_ref_am_path()
    layers, prior, L, R = synth.model(name)
    am = pk.AcousticModel(layers, prior, L, R).set_softmax("reference")
    got = pk.Decodable(am, 0.1, z["cmvn_hello"]).log_prob()
    assert same_bits(got[[0, 23, 46]], z["ll_%s_hello_rows" % name])
    assert np.array_equal(sha256_rows(got), z["ll_%s_hello_sha256" % name])
    for prec in ("f32", "f16x3"):                                   # the default (stable) tail
        got = pk.Decodable(pk.AcousticModel(layers, prior, L, R, precision=prec), 0.1, z["cmvn_hello"]).log_prob()
        ok, worst = within_contract(got[[0, 23, 46]], z["ll_%s_hello_rows" % name])
        print("model %s %s, stable tail, against the reference's rows: max |err| / max(|ref|, 1) = %.3e" % (name, prec, worst))
        assert ok, worst


def test_overflowing_softmax_reproduces_the_reference_fixture():
    z = load_ref_am_path()
    layers, prior = overflow_model()
    am = pk.AcousticModel(layers, prior, 0, 0).set_softmax("reference")
    assert same_bits(pk.Decodable(am, 0.1, np.zeros((5, 40), np.float32)).log_prob(), z["ll_overflow"])


# ------------------------------------------------------------------ symbol isolation (the live library is host code)

ISOLATION_CHILD = """
import os, sys
sys.path[:0] = [%r, %r]
from oracle import oracle as O
from refmodel_files import load_ref_am_path
z = load_ref_am_path()
d = %r
ref = O.RefAm(os.path.join(d, "refmodel.conf"))
feats = O.ref_cmvn(O.read_vec(os.path.join(d, "refmodel_cmvn.bin")), z["fbank_hello"])
assert ref.decodable(feats, 0.1).tobytes() == z["ll_refmodel_hello"].tobytes()
assert "pocketkaldi_amd" not in sys.modules and "torch" not in sys.modules
assert not [l for l in open("/proc/self/maps") if "libamdhip64" in l or "libpk_mi355" in l or "libhsa" in l]
print("reference alone: ok")
"""


@needs_live
def test_reference_library_alone_in_a_process_without_the_device():
    """A fresh process that never imports the product or opens the device: the reference library gives the fixture's
    bytes, and no GPU runtime is mapped into that process afterwards (it is host code; nothing in it enters a GPU API)."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-S", "-c", ISOLATION_CHILD % (repo, os.path.join(repo, "tests"), DIR)],
                       capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p)))
    assert r.returncode == 0 and "reference alone: ok" in r.stdout, r.stdout + r.stderr


@needs_live
def test_reference_symbols_do_not_bind_to_the_product_library():
    """libpk_mi355.so exports pk_decodable_init / _destroy too (the drop-in boundary).  In a process that holds it --
    made globally visible here -- and after it has scored a batch, the reference's pkref_decodable still calls the
    REFERENCE's own functions (-Bsymbolic; only pkref_* exported): it returns the fixture's bytes.  The libraries define
    nothing but pkref_*, leave no pk_* symbol undefined and need no GPU runtime."""
    import ctypes
    import subprocess
    ctypes.CDLL(pk.lib_path(), mode=ctypes.RTLD_GLOBAL)
    layers, prior, L, R = synth.model("tiny")
    batch(pk.AcousticModel(layers, prior, L, R), synth.global_cmvn_stats(), [synth.utterance(1, 1.0)])
    z = load_ref_am_path()
    ref = O.RefAm(os.path.join(DIR, "refmodel.conf"))
    feats = O.ref_cmvn(O.read_vec(os.path.join(DIR, "refmodel_cmvn.bin")), z["fbank_hello"])
    assert same_bits(ref.decodable(feats, 0.1), z["ll_refmodel_hello"])
    for lib in ("libpkref_am.so", "libpkref_am_ndebug.so"):
        path = os.path.join(os.path.dirname(O.__file__), "_ref", lib)
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        names = [l.split()[-1] for l in out.splitlines() if l.strip()]
        assert names and all(n.startswith("pkref_") for n in names), names
        und = subprocess.check_output(["nm", "-D", "--undefined-only", path], text=True)
        assert " pk_" not in und and "hip" not in und.lower()
        assert "hip" not in subprocess.check_output(["ldd", path], text=True).lower()


# ------------------------------------------------------------------ against the live reference

def ragged_waves():
    """>= 8 utterances: 0-frame, 1-frame, 599 / 600 / 601 frames (the CMVN window fills), > 1300 frames."""
    frames = [47, 0, 1, 599, 600, 601, 1333, 3, 130]
    return [synth.utterance(700 + i, 14.0)[:(400 + 160 * (t - 1)) if t > 0 else 250] for i, t in enumerate(frames)], frames


def reference_stages(conf, g, waves, ndebug=False):
    am = O.RefAm(conf, ndebug=ndebug)
    out = []
    for w in waves:
        fb = O.ref_fbank(w, ndebug=ndebug)
        cm = O.ref_cmvn(g, fb, ndebug=ndebug)
        out.append((fb, cm, am.decodable(cm, 0.1)))
    return out


@needs_live
def test_ragged_batch_every_stage_equals_the_live_reference(tmp_path, monkeypatch):
    """Model "S" as NNT0 / VEC0 files: the reference reads them with its reader, the product with pk_mi355_load; fbank,
    CMVN and log-likelihoods equal bit for bit per utterance, whatever the chunk size and row layout.  The default
    (stable) tail against the same reference output under the contract."""
    layers, prior, L, R = synth.model("S")
    g = synth.global_cmvn_stats()
    conf = write_model(tmp_path, layers, prior, L, R, cmvn_stats=g)
    waves, frames = ragged_waves()
    want = reference_stages(conf, g, waves)
    for chunk, compact in ((None, None), ("128", "1"), ("8192", "0"), ("128", "0"), ("8192", "1")):
        if chunk:
            monkeypatch.setenv("PK_MI355_CHUNK", chunk)
            monkeypatch.setenv("PK_MI355_COMPACT_ROWS", compact)
        am, stats = pk.AcousticModel.load(conf)
        assert same_bits(stats, g)
        am.set_softmax("reference")
        bs = batch(am, stats, waves)
        for u, (fb, cm, ll) in enumerate(want):
            assert bs.num_frames(u) == frames[u] == fb.shape[0]
            assert same_bits(bs.fetch_fbank(u), fb) and same_bits(bs.fetch_cmvn(u), cm), (chunk, compact, u)
            assert same_bits(bs.fetch(u).log_prob().reshape(ll.shape), ll), (chunk, compact, u)
        bs.close()
    monkeypatch.delenv("PK_MI355_CHUNK")
    monkeypatch.delenv("PK_MI355_COMPACT_ROWS")
    worst = {}
    for prec in ("f32", "f16x3"):
        am, stats = pk.AcousticModel.load(conf, precision=prec)
        bs = batch(am, stats, waves)
        oks = [within_contract(bs.fetch(u).log_prob(), ll) for u, (_, _, ll) in enumerate(want) if frames[u]]
        worst[prec] = max(w for _, w in oks)
        print("model S %s, stable tail, against the live reference: max |err| / max(|ref|, 1) = %.3e" % (prec, worst[prec]))
        assert all(ok for ok, _ in oks), worst


@needs_live
@pytest.mark.parametrize("seed", fuzz_seeds(6))
def test_fuzz_contexts_dims_and_layer_patterns_equal_the_live_reference(seed, tmp_path):
    from test_gpu_parity import _random_net
    rng = np.random.default_rng(60606 + seed)
    D = int(rng.integers(1, 49))
    L, R = int(rng.integers(0, 7)), int(rng.integers(0, 7))
    dims = [D * (L + R + 1)] + [int(rng.integers(8, 600)) for _ in range(int(rng.integers(1, 4)))] + [int(rng.integers(2, 700))]
    layers, prior = _random_net(rng, dims, normalize_p=0.4)
    T = int(rng.choice([1, 2, 5, 64, 500, 4097]))
    feats = rng.standard_normal((T, D)).astype(np.float32)
    tid2pdf = np.concatenate([[0], rng.integers(0, dims[-1], 40)]).astype(np.int32)
    conf = write_model(tmp_path, layers, prior, L, R, tid2pdf)
    oracle = O.Nnet(layers).am_compute(feats, prior, L, R, 0.1)
    # (an all-zero row in front of a Normalize is NaN in the reference and aborts its assertions-on build at vector.cc:336)
    ref = O.RefAm(conf, ndebug=bool(np.isnan(oracle).any()))
    want = ref.decodable(feats, 0.1)
    am = pk.AcousticModel.read(os.path.join(tmp_path, "am.nnet"), os.path.join(tmp_path, "am.prior"),
                               os.path.join(tmp_path, "tid2pdf.bin"), L, R, dims[-1]).set_softmax("reference")
    d = pk.Decodable(am, 0.1, feats)
    assert same_bits(d.log_prob(), want) and same_bits(oracle, want), "dims %s L %d R %d T %d" % (dims, L, R, T)
    assert [am.transition_id_to_pdf_id(t) for t in range(41)] == [ref.tid2pdf(t) for t in range(41)]


# ------------------------------------------------------------------ the context-free model through the batch scorer

def context_free_waves():
    frames = [5, 1, 130, 0, 611, 3, 64] + [998] * 6                # 6 802 rows: "S"'s first layer (8 column tiles) takes the
    return [synth.utterance(800 + i, 10.0)[:(400 + 160 * (t - 1)) if t > 0 else 100] for i, t in enumerate(frames)], frames  # 128-wide tiles from 6 144


@pytest.mark.parametrize("which", ["S", "tiny"])
def test_context_free_model_through_the_batch_scorer(which, tmp_path, monkeypatch):
    """L = R = 0 through BatchScorer.  Compact rows pad an utterance's rows to four but not its columns, so with fewer
    than three context frames the column shift of a later utterance is negative, and the kernels add it to unsigned
    32-bit lane offsets of scalar-base LDS-DMA (a wrap to +4 GiB): pk_mi355_batch_create therefore keeps such models in
    the row = column layout.  Lengths that end inside, at and across groups of four rows, a batch large enough for the
    128-wide tiles, one chunk and 128-row chunks, both settings of the layout switch: f32 + reference softmax
    bit-identical to the oracle and to the live reference; f16x3 within the contract."""
    layers, prior, L, R = synth.model(which, left=0, right=0)
    g = synth.global_cmvn_stats()
    waves, frames = context_free_waves()
    nn, fb = O.Nnet(layers), O.Fbank()
    want = [nn.am_compute(O.cmvn(g, fb.compute(w)), prior, 0, 0, 0.1) for w in waves]
    if O.have_ref_am():
        conf = write_model(tmp_path, layers, prior, 0, 0)
        for (_, _, ll), o in zip(reference_stages(conf, g, waves), want):
            assert same_bits(ll, o)
    for chunk in (None, "128"):
        for compact in ("1", "0"):
            monkeypatch.setenv("PK_MI355_COMPACT_ROWS", compact)
            if chunk:
                monkeypatch.setenv("PK_MI355_CHUNK", chunk)
            for prec in ("f32", "f16x3"):
                am = pk.AcousticModel(layers, prior, 0, 0, precision=prec)
                if prec == "f32":
                    am.set_softmax("reference")
                bs = batch(am, g, waves)
                for u, ref in enumerate(want):
                    got = bs.fetch(u).log_prob()
                    assert got.shape[0] == frames[u]
                    if frames[u] == 0:
                        continue
                    if prec == "f32":
                        assert same_bits(got, ref), (which, chunk, compact, u)
                    else:
                        ok, worst = within_contract(got, ref)
                        assert ok, (which, chunk, compact, u, worst)
                bs.close()


@pytest.mark.parametrize("L,R", [(1, 0), (1, 1)])
def test_one_and_two_context_frames_through_the_batch_scorer(L, R):
    """L + R = 1 and 2: the other two context sizes whose compact-row shift could go negative."""
    layers, prior, _, _ = synth.model("tiny", left=L, right=R)
    g = synth.global_cmvn_stats()
    waves, frames = context_free_waves()
    waves, frames = waves[:8], frames[:8]
    am = pk.AcousticModel(layers, prior, L, R).set_softmax("reference")
    bs = batch(am, g, waves)
    nn, fb = O.Nnet(layers), O.Fbank()
    for u, w in enumerate(waves):
        if frames[u]:
            assert same_bits(bs.fetch(u).log_prob(), nn.am_compute(O.cmvn(g, fb.compute(w)), prior, L, R, 0.1)), u
