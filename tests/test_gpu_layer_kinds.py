"""The layer kinds 4 to 8 on the GPU: every kind alone in both activation layouts, a stack of all
of them through the batch scorer, chunked, after poison, live and from a model file -- bit for bit against the composer
of tests/layer_cases.py (oracle affine layers, the numpy restatement of the rules) in softmax mode "reference" -- and
the refusals that need the device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import layer_cases as LC
from test_gpu_stream_features import run_jobs

pytestmark = pytest.mark.gpu

F32 = np.float32


def identity(D):
    return ("linear", np.eye(D, dtype=F32), np.zeros(D, F32))


def kind_cases():
    out = []
    for D in (7, 17, 129):
        v = LC.designed(1, D, 40 + D)[0]
        out += [(D, ("sigmoid",)), (D, ("tanh",)), (D, ("add", v)), (D, ("mul", v))]
    for O in (7, 17, 129):
        for G in (2, 5):
            out.append((O * G, ("pnorm", O)))
    return out


def case_id(c):
    return "%s-%d%s" % (c[1][0], c[0], "-to-%d" % c[1][1] if c[1][0] == "pnorm" else "")


# ---------------------------------------------------------------- 1. each kind alone

@pytest.mark.parametrize("case", kind_cases(), ids=case_id)
def test_each_kind_alone(case):
    """One identity-weight Linear of width D, then the kind.  Through pk.Decodable the activations are feature-major
    panels (the model's first layer reads the spliced view) and the rows are log(max(y, 1e-20)); through propagate they
    are frame-major rows behind the last Linear and the rows are the layer's own output, negative values included."""
    D, layer = case
    layers = [identity(D), layer]
    N = layer[1] if layer[0] == "pnorm" else D
    am = pk.AcousticModel(layers, np.ones(N, F32)).set_softmax("reference")
    try:
        for T in (1, 67):
            x = LC.designed(T, D, 7)
            want = LC.loglik(layers, x, np.ones(N, F32), 0, 0, 1.0)
            d = pk.Decodable(am, 1.0, x)
            got = d.log_prob()
            d.destroy()
            assert got.shape == (T, N)
            assert LC.same(got, want), (case_id(case), T, "panels")
            raw = LC.propagate(layers, x)
            assert LC.same(am.propagate(x), raw), (case_id(case), T, "rows")
            if T == 67:                                 # the designed non-finite values land where the composer has them
                assert np.isnan(raw).any() and np.isfinite(raw).any()
    finally:
        am.close()


def test_infinite_features_in_front_of_narrow_hidden_layers():
    """Hidden widths 4 and 6, no multiples of 16: the panels have padding rows, which the zero rows of the padded weights
    make 0 * inf = NaN for a frame that holds an infinite feature.  The next affine layer's k-padding must not meet them:
    the frame's real features are +-inf and 0, and the reference's logits are +-inf, not NaN in every output."""
    import grid_walk_cases as GW
    layers, prior = GW.row_layers()
    x = LC.designed(67, 2, 11)
    assert np.isinf(x).sum() == 2
    want = LC.loglik(layers, x, prior, 0, 0, 0.1)
    assert (np.isinf(x).any(axis=1) & np.isfinite(want).all(axis=1)).any()      # tanh saturates: such a row is finite, not NaN
    am = pk.AcousticModel(layers, prior).set_softmax("reference")
    try:
        d = pk.Decodable(am, 0.1, x)
        got = d.log_prob()
        d.destroy()
        assert LC.same(got, want)
    finally:
        am.close()


# ---------------------------------------------------------------- the stack

@pytest.fixture(scope="module")
def stack():
    """The stack's model, its features and the composer's rows: made once, shared, left unchanged."""
    layers, prior = LC.stack()
    feats = LC.stack_feats()
    want = [LC.loglik(layers, f, prior, LC.STACK_LEFT, LC.STACK_RIGHT, 0.1) for f in feats]
    assert all(np.isfinite(w).all() for w in want)
    am = pk.AcousticModel(layers, prior, LC.STACK_LEFT, LC.STACK_RIGHT).set_softmax("reference")
    yield {"layers": layers, "prior": prior, "feats": feats, "want": want, "am": am}
    am.close()


def score(am, feats, fs=None):
    own = fs is None
    if own:
        fs = pk.FeatureScorer(am, len(feats), sum(f.shape[0] for f in feats))
    fs.set_features(feats, "normalized")
    fs.score(0.1)
    out = [fs.fetch(u).log_prob() for u in range(len(feats))]
    if own:
        fs.close()
    return out


def assert_rows(got, want, what):
    assert len(got) == len(want)
    for u, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (what, u, a.shape, b.shape)
        for t in range(a.shape[0]):
            assert a[t].tobytes() == b[t].tobytes(), "%s: utterance %d row %d differs" % (what, u, t)


def test_stack_equals_the_composer(stack):
    assert stack["am"].feat_dim() == LC.STACK_FEAT_DIM and stack["am"].num_pdfs() == LC.STACK_PDFS
    assert_rows(score(stack["am"], stack["feats"]), stack["want"], "stack")


def test_stack_stable_tail_within_the_bound(stack):
    """The default tail (log-softmax in its stable form) on the same stack: the project's bound 1e-4 max(|ref|, 1)."""
    am = pk.AcousticModel(stack["layers"], stack["prior"], LC.STACK_LEFT, LC.STACK_RIGHT)
    try:
        for a, b in zip(score(am, stack["feats"]), stack["want"]):
            assert a.shape == b.shape and np.all(np.abs(a - b) <= 1e-4 * np.maximum(np.abs(b), 1.0))
    finally:
        am.close()


def test_stack_chunked(stack, monkeypatch):
    """264 frames under PK_MI355_CHUNK=128: three passes, the rows of the one-pass scorer."""
    monkeypatch.setenv("PK_MI355_CHUNK", "128")
    assert sum(LC.STACK_LENGTHS) > 2 * 128
    assert_rows(score(stack["am"], stack["feats"]), stack["want"], "chunked")


def test_padding_rows_under_poison(stack):
    """One scorer: first a batch whose features are NaN and 3e38, then the clean batch.  A p-norm that left the rows
    [out_dim, RoundUp(out_dim, 16)) of its destination unwritten would hand the first call's NaN to the next GEMM."""
    feats = stack["feats"]
    poison = []
    for u, f in enumerate(feats):
        p = np.full_like(f, np.nan if u % 2 == 0 else 3e38)
        p[::2, ::3] = 3e38 if u % 2 == 0 else np.nan
        poison.append(p)
    fs = pk.FeatureScorer(stack["am"], len(feats), sum(f.shape[0] for f in feats))
    try:
        dirty = score(stack["am"], poison, fs)
        assert all(np.isnan(d).all() for d in dirty[::2])              # (every frame of these holds a NaN)
        assert_rows(score(stack["am"], feats, fs), stack["want"], "after poison")
    finally:
        fs.close()


def test_stack_live(stack):
    """pk.OnlineFeatureScorer, every utterance pushed as 1, 2, 5 frames and then the rest."""
    feats = stack["feats"]
    sc = pk.OnlineFeatureScorer(stack["am"], len(feats), sum(f.shape[0] for f in feats))
    try:
        jobs = []
        for u, f in enumerate(feats):
            chunks, left = [], f.shape[0]
            for c in (1, 2, 5):
                if left > 0:
                    chunks.append(min(c, left))
                    left -= chunks[-1]
            if left:
                chunks.append(left)
            jobs.append({"slot": u, "kind": "normalized", "data": f, "chunks": chunks, "start": 0, "close_with_last": False})
        assert_rows(run_jobs(sc, jobs), stack["want"], "live")
    finally:
        sc.destroy()


def write_vec(path, v, fmt="f"):
    v = np.ascontiguousarray(v, F32 if fmt == "f" else np.int32)
    with open(path, "wb") as f:
        f.write(b"VEC0" + struct.pack("<ii", 4 * v.shape[0] + 4, v.shape[0]) + v.tobytes())


def test_stack_from_a_model_file(stack, tmp_path):
    """pk.write_nnet, then AcousticModel.read and pk_mi355_load_stats' key = value file: the rows of the model built in memory."""
    pk.write_nnet(str(tmp_path / "stack.nnet"), stack["layers"])
    write_vec(tmp_path / "stack.prior", stack["prior"])
    am = pk.AcousticModel.read(str(tmp_path / "stack.nnet"), str(tmp_path / "stack.prior"), None, LC.STACK_LEFT, LC.STACK_RIGHT,
                               LC.STACK_PDFS).set_softmax("reference")
    try:
        assert_rows(score(am, stack["feats"]), stack["want"], "read")
    finally:
        am.close()
    write_vec(tmp_path / "cmvn.bin", np.arange(LC.STACK_FEAT_DIM + 1) + 1.0)
    write_vec(tmp_path / "tid2pdf.bin", np.arange(LC.STACK_PDFS), "i")
    (tmp_path / "model.conf").write_text("cmvn_stats = cmvn.bin\nnnet = stack.nnet\nprior = stack.prior\nleft_context = %d\nright_context = %d\n"
                                         "num_pdfs = %d\ntid2pdf = tid2pdf.bin\n" % (LC.STACK_LEFT, LC.STACK_RIGHT, LC.STACK_PDFS))
    am, stats = pk.AcousticModel.load_stats(str(tmp_path / "model.conf"))
    try:
        assert stats.shape == (LC.STACK_FEAT_DIM + 1,)
        assert_rows(score(am.set_softmax("reference"), stack["feats"]), stack["want"], "load_stats")
    finally:
        am.close()


def test_model_files_through_load_and_the_command_line(tmp_path, capsys):
    """The golden recognizer's files with the network written by pk.write_nnet.  With a scale of ones and an offset of
    zeros in nnet2's place before the Softmax (kinds 5 and 4: x * 1 + 0) the command line prints what it prints for the
    golden model; with all five kinds pk_mi355_load gives the rows of the model built in memory, and the command line
    decodes."""
    import shutil
    from pocketkaldi_amd import recognize
    from refmodel_text import load_text_model
    from test_gpu_recognizer import CAT, CONF, DIR, HELLO
    layers, prior, L, R, tid2pdf, g = load_text_model()
    for name in ("wordloop.fst", "wordloop_words.bin", "refmodel_cmvn.bin", "refmodel.prior", "refmodel_tid2pdf.bin"):
        shutil.copy(os.path.join(DIR, name), tmp_path / name)
    rng = np.random.default_rng(8)
    same = layers[:-1] + [("mul", np.ones(18, F32)), ("add", np.zeros(18, F32)), ("softmax",)]
    five = [layers[0], ("tanh",), ("normalize",), layers[3], ("pnorm", 24), ("sigmoid",), layers[5], ("mul", rng.uniform(0.5, 2.0, 18).astype(F32)),
            ("add", rng.standard_normal(18).astype(F32)), ("softmax",)]
    conf = open(CONF).read()
    for name, net in (("same", same), ("five", five)):
        pk.write_nnet(str(tmp_path / (name + ".nnet")), net)
        (tmp_path / (name + ".conf")).write_text(conf.replace("refmodel.nnet", name + ".nnet"))

    (tmp_path / "waves.scp").write_text(HELLO + "\n" + CAT + "\n")

    def lines(conf_path):
        capsys.readouterr()
        rc = recognize.main([str(conf_path), str(tmp_path / "waves.scp")])
        out = capsys.readouterr()
        assert rc == 0, out.out + out.err
        return out.out.splitlines()

    want = lines(CONF)
    assert len(want) == 2 and lines(tmp_path / "same.conf") == want
    assert len(lines(tmp_path / "five.conf")) == 2
    waves = [pk.read_wav(HELLO), pk.read_wav(CAT)]
    loaded, stats = pk.AcousticModel.load(str(tmp_path / "five.conf"))
    built = pk.AcousticModel(five, prior, L, R, tid2pdf)
    try:
        assert stats.tobytes() == np.ascontiguousarray(g, F32).tobytes()
        rows = []
        for am in (loaded, built):
            bs = pk.BatchScorer(am, stats, 2, sum(len(w) for w in waves))
            bs.set_waves(waves)
            bs.score(0.1)
            rows.append([bs.fetch(u).log_prob() for u in range(2)])
            bs.close()
        assert all(r.shape[0] > 0 and np.isfinite(r).all() for r in rows[0])
        assert_rows(rows[0], rows[1], "pk_mi355_load")
    finally:
        loaded.close()
        built.close()


# ---------------------------------------------------------------- refusals that need the device

def test_refusals_on_the_device():
    W = np.eye(8, dtype=F32)
    with pytest.raises(pk.PkError, match=r"f16x3 / f16 precision supports \(Linear \[ReLU\] \[Normalize\]\)\+ \[Softmax\] networks only"):
        pk.AcousticModel([("linear", W, np.zeros(8, F32)), ("sigmoid",)], np.ones(8, F32), precision="f16x3")
    # a vector layer in front of the first Linear of a spliced input: built, refused when it is scored
    am = pk.AcousticModel([("mul", np.ones(8, F32)), ("linear", W, np.zeros(8, F32))], np.ones(8, F32), 1, 0)
    try:
        assert am.feat_dim() == 4
        with pytest.raises(pk.PkError, match="network must start with a linear layer"):
            pk.Decodable(am, 1.0, np.ones((5, 4), F32))
    finally:
        am.close()


# ---------------------------------------------------------------- the C++ mirror

def weight(k):
    k = (np.asarray(k, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return ((k >> np.uint64(16)).astype(F32) / F32(65536.0) - F32(0.5)) * F32(0.05)


def test_layer_kinds_example_equals_python():
    from test_cpp_ark_features import fnv
    from test_cpp_stream import build
    got = subprocess.run([build("layer_kinds_example")], capture_output=True, text=True)
    assert got.returncode == 0 and "layer_kinds_example ok" in got.stdout, got.stdout + got.stderr
    D, L, R, H, O, N, T = 6, 2, 1, 40, 10, 8, 37
    n_in = D * (L + R + 1)
    layers = [("linear", (F32(8.0) * weight(np.arange(H * n_in))).reshape(H, n_in), weight(1000003 + np.arange(H))), ("pnorm", O), ("normalize",),
              ("linear", (F32(8.0) * weight(2000003 + np.arange(N * O))).reshape(N, O), weight(3000017 + np.arange(N))),
              ("mul", F32(1.0) + F32(4.0) * weight(4000037 + np.arange(N))), ("softmax",)]
    prior = np.full(N, 1.0 / N, F32)
    feats = (F32(40.0) * weight(6000011 + np.arange(T * D))).reshape(T, D)
    am = pk.AcousticModel(layers, prior, L, R)
    try:
        d = pk.Decodable(am, 1.0, feats)
        rows = d.log_prob()
        d.destroy()
    finally:
        am.close()
    lines = got.stdout.splitlines()
    assert lines[0] == "frames %d pdfs %d" % (T, N)
    assert lines[1] == "row 17:" + "".join(" %.9g" % v for v in rows[17])
    assert lines[2] == "loglik " + fnv(rows.tobytes())
    want = LC.loglik(layers, feats, prior, L, R, 1.0)
    assert np.all(np.abs(rows - want) <= 1e-4 * np.maximum(np.abs(want), 1.0))
