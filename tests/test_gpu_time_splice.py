"""The time-splice layer, kind 9, on the GPU: the kind alone at the padding, tile and wave edges, a
stack with two such layers through every object that scores whole utterances -- ragged batches with an empty utterance,
poisoned neighbours, reused buffers, several passes on one and on two lanes, the decoder, a model file, the recognizer and
the C++ mirror -- bit for bit against tests/time_splice_cases.py's loglik_time (oracle affine layers, the numpy
restatement of the rules, the edge rule) in softmax mode "reference", and the refusals of the objects that do not take it."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth_graph as SG

import frontend_any_cases as FA
import layer_cases as LC
import refmodel_files as RF
import time_splice_cases as TC

pytestmark = pytest.mark.gpu

F32 = np.float32
ONLINE_REFUSAL = "time-splice layers are not supported by the online scorers yet"


def assert_rows(got, want, what):
    assert len(got) == len(want)
    for u, (a, b) in enumerate(zip(got, want)):
        if b.shape[0] == 0:                             # (an empty utterance's decodable has no rows and no width)
            assert a.shape[0] == 0, (what, u, a.shape)
            continue
        assert a.shape == b.shape, (what, u, a.shape, b.shape)
        for t in range(a.shape[0]):
            assert a[t].tobytes() == b[t].tobytes(), "%s: utterance %d row %d of %d differs" % (what, u, t, a.shape[0])


def score(am, feats, fs=None, scale=TC.SCALE):
    own = fs is None
    if own:
        fs = pk.FeatureScorer(am, len(feats), max(sum(f.shape[0] for f in feats), 1))
    fs.set_features(feats, "normalized")
    fs.score(scale)
    out = [fs.fetch(u).log_prob() for u in range(len(feats))]
    if own:
        fs.close()
    return out


# ---------------------------------------------------------------- a. the kind alone

alone_layers = TC.alone_layers


@pytest.mark.parametrize("offsets", [[0], [-1, 0, 1], [-3, 3], [0, 2], [-2, 1]], ids=lambda o: "o" + "_".join(str(v) for v in o))
@pytest.mark.parametrize("D", [7, 16, 17])
def test_the_kind_alone(D, offsets):
    """An identity Linear of width D, the splice, a seeded Linear n D -> 5, through pk.Decodable.  T = 1, 2 and 3 lie below
    the context (every row is made of edge frames); n D = 7, 21, 34, 51 are no multiples of 16 (padding rows)."""
    layers = alone_layers(D, offsets, 1)
    prior = np.ones(5, F32)
    am = pk.AcousticModel(layers, prior).set_softmax("reference")
    try:
        assert am.time_context() == TC.time_context(layers) == TC.lo_hi(offsets)
        for T in (1, 2, 3, 67):
            x = LC.designed(T, D, 7)
            want = TC.loglik_time(layers, x, prior, 0, 0, 1.0)
            d = pk.Decodable(am, 1.0, x)
            got = d.log_prob()
            d.destroy()
            assert got.shape == (T, 5)
            assert LC.same(got, want), (D, offsets, T)
            if T == 67:                                 # the designed non-finite values land where the composer has them
                assert np.isnan(want).any() and np.isfinite(want).any()
    finally:
        am.close()


# ---------------------------------------------------------------- b. the padding rows under poison

def test_padding_rows_under_poison():
    """One scorer: first a batch whose features are NaN and 3e38, then the clean batch.  Linear 24 -> 10, splice [-1, 2]
    (20 rows, 12 of padding up to 32), Linear 20 -> 12 + ReLU, Linear 12 -> 9, tanh, Linear 9 -> 7, Softmax: the splice is
    the first writer of its work buffer in a call, and the third Linear of the call before left NaN in all of that
    buffer's first 128 rows.  A splice that left rows [20, 32) unwritten would hand them to the next GEMM."""
    rng = np.random.default_rng(0xB01)
    layers = [LC._linear(rng, 24, 10), ("splice", [-1, 2]), LC._linear(rng, 20, 12), ("relu",), LC._linear(rng, 12, 9), ("tanh",),
              LC._linear(rng, 9, 7), ("softmax",)]
    prior = rng.uniform(0.05, 0.3, 7).astype(F32)
    feats = [f for f in TC.stack_feats() if f.shape[0]]
    want = [TC.loglik_time(layers, f, prior, 2, 1, TC.SCALE) for f in feats]
    assert all(np.isfinite(w).all() for w in want)
    poison = []
    for u, f in enumerate(feats):
        p = np.full_like(f, np.nan if u % 2 == 0 else 3e38)
        p[::2, ::3] = 3e38 if u % 2 == 0 else np.nan
        poison.append(p)
    am = pk.AcousticModel(layers, prior, 2, 1).set_softmax("reference")
    fs = pk.FeatureScorer(am, len(feats), sum(f.shape[0] for f in feats))
    try:
        dirty = score(am, poison, fs)
        assert all(np.isnan(d).all() for d in dirty[::2])              # (every frame of these holds a NaN)
        assert_rows(score(am, feats, fs), want, "after poison")
    finally:
        fs.close()
        am.close()


def test_offsets_of_zero_alone_change_no_layout():
    """A model whose only offset list is [0] has no time context: with left 2 / right 1 it keeps the compact rows, and
    propagate and the online scorers take it.  The layer is a copy between the two Linears."""
    rng = np.random.default_rng(0x0FF5)
    layers = [LC._linear(rng, 24, 10), ("splice", [0]), LC._linear(rng, 10, 7), ("softmax",)]
    prior = rng.uniform(0.05, 0.3, 7).astype(F32)
    feats = TC.stack_feats()
    want = [TC.loglik_time(layers, f, prior, 2, 1, TC.SCALE) for f in feats]
    am = pk.AcousticModel(layers, prior, 2, 1).set_softmax("reference")
    try:
        assert am.time_context() == (0, 0)
        assert_rows(score(am, feats), want, "offsets [0], compact rows")
        x = LC.O.splice(feats[4], 2, 1)
        assert am.propagate(x).tobytes() == TC.propagate_time(layers, x).tobytes()
        from test_gpu_stream_features import run_jobs
        sc = pk.OnlineFeatureScorer(am, 1, 200)
        try:
            jobs = [{"slot": 0, "kind": "normalized", "data": feats[4], "chunks": [1, 2, 5, feats[4].shape[0] - 8], "start": 0, "close_with_last": False}]
            assert_rows(run_jobs(sc, jobs), [want[4]], "offsets [0], live")
        finally:
            sc.destroy()
    finally:
        am.close()


# ---------------------------------------------------------------- c. tile and wave edges of the kernel

def test_tile_and_wave_edges():
    D, offsets = 17, [-3, 0, 3]
    layers = alone_layers(D, offsets, 2)
    prior = np.ones(5, F32)
    am = pk.AcousticModel(layers, prior).set_softmax("reference")
    fs = pk.FeatureScorer(am, 1, 261)
    try:
        for T in (127, 128, 129, 255, 256, 257, 261):
            x = (np.random.default_rng([0xED6E, T]).standard_normal((T, D)) * 2.0).astype(F32)
            want = TC.loglik_time(layers, x, prior, 0, 0, 1.0)
            assert_rows(score(am, [x], fs, 1.0), [want], "T = %d" % T)
    finally:
        fs.close()
        am.close()


# ---------------------------------------------------------------- the stack

@pytest.fixture(scope="module")
def stack():
    """The stack's model, its features and loglik_time's rows: made once, shared, left unchanged."""
    layers, prior = TC.stack()
    feats = TC.stack_feats()
    want = [TC.loglik_time(layers, f, prior, TC.LEFT, TC.RIGHT, TC.SCALE) for f in feats]
    assert all(np.isfinite(w).all() for w in want)
    am = pk.AcousticModel(layers, prior, TC.LEFT, TC.RIGHT, tid2pdf=np.arange(TC.PDFS, dtype=np.int32)).set_softmax("reference")
    yield {"layers": layers, "prior": prior, "feats": feats, "want": want, "am": am}
    am.close()


def test_stack_equals_loglik_time(stack):
    """d: fetch(u) for every u, fetch_all and gather_loglik on a ragged batch with an empty utterance in the middle."""
    am, feats, want = stack["am"], stack["feats"], stack["want"]
    assert am.feat_dim() == TC.FEAT_DIM and am.num_pdfs() == TC.PDFS and am.time_context() == (TC.LH, TC.RH)
    fs = pk.FeatureScorer(am, len(feats), sum(f.shape[0] for f in feats))
    try:
        assert_rows(score(am, feats, fs), want, "fetch")
        views = fs.fetch_all()
        assert_rows([v.log_prob() for v in views], want, "fetch_all")
        L_ = pk.lib()

        def to_device(arr):
            p = L_.pk_mi355_device_malloc(arr.nbytes)
            assert p and L_.pk_mi355_memcpy(p, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes, 1) == 0
            return p
        for u, w in enumerate(want):
            T = w.shape[0]
            if T == 0:
                continue
            rng = np.random.default_rng([0x6A7, u])
            frames = np.concatenate([[0, T - 1], rng.integers(0, T, 200)]).astype(np.int32)
            tids = rng.integers(1, TC.PDFS, frames.shape[0]).astype(np.int32)
            out = np.zeros(frames.shape[0], F32)
            df, dt, do = to_device(frames), to_device(tids), to_device(out)
            fs.gather_loglik(u, df, dt, frames.shape[0], do)
            fs.synchronize()
            assert L_.pk_mi355_memcpy(out.ctypes.data_as(ctypes.c_void_p), do, out.nbytes, 2) == 0
            for p in (df, dt, do):
                L_.pk_mi355_device_free(p)
            assert out.tobytes() == w[frames, tids].tobytes(), u
    finally:
        fs.close()


def test_stack_isolation_and_reuse(stack):
    """e: an utterance's rows are the same bits whether every other utterance is NaN / 3e38 or healthy, also after a
    larger poisoned batch on the same scorer."""
    am, feats, want = stack["am"], stack["feats"], stack["want"]
    big = TC.feats_of([40, 150, 7, 90, 131, 3, 64, 20], seed=9)
    fs = pk.FeatureScorer(am, len(big), sum(f.shape[0] for f in big))
    try:
        score(am, [np.full_like(f, np.nan if u % 2 else 3e38) for u, f in enumerate(big)], fs)      # the larger poisoned batch first
        for keep in range(len(feats)):
            if feats[keep].shape[0] == 0:
                continue
            mixed = [f if u == keep else np.full_like(f, np.nan if (u + keep) % 2 else 3e38) for u, f in enumerate(feats)]
            got = score(am, mixed, fs)
            assert got[keep].tobytes() == want[keep].tobytes(), keep
            assert all(np.isnan(g).all() for u, g in enumerate(got) if u != keep and g.shape[0] and (u + keep) % 2)
        assert_rows(score(am, feats, fs), want, "healthy after poison")
    finally:
        fs.close()


PASS_LENGTHS = [250, 9, 300, 5, 700]


@pytest.fixture(scope="module")
def passes(stack):
    feats = TC.feats_of(PASS_LENGTHS, seed=3)
    return feats, [TC.loglik_time(stack["layers"], f, stack["prior"], TC.LEFT, TC.RIGHT, TC.SCALE) for f in feats]


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_stack_in_passes(stack, passes, lanes, monkeypatch):
    """f: PK_MI355_CHUNK=128 makes passes of 256 rows: the utterances straddle pass boundaries (row 256 lies two rows
    behind the first utterance's last frame, inside its Rh virtual frames), on one lane and on two.  The rows are the
    one-pass scorer's and loglik_time's."""
    feats, want = passes
    one = score(stack["am"], feats)
    assert_rows(one, want, "one pass")
    monkeypatch.setenv("PK_MI355_CHUNK", "128")
    monkeypatch.setenv("PK_MI355_LANES", lanes)
    assert sum(PASS_LENGTHS) > 4 * 256
    assert_rows(score(stack["am"], feats), one, "passes of 256 rows, lanes = " + lanes)


def test_decodable_of_two_passes(stack):
    """f: 4 200 frames through pk.Decodable, more than the 4 096 rows of a pass of the model's own scorer."""
    x = TC.feats_of([4200], seed=5)[0]
    want = TC.loglik_time(stack["layers"], x, stack["prior"], TC.LEFT, TC.RIGHT, TC.SCALE)
    d = pk.Decodable(stack["am"], TC.SCALE, x)
    got = d.log_prob()
    d.destroy()
    assert_rows([got], [want], "4200 frames")
    short = pk.Decodable(stack["am"], TC.SCALE, stack["feats"][4])          # and a short one on the same buffers afterwards
    got = short.log_prob()
    short.destroy()
    assert_rows([got], [stack["want"][4]], "67 frames after 4200")


# ---------------------------------------------------------------- g. the decoder

def graph_file(tmp_path):
    g = SG.general(40, seed=5, num_pdfs=TC.PDFS)
    path = str(tmp_path / "general.fst")
    SG.write_fst(path, g["start"], g["final"], g["arcs"])
    return path


def test_decode_batch_reads_the_right_rows(stack, tmp_path):
    """decode_batch on the scored batch equals decode on the host rows fetch returned: a wrong out_base would not."""
    am, feats = stack["am"], stack["feats"]
    fst = pk.Fst(graph_file(tmp_path))
    fs = pk.FeatureScorer(am, len(feats), sum(f.shape[0] for f in feats))
    dec = pk.Decoder(fst, am, len(feats))
    try:
        rows = score(am, feats, fs)
        assert_rows(rows, stack["want"], "rows")
        dec.decode_batch(fs)
        got = [dec.result(u) for u in range(len(feats))]
        dec.decode(rows)
        want = [dec.result(u) for u in range(len(feats))]
        for u in range(len(feats)):
            assert got[u][0] == want[u][0] and np.float32(got[u][1]).tobytes() == np.float32(want[u][1]).tobytes() and got[u][2] == want[u][2], u
        assert any(w[2] == 1 for w in want)
    finally:
        dec.close()
        fs.close()
        fst.close()


# ---------------------------------------------------------------- h. from a file; the refusals

def write_symbols(path, n):
    words = [b"w%d" % i for i in range(n)]
    buf, offsets = b"", []
    for w in words:
        offsets.append(len(buf))
        buf += w + b"\0"
    with open(path, "wb") as f:
        f.write(b"SYM0" + struct.pack("<iii", 8 + 4 * n + len(buf), n, len(buf)) + struct.pack("<%di" % n, *offsets) + buf)


@pytest.fixture(scope="module")
def model_file(stack, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("time_splice_model")
    stats = np.concatenate([np.zeros(TC.FEAT_DIM), [100.0]]).astype(F32)
    conf = RF.write_model(tmp, [], stack["prior"], TC.LEFT, TC.RIGHT, tid2pdf=np.arange(TC.PDFS, dtype=np.int32), cmvn_stats=stats)
    pk.write_nnet(str(tmp / "am.nnet"), stack["layers"])
    graph_file(tmp)
    write_symbols(str(tmp / "words.bin"), 50)
    with open(conf, "a") as f:
        f.write("fst = general.fst\nsymbol_table = words.bin\n")
    return tmp, conf, stats


def test_stack_from_a_model_file(stack, model_file):
    tmp, conf, stats = model_file
    am = pk.AcousticModel.read(str(tmp / "am.nnet"), str(tmp / "am.prior"), None, TC.LEFT, TC.RIGHT, TC.PDFS).set_softmax("reference")
    try:
        assert am.time_context() == (TC.LH, TC.RH)
        assert_rows(score(am, stack["feats"]), stack["want"], "read")
    finally:
        am.close()
    am, got_stats = pk.AcousticModel.load_stats(conf)
    try:
        assert got_stats.tobytes() == stats.tobytes() and am.time_context() == (TC.LH, TC.RH)
        assert_rows(score(am.set_softmax("reference"), stack["feats"]), stack["want"], "load_stats")
    finally:
        am.close()


def test_recognizer_on_the_model_file(stack, model_file):
    """Recognizer.process_features on the model file equals FeatureScorer + Decoder on the model built in memory."""
    tmp, conf, stats = model_file
    feats = [f for f in stack["feats"] if f.shape[0]]
    spec = FA.S(bins=TC.FEAT_DIM)
    am = stack["am"]
    fst = pk.Fst(str(tmp / "general.fst"))
    fs = pk.FeatureScorer(am, len(feats), sum(f.shape[0] for f in feats))
    dec = pk.Decoder(fst, am, len(feats))
    rec = pk.Recognizer(conf, max_utts=len(feats), max_total_samples=160 * sum(f.shape[0] for f in feats), frontend=spec)
    try:
        rec.am.set_softmax("reference")
        assert rec.am.time_context() == (TC.LH, TC.RH)
        score(am, feats, fs)
        dec.decode_batch(fs)
        want = [dec.result(u) for u in range(len(feats))]
        got = rec.process_features(feats, "normalized")
        for u in range(len(feats)):
            assert got[u].words == want[u][0] and np.float32(got[u].weight).tobytes() == np.float32(want[u][1]).tobytes() and got[u].ok == want[u][2], u
            assert rec.batch.fetch(u).log_prob().tobytes() == fs.fetch(u).log_prob().tobytes(), u
        assert any(w[2] == 1 for w in want)
    finally:
        rec.close()
        dec.close()
        fs.close()
        fst.close()


def test_refusals_by_name(stack, model_file, capsys):
    tmp, conf, stats = model_file
    am = stack["am"]
    spec = FA.S(bins=TC.FEAT_DIM)
    assert pk.ONLINE_TIME_SPLICE_REFUSAL == ONLINE_REFUSAL          # (what recognize.py looks for is what the library says)
    with pytest.raises(pk.PkError, match="propagate takes spliced rows without utterance edges; a model with time-splice layers needs a scorer"):
        am.propagate(np.zeros((5, am.input_dim()), F32))
    with pytest.raises(pk.PkError, match=ONLINE_REFUSAL):
        pk.OnlineFeatureScorer(am, 2, 64)
    with pytest.raises(pk.PkError, match=ONLINE_REFUSAL):
        pk.OnlineFeatureScorer(am, 2, 64, global_stats=stats)
    with pytest.raises(pk.PkError, match=ONLINE_REFUSAL):
        pk.OnlineScorer(am, stats, 2, 1600, frontend=spec)
    with pytest.raises(pk.PkError, match=ONLINE_REFUSAL):
        pk.OnlineRecognizer(conf, max_streams=2, max_step_samples=1600, frontend=spec)
    # the command line: --online with such a model is a usage error that says why
    from pocketkaldi_amd import recognize
    wav = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "en-us-hello.wav")
    capsys.readouterr()
    rc = recognize.main([conf, wav, "--frontend", "num_mel_bins=%d" % TC.FEAT_DIM, "--online"])
    out = capsys.readouterr()
    assert rc == 1 and ONLINE_REFUSAL in out.out and "Usage:" in out.out, out.out + out.err
    capsys.readouterr()
    assert recognize.main([conf, wav, "--frontend", "num_mel_bins=%d" % TC.FEAT_DIM]) == 0       # and without --online it recognizes
    capsys.readouterr()


# ---------------------------------------------------------------- i. the default tail

def test_stack_stable_tail_within_the_bound(stack):
    """The default tail (log-softmax in its stable form) on the same stack: the project's bound 1e-4 max(|ref|, 1)."""
    am = pk.AcousticModel(stack["layers"], stack["prior"], TC.LEFT, TC.RIGHT)
    try:
        for a, b in zip(score(am, stack["feats"]), stack["want"]):
            assert a.shape[0] == b.shape[0] and (b.shape[0] == 0 or a.shape == b.shape)
            assert b.shape[0] == 0 or np.all(np.abs(a - b) <= 1e-4 * np.maximum(np.abs(b), 1.0))
    finally:
        am.close()


def test_one_pass_keeps_the_fused_tail(monkeypatch):
    """A walk of one pass keeps the tail fused into the last GEMM (stable softmax, 1 000 pdfs = 4 chunks of 256 columns,
    49 row tiles x 8 column tiles >= 384): the pass runs Rh rows more than it owns, and the fused tail must stop at the
    owned ones.  Its rows are those of the same utterance in passes of 2 048 rows, which take the separate tail launch over
    the owned sub-range, and they stay within the project's bound of loglik_time."""
    rng = np.random.default_rng(0xF05E)
    layers = [LC._linear(rng, 24, 10), ("splice", [-1, 2]), LC._linear(rng, 20, 12), ("tanh",), ("splice", [-3, 3]), LC._linear(rng, 24, 1000), ("softmax",)]
    prior = rng.uniform(0.5, 1.5, 1000).astype(F32)
    prior /= prior.sum()
    x = TC.feats_of([6200], seed=11)[0]
    want = TC.loglik_time(layers, x, prior, 2, 1, TC.SCALE)
    am = pk.AcousticModel(layers, prior, 2, 1)
    try:
        one = score(am, [x])[0]
        monkeypatch.setenv("PK_MI355_CHUNK", "2048")
        cut = score(am, [x])[0]
        assert one.shape == want.shape and one.tobytes() == cut.tobytes()
        assert np.all(np.abs(one - want) <= 1e-4 * np.maximum(np.abs(want), 1.0))
    finally:
        am.close()


# ---------------------------------------------------------------- j. the C++ mirror

def weight(k):
    k = (np.asarray(k, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return ((k >> np.uint64(16)).astype(F32) / F32(65536.0) - F32(0.5)) * F32(0.05)


def example_linear(l, n_in, n_out):
    return ("linear", (F32(8.0) * weight(l * 1000003 + np.arange(n_out * n_in))).reshape(n_out, n_in), weight(500009 + l * 1000003 + np.arange(n_out)))


def test_time_splice_example_equals_python():
    from test_cpp_ark_features import fnv
    from test_cpp_stream import build
    got = subprocess.run([build("time_splice_example")], capture_output=True, text=True)
    assert got.returncode == 0 and "time_splice_example ok" in got.stdout, got.stdout + got.stderr
    D, L, R, N, T = 6, 2, 1, 7, 37
    layers = [example_linear(0, D * (L + R + 1), 40), ("pnorm", 10), ("normalize",), ("splice", [-1, 2]), example_linear(1, 20, 34), ("relu",),
              ("splice", [-3, 3]), example_linear(2, 68, 12), ("tanh",), example_linear(3, 12, N), ("softmax",)]
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
    assert lines[0] == "frames %d pdfs %d context 4 5" % (T, N)
    for i, t in enumerate((0, 17, 36)):
        assert lines[1 + i] == "row %d:" % t + "".join(" %.9g" % v for v in rows[t])
    assert lines[4] == "loglik " + fnv(rows.tobytes())
    want = TC.loglik_time(layers, feats, prior, L, R, 1.0)
    assert np.all(np.abs(rows - want) <= 1e-4 * np.maximum(np.abs(want), 1.0))
