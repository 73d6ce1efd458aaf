"""The time-splice layer, kind 9, on the GPU beyond the corner tests/test_gpu_time_splice.py covers:
  1. the kind at its limits -- |o| = 32, 16 offsets, n D = 512 and 528 (the GEMM behind the splice runs two k-chunks), four
     splices with the context (64, 64)
  2. a multisplice shape, shrunk (context (11, 8): the halo rounding does something) through every way to the rows
  3. the pass boundary on every kind of row and column between two utterances; the last frame of the batch on the last and
     on the first row of a tile
  4. the fused 40-bin CMVN writer and the wave path in front of such a model, and one case per other producer of the
     layout's input
all bit for bit in softmax mode "reference" against tests/time_splice_cases.py's loglik_time (the oracle's Fbank and cmvn in
front of it where waves or raw rows go in), except the one default-tail case.  tests/test_time_splice_host.py checks on the
CPU that these cases can tell the right edge rule from the wrong one."""
import ctypes

import numpy as np
import pytest

import pocketkaldi_amd as pk

import refmodel_files as RF
import time_splice_cases as TC
from test_gpu_time_splice import assert_rows, graph_file, score

pytestmark = pytest.mark.gpu

F32 = np.float32
MS = (TC.MS_LEFT, TC.MS_RIGHT, TC.MS_LH, TC.MS_RH)


def want_rows(layers, prior, left, right, feats):
    return [TC.loglik_time(layers, f, prior, left, right, TC.SCALE) for f in feats]


def poisoned(rows):
    """The same shapes filled with NaN and 3e38, both in every utterance."""
    out = []
    for u, f in enumerate(rows):
        p = np.full_like(f, np.nan if u % 2 == 0 else 3e38)
        p[::2, ::3] = 3e38 if u % 2 == 0 else np.nan
        out.append(p)
    return out


def scorer_for(am, feats, **kw):
    return pk.FeatureScorer(am, len(feats), max(sum(f.shape[0] for f in feats), 1), **kw)


def fetch_rows(bs):
    return [bs.fetch(u).log_prob() for u in range(bs.num_utts())]


# ---------------------------------------------------------------- 1. the kind at its limits

@pytest.mark.parametrize("case", TC.LIMIT_CASES, ids=[c[0] for c in TC.LIMIT_CASES])
def test_the_kind_alone_at_its_limits(case):
    """The "alone" form (identity Linear of width D, the splice, a seeded Linear n D -> 5) through pk.Decodable on
    layer_cases.designed inputs: offsets -32 and 32; sixteen offsets of two residues mod 4; n D = 528 and n D = 512."""
    _, D, offsets = case
    layers = TC.alone_layers(D, offsets, 1)
    prior = np.ones(5, F32)
    am = pk.AcousticModel(layers, prior).set_softmax("reference")
    try:
        assert am.time_context() == TC.time_context(layers) == TC.lo_hi(offsets)
        for T in TC.LIMIT_T:
            x = TC.limit_input(D, T)
            want = TC.loglik_time(layers, x, prior, 0, 0, 1.0)
            d = pk.Decodable(am, 1.0, x)
            got = d.log_prob()
            d.destroy()
            assert got.shape == (T, 5)
            bad = np.flatnonzero(~TC.same_rows(got, want))
            assert bad.size == 0, "D = %d, %d offsets, T = %d: rows %s differ" % (D, len(offsets), T, bad[:8])
    finally:
        am.close()


@pytest.mark.parametrize("walk", ["one_pass", "passes"])
def test_four_splices_at_the_largest_context(walk, monkeypatch):
    """Four splices [-16, 16], context (64, 64), the ragged batch [1, 1, 130, 2, 1]: 790 columns, four passes of 256 rows
    under PK_MI355_CHUNK=128 with halos of 64 rows on either side."""
    layers, prior = TC.deep()
    feats = TC.deep_feats()
    want = want_rows(layers, prior, TC.LEFT, TC.RIGHT, feats)
    if walk == "passes":
        monkeypatch.setenv("PK_MI355_CHUNK", "128")
    am = pk.AcousticModel(layers, prior, TC.LEFT, TC.RIGHT).set_softmax("reference")
    try:
        assert am.time_context() == TC.DEEP_CONTEXT
        assert_rows(score(am, feats), want, walk)
    finally:
        am.close()


# ---------------------------------------------------------------- 2. a multisplice shape, shrunk

@pytest.fixture(scope="module")
def ms():
    """The model, its batch and loglik_time's rows: made once, shared, left unchanged."""
    layers, prior = TC.multisplice()
    feats = TC.ms_feats()
    want = want_rows(layers, prior, TC.MS_LEFT, TC.MS_RIGHT, feats)
    am = pk.AcousticModel(layers, prior, TC.MS_LEFT, TC.MS_RIGHT, tid2pdf=np.arange(TC.MS_PDFS, dtype=np.int32)).set_softmax("reference")
    yield {"layers": layers, "prior": prior, "feats": feats, "want": want, "am": am}
    am.close()


def test_multisplice_fetch_fetch_all_gather(ms):
    am, feats, want = ms["am"], ms["feats"], ms["want"]
    assert am.feat_dim() == TC.MS_FEAT_DIM and am.num_pdfs() == TC.MS_PDFS and am.time_context() == (TC.MS_LH, TC.MS_RH)
    fs = scorer_for(am, feats)
    L_ = pk.lib()

    def to_device(arr):
        p = L_.pk_mi355_device_malloc(arr.nbytes)
        assert p and L_.pk_mi355_memcpy(p, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes, 1) == 0
        return p
    try:
        assert_rows(score(am, feats, fs), want, "fetch")
        assert_rows([v.log_prob() for v in fs.fetch_all()], want, "fetch_all")
        for u, w in enumerate(want):
            T = w.shape[0]
            if T == 0:
                continue
            rng = np.random.default_rng([0x6A7, u])
            frames = np.concatenate([[0, T - 1], rng.integers(0, T, 200)]).astype(np.int32)
            tids = rng.integers(1, TC.MS_PDFS, frames.shape[0]).astype(np.int32)
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


def test_multisplice_decode_batch_reads_the_right_rows(ms, tmp_path):
    am, feats = ms["am"], ms["feats"]
    fst = pk.Fst(graph_file(tmp_path))                 # (the graph has 7 pdfs of the model's 11)
    fs = scorer_for(am, feats)
    dec = pk.Decoder(fst, am, len(feats))
    try:
        rows = score(am, feats, fs)
        assert_rows(rows, ms["want"], "rows")
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


def test_multisplice_after_a_larger_poisoned_batch(ms):
    am = ms["am"]
    big = poisoned(TC.ms_feats(TC.MS_POISON_LENGTHS, seed=32))
    fs = scorer_for(am, big)
    try:
        dirty = score(am, big, fs)
        assert all(np.isnan(d).all() for d in dirty)
        assert_rows(score(am, ms["feats"], fs), ms["want"], "after poison")
    finally:
        fs.close()


def test_multisplice_written_and_read_back(ms, tmp_path):
    RF.write_model(tmp_path, [], ms["prior"], TC.MS_LEFT, TC.MS_RIGHT)
    pk.write_nnet(str(tmp_path / "am.nnet"), ms["layers"])
    am = pk.AcousticModel.read(str(tmp_path / "am.nnet"), str(tmp_path / "am.prior"), None, TC.MS_LEFT, TC.MS_RIGHT, TC.MS_PDFS).set_softmax("reference")
    try:
        assert am.time_context() == (TC.MS_LH, TC.MS_RH)
        assert_rows(score(am, ms["feats"]), ms["want"], "read back")
    finally:
        am.close()


def test_multisplice_stable_tail_within_the_bound(ms):
    """The default tail on the same model: the project's bound 1e-4 max(|ref|, 1)."""
    am = pk.AcousticModel(ms["layers"], ms["prior"], TC.MS_LEFT, TC.MS_RIGHT)
    try:
        for a, b in zip(score(am, ms["feats"]), ms["want"]):
            assert a.shape[0] == b.shape[0] and (b.shape[0] == 0 or a.shape == b.shape)
            assert b.shape[0] == 0 or np.all(np.abs(a - b) <= 1e-4 * np.maximum(np.abs(b), 1.0))
    finally:
        am.close()


# ---------------------------------------------------------------- 3. the pass boundary across an utterance edge; the end of the batch

@pytest.fixture(scope="module")
def sweep(ms):
    """[T0, 40, 300] for every T0 of the sweep: the features, loglik_time's rows and the one-pass scorer's."""
    rest = TC.ms_feats(TC.SWEEP_REST, seed=33)
    rest_want = want_rows(ms["layers"], ms["prior"], TC.MS_LEFT, TC.MS_RIGHT, rest)
    out = []
    fs = pk.FeatureScorer(ms["am"], 3, 600)
    for T0 in TC.sweep_lengths(*MS):
        first = TC.sweep_first(T0)
        feats = [first] + rest
        out.append((T0, feats, want_rows(ms["layers"], ms["prior"], TC.MS_LEFT, TC.MS_RIGHT, [first]) + rest_want, score(ms["am"], feats, fs)))
    fs.close()
    return out


def test_sweep_in_one_pass(sweep):
    for T0, _, want, one in sweep:
        assert_rows(one, want, "T0 = %d, one pass" % T0)


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_sweep_of_the_pass_boundary(ms, sweep, lanes, monkeypatch):
    """Passes of 256 rows: row 256 -- the second pass's first own row; its halo starts 12 rows in front, not 11 -- lies in
    turn on utterance 0's last frames, its right virtual frames, the rows of no frame, utterance 1's left virtual frames
    and its first frames (tests/test_time_splice_host.py::test_the_sweep_visits_every_place_at_the_edge)."""
    monkeypatch.setenv("PK_MI355_CHUNK", "128")
    monkeypatch.setenv("PK_MI355_LANES", lanes)
    fs = pk.FeatureScorer(ms["am"], 3, 600)
    try:
        for T0, feats, want, one in sweep:
            got = score(ms["am"], feats, fs)
            assert_rows(got, one, "T0 = %d, lanes = %s, against one pass" % (T0, lanes))
            assert_rows(got, want, "T0 = %d, lanes = %s" % (T0, lanes))
    finally:
        fs.close()


END_BATCHES = TC.end_batches(*MS)


@pytest.mark.parametrize("walk", ["one_pass", "passes"])
@pytest.mark.parametrize("name", sorted(END_BATCHES))
def test_the_end_of_the_batch(ms, name, walk, monkeypatch):
    """The last utterance's last frame on the last row of a 128-row tile (its Rh virtual frames, which the last pass must
    still run, lie in a tile of their own) and on the first: tiles counted from row 0, where a walk of one pass starts,
    and from the last pass's first row.  A fresh scorer each, so the rows behind the end hold nothing of an earlier call."""
    feats = TC.ms_feats(END_BATCHES[name], seed=35)
    want = want_rows(ms["layers"], ms["prior"], TC.MS_LEFT, TC.MS_RIGHT, feats)
    if walk == "passes":
        monkeypatch.setenv("PK_MI355_CHUNK", "128")
    assert_rows(score(ms["am"], feats), want, "%s, %s" % (name, walk))


# ---------------------------------------------------------------- 4. behind the fused CMVN writer and behind audio

@pytest.fixture(scope="module")
def audio():
    layers, prior = TC.audio_model()
    am = pk.AcousticModel(layers, prior, TC.AUDIO_LEFT, TC.AUDIO_RIGHT).set_softmax("reference")
    assert am.time_context() == TC.AUDIO_CONTEXT
    yield {"layers": layers, "prior": prior, "am": am}
    am.close()


def audio_want(audio, front):
    return want_rows(audio["layers"], audio["prior"], TC.AUDIO_LEFT, TC.AUDIO_RIGHT, front)


def assert_cmvn(bs, front, what):
    for u, f in enumerate(front):
        assert bs.fetch_cmvn(u).tobytes() == f.tobytes(), "%s: utterance %d, the normalised features differ" % (what, u)


@pytest.mark.parametrize("before", ["fresh", "after_poison"])
def test_raw_rows_through_the_fused_cmvn_writer(audio, before):
    """Raw [T][40] rows with global statistics: the SLIDING plan, CmvnKernel writes Yt and both pads of left + Lh = 9 and
    right + Rh = 10 columns.  T = 1 and 2 (both pads from the first tile), 63 / 64 / 65 (the last tile ragged, full, one
    frame), 601 and 664 (the window slides at the right edge)."""
    g, raw, front = TC.raw_front()
    want = audio_want(audio, front)
    big = poisoned(TC.raw_rows(TC.RAW_POISON_LENGTHS, 42))
    fs = scorer_for(audio["am"], big, global_stats=g)
    try:
        if before == "after_poison":
            fs.set_features(big, "raw")
            fs.score(TC.SCALE)
            assert all(np.isnan(r).all() for r in fetch_rows(fs))
        fs.set_features(raw, "raw")
        fs.enable_timing(True)
        fs.score(TC.SCALE)
        t = fs.timing()
        assert t["fbank"][1] == 0 and t["cmvn"][1] == 1, t
        assert_cmvn(fs, front, before)
        assert_rows(fetch_rows(fs), want, before)
    finally:
        fs.close()


@pytest.mark.parametrize("samples", ["float", "int16"])
def test_golden_waves_into_a_time_splice_model(audio, samples):
    """Wave in, rows out: the oracle's Fbank and cmvn, then loglik_time."""
    stats, waves, front = TC.golden_waves()
    want = audio_want(audio, front)
    assert all(w.shape[0] > sum(TC.AUDIO_CONTEXT) for w in want)
    bs = pk.BatchScorer(audio["am"], stats, len(waves), sum(w.shape[0] for w in waves))
    try:
        if samples == "float":
            bs.set_waves(waves)
        else:
            assert all(np.array_equal(w, w.astype(np.int16)) for w in waves)
            bs.set_waves_i16([w.astype(np.int16) for w in waves])
        bs.score(TC.SCALE)
        assert_cmvn(bs, front, samples)
        assert_rows(fetch_rows(bs), want, samples)
    finally:
        bs.close()


@pytest.mark.parametrize("name", TC.PRODUCERS)
def test_every_other_producer_in_front_of_a_time_splice_model(name):
    """FeatureLayoutKernel behind a normalisation spec, behind the deltas and behind an LDA transform, and the any-bin
    front-end with the chain CMVN: each hands the layout left + Lh and right + Rh frames to replicate."""
    case = TC.producer_case(name)
    layers, prior = TC.narrow(case["dim"])
    want = want_rows(layers, prior, 2, 1, case["front"])
    am = pk.AcousticModel(layers, prior, 2, 1).set_softmax("reference")
    n, frames = len(case["input"]), sum(f.shape[0] for f in case["front"])
    try:
        assert am.time_context() == TC.NARROW_CONTEXT
        if name == "frontend":
            bs = pk.BatchScorer(am, case["stats"], n, sum(w.shape[0] for w in case["input"]), frontend=case["spec"])
            bs.set_waves_i16(case["input"])
        else:
            if name == "norm":
                bs = pk.FeatureScorer(am, n, frames)
                bs.set_norm(pk.NormSpec("utterance", True, True))
            elif name == "deltas":
                bs = pk.FeatureScorer(am, n, frames, deltas=pk.DeltaSpec(2, 2))
                bs.set_norm(pk.NormSpec("utterance", True, True))
            else:
                bs = pk.FeatureScorer(am, n, frames, transform=pk.TransformSpec(case["matrix"], 3, 3))
                bs.set_norm(pk.NormSpec("none"))
            bs.set_features(case["input"], "raw")
        try:
            bs.score(TC.SCALE)
            assert_cmvn(bs, case["front"], name)
            assert_rows(fetch_rows(bs), want, name)
        finally:
            bs.close()
    finally:
        am.close()
