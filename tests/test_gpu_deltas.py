"""Delta features on the GPU: DeltaKernel between the normalisation and FeatureLayoutKernel in a
batch scorer made with deltas=, against the numpy restatement of the rule (tests/delta_cases.py).
  * Every base dimension, spec and context, ragged batches with frameless utterances first, in the middle and last and
    frame counts around the reach M and the kernel's run of G frames: fetch_cmvn equals the restatement as bits,
    fetch_fbank is the input, the log-likelihoods equal a plain FeatureScorer's on the host result fed as NORMALIZED,
    host and device entry, both softmax modes.
  * Every norm mode in front of the deltas: fetch_cmvn is pk.add_deltas of a plain Db-dim scorer's fetch_cmvn under the
    same spec -- none, utterance with variance, speaker, online CMVN at W = 8, sliding at Db = 40 (where the plain
    scorer runs CmvnKernel's fused path and this one the chain kernel) and at Db = 41; norm_stats are at Db.
  * Audio through a 13-of-23 MFCC and an 80-bin fbank.
  * NaN, +inf at a centre tap, -0.0; poisoned neighbours and reused buffers; an existing-entry batch on the same process
    still gives the bits it gave; f16x3 at feat_dim = 120 within the contract; every failure code."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pocketkaldi_amd as pk
from oracle import oracle as O

import cmvn_any_cases as CA
import delta_cases as DC
import frontend_any_cases as FA
import norm_cases as NC
from test_gpu_cmvn_any import DeviceCopy, fetch_rows, tiny
from test_gpu_parity import assert_loglik_close

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
DIMS = [1, 13, 40, 63, 64, 65, 80]
SPECS = [(1, 1), (2, 2), (3, 1), (2, 5)]
CONTEXTS = [(0, 0), (2, 1), (5, 5)]
G = int(re.search(r"kDeltaFrames\s*=\s*(\d+)", open(os.path.join(REPO, "pocketkaldi_amd", "csrc", "pk_delta_kernel.h")).read()).group(1))


def frame_list(order, window):
    """Frameless first, in the middle and last; T in {1, 2, M, M + 1, 2M + 1, G - 1, G, G + 1, 130}."""
    M = order * window
    ts = sorted({1, 2, M, M + 1, 2 * M + 1, G - 1, G, G + 1, 130})
    half = len(ts) // 2
    return [0] + ts[:half] + [0] + ts[half:] + [0]


_raw = {}


def raw_case(Db, frames):
    """The utterances of a shape: computed once, shared, left unchanged."""
    key = (Db, tuple(frames))
    if key not in _raw:
        _raw[key] = [NC.features(T, Db, 7 + u) if u % 2 else DC.wide(T, Db, 7 + u) for u, T in enumerate(frames)]
    return _raw[key]


def score_code(fs):
    return pk.lib().pk_mi355_batch_score(fs._h, C.c_float(0.1), 1)


def error_text():
    return pk.lib().pk_mi355_last_error().decode()


def code_of(call):
    with pytest.raises(pk.PkCodeError) as e:
        call()
    return e.value.code, str(e.value)


# ---------------------------------------------------------------- every shape

@pytest.mark.parametrize("Db", DIMS)
def test_every_shape_is_the_restatement_and_the_scores_are_the_normalized_ones(Db):
    for k, (order, window) in enumerate(SPECS):
        spec = pk.DeltaSpec(order, window)
        F = spec.dim(Db)
        frames = frame_list(order, window)
        raw = raw_case(Db, frames)
        want = [DC.add_deltas(x, order, window) for x in raw]
        assert all(NC.bits_equal(pk.add_deltas(x, spec), w) for x, w in zip(raw, want))
        dev = DeviceCopy(raw, Db)
        try:
            for c in (k % 3, (k + 1) % 3):
                L, R = CONTEXTS[c]
                what = "Db=%d order=%d window=%d L=%d R=%d" % (Db, order, window, L, R)
                am, _, _ = tiny(F, L, R, softmax=("stable", "reference")[c % 2])
                fs = pk.FeatureScorer(am, len(raw), sum(frames), deltas=spec)
                plain = pk.FeatureScorer(am, len(raw), sum(frames))
                assert (fs.base_dim(), fs.feat_dim(), plain.base_dim()) == (Db, F, F)
                fs.set_norm(pk.NormSpec("none"))
                fs.enable_timing(True)
                plain.set_features(want, "normalized")
                plain.score(0.1)
                rows = fetch_rows(plain)
                for device in (False, True):
                    if device:
                        fs.set_features_device(dev.ptr, frames, "raw")
                    else:
                        fs.set_features(raw, "raw")
                    fs.score(0.1)
                    t = fs.timing()
                    assert t["fbank"][1] == 0 and t["cmvn"][1] == 1, t          # DeltaKernel and the layout share the CMVN slot
                    got = fetch_rows(fs)
                    for u, x in enumerate(raw):
                        assert fs.num_frames(u) == x.shape[0]
                        assert NC.bits_equal(fs.fetch_fbank(u), x), "%s utterance %d: fetch_fbank is not the input" % (what, u)
                        assert NC.bits_equal(fs.fetch_cmvn(u), want[u]), "%s utterance %d (%d frames) device=%d: rows differ" % (what, u, x.shape[0], device)
                        assert NC.bits_equal(got[u], rows[u]) or frames[u] == 0, "%s utterance %d device=%d: scores differ from NORMALIZED" % (what, u, device)
                fs.set_features(want, "normalized")                             # NORMALIZED passes the norm and the deltas by
                fs.score(0.1)
                for u, r in enumerate(fetch_rows(fs)):
                    assert NC.bits_equal(r, rows[u]) or frames[u] == 0, "%s utterance %d: NORMALIZED on the deltas scorer" % (what, u)
                    assert NC.bits_equal(fs.fetch_cmvn(u), want[u])
                for o in (fs, plain, am):
                    o.close()
        finally:
            dev.free()


# ---------------------------------------------------------------- every norm mode in front of the deltas

NORMS = [("none", 13), ("utterance", 13), ("speaker", 65), ("online", 13), ("sliding", 40), ("sliding", 41)]


@pytest.mark.parametrize("mode, Db", NORMS, ids=["%s-%d" % n for n in NORMS])
def test_every_norm_mode_in_front_of_the_deltas(mode, Db):
    order, window, L, R = 2, 2, 2, 1
    spec = pk.DeltaSpec(order, window)
    frames = [0, 5, 130, 0, 1, 33, 650, 0]
    raw = [CA.features(T, Db, 30 + u) for u, T in enumerate(frames)]
    g = CA.stats_for(Db) if mode == "sliding" else None
    rec = [NC.accumulate(x) for x in raw]
    spk = [r + rec[2] for r in rec]
    am_base, _, _ = tiny(Db, L, R)
    am, _, _ = tiny(spec.dim(Db), L, R)
    plain = pk.FeatureScorer(am_base, len(raw), sum(frames), global_stats=g)
    fs = pk.FeatureScorer(am, len(raw), sum(frames), global_stats=g, deltas=spec)
    for o in (plain, fs):
        if mode == "online":
            o.set_norm(pk.OnlineCmvnSpec(8, 600, 0, True))
        elif mode != "sliding":
            o.set_norm(pk.NormSpec(mode, True, mode != "none"))
        if mode == "speaker":
            o.set_speaker_stats(spk)
        o.set_features(raw, "raw")
        o.score(0.1)
    for u, x in enumerate(raw):
        base = plain.fetch_cmvn(u)
        assert base.shape == (frames[u], Db)
        assert NC.bits_equal(fs.fetch_cmvn(u), pk.add_deltas(base, spec)), (mode, Db, u)
        assert NC.bits_equal(fs.fetch_fbank(u), x)
        if mode == "utterance":                                                 # the records are at Db
            assert fs.norm_stats(u).shape == (2, Db + 1) and NC.bits_equal(fs.norm_stats(u), rec[u]), u
    if mode == "none":
        assert NC.bits_equal(plain.fetch_cmvn(2), raw[2])
    if mode == "utterance":
        assert NC.bits_equal(plain.fetch_cmvn(2), NC.normalize(raw[2], "utterance", True, True)[0])
    if mode == "sliding":
        assert NC.bits_equal(plain.fetch_cmvn(6), O.cmvn(g, raw[6]) if Db == 40 else CA.cmvn_any(g, raw[6]))
    for o in (plain, fs, am, am_base):
        o.close()


# ---------------------------------------------------------------- audio

AUDIO = [("mfcc13of23", FA.SPECS[9]), ("fbank80", FA.SPECS[1])]


@pytest.mark.parametrize("name, fe", AUDIO, ids=[a[0] for a in AUDIO])
def test_audio_through_a_front_end(name, fe):
    Db = fe.dim
    spec = pk.DeltaSpec()
    am_base, _, _ = tiny(Db, 2, 1)
    am, _, _ = tiny(spec.dim(Db), 2, 1)
    g = np.concatenate([np.full(Db, 10.0 * 2500.0), [2500.0]]).astype(np.float32)
    waves = [FA.wave_i16(n, 50 + u).astype(np.float32) for u, n in enumerate((399, 1237, 0, 4321, 159, 2000))]
    cap = sum(w.size for w in waves) + 1
    plain = pk.BatchScorer(am_base, g, len(waves), cap, frontend=fe)
    bs = pk.BatchScorer(am, g, len(waves), cap, frontend=fe, deltas=spec)
    assert (bs.base_dim(), bs.feat_dim()) == (Db, 3 * Db)
    front = pk.Frontend(fe)
    for norm in (None, pk.NormSpec("utterance", True, True)):
        for o in (plain, bs):
            if norm is not None:
                o.set_norm(norm)
            o.set_waves(waves)
            o.score(0.1)
        for u, w in enumerate(waves):
            rows = bs.fetch_fbank(u)
            assert rows.shape == (pk.num_frames(w.size), Db) and NC.bits_equal(rows, front.compute(w).reshape(rows.shape)), (name, u)
            assert NC.bits_equal(bs.fetch_cmvn(u), pk.add_deltas(plain.fetch_cmvn(u), spec)), (name, norm, u)
            if norm is not None:
                assert NC.bits_equal(bs.norm_stats(u), NC.accumulate(rows)), (name, u)
    # the same rows handed over as raw features give the audio's bits
    rows = [bs.fetch_fbank(u) for u in range(len(waves))]
    ll = fetch_rows(bs)
    bs.set_features(rows, "raw")
    bs.score(0.1)
    assert all(NC.bits_equal(a, b) or r.shape[0] == 0 for a, b, r in zip(fetch_rows(bs), ll, rows))
    for o in (plain, bs, am, am_base):
        o.close()


# ---------------------------------------------------------------- edge values, isolation, reuse

def test_edge_values_stay_in_their_column_and_utterance():
    Db, order, window = 65, 2, 2
    spec = pk.DeltaSpec(order, window)
    am, _, _ = tiny(spec.dim(Db), 2, 1)
    x = NC.features(200, Db, 90)
    x[100, 5], x[150, 64], x[40, 7] = np.nan, np.inf, -0.0
    clean = NC.features(130, Db, 91)
    raw = [clean, x, NC.features(1, Db, 92), clean]
    fs = pk.FeatureScorer(am, 4, 461, deltas=spec)
    fs.set_norm(pk.NormSpec("none"))
    fs.set_features(raw, "raw")
    fs.score(0.1)
    want = [DC.add_deltas(r, order, window) for r in raw]
    for u in range(4):
        assert DC.same_but_nan(fs.fetch_cmvn(u), want[u]), u
    got = fs.fetch_cmvn(1)
    assert got[40, 7].tobytes() == np.float32(0.0).tobytes()                  # -0.0 leaves block 0 as +0.0
    assert got[150, 64] == np.inf and not np.isnan(got[150, Db + 64])         # the zero centre tap of block 1 is skipped
    for i in range(order + 1):                                                  # the NaN: its column, within M_i frames
        M = i * window
        nan = np.isnan(got[:, i * Db:(i + 1) * Db])
        assert nan[100 - M:100 + M + 1, 5].any() and not nan[:100 - M, 5].any() and not nan[100 + M + 1:, 5].any()
        nan[:, 5] = False
        nan[:, 64] = False
        assert not nan.any()
    assert NC.bits_equal(fs.fetch_cmvn(0), fs.fetch_cmvn(3)) and NC.bits_equal(fs.fetch(0).log_prob(), fs.fetch(3).log_prob())
    assert np.isfinite(fs.fetch(0).log_prob()).all() and np.isfinite(fs.fetch(2).log_prob()).all()
    fs.close()
    am.close()


def test_poisoned_neighbours_and_reuse_change_no_bit():
    Db, L, R = 41, 2, 1
    spec = pk.DeltaSpec(2, 2)
    am, _, _ = tiny(spec.dim(Db), L, R)
    sets = {"large": [NC.features(T, Db, 60 + u) for u, T in enumerate((700, 0, 64, 1))],
            "small": [NC.features(T, Db, 70 + u) for u, T in enumerate((5, 130))]}
    cap = 765
    norms = [pk.NormSpec("none"), pk.NormSpec("utterance", True, True)]

    def run(fs, which, norm):
        fs.set_norm(norm)
        fs.set_features(sets[which], "raw")
        fs.score(0.1)
        return [fs.fetch_cmvn(u) for u in range(len(sets[which]))], fetch_rows(fs)

    def fresh(which, norm):
        fs = pk.FeatureScorer(am, 4, cap, deltas=spec)
        out = run(fs, which, norm)
        fs.close()
        return out

    want = {(which, i): fresh(which, n) for which in sets for i, n in enumerate(norms)}
    for (which, i), (cm, _) in want.items():                                    # (and the fresh results are the restatement)
        mode = ("none", "utterance")[i]
        assert all(NC.bits_equal(c, DC.add_deltas(NC.normalize(x, mode, True, True)[0], 2, 2)) for c, x in zip(cm, sets[which]))
    one = pk.FeatureScorer(am, 4, cap, deltas=spec)
    for which in ("large", "small", "large"):
        for i, n in enumerate(norms):
            cm, rows = run(one, which, n)
            assert all(NC.bits_equal(a, b) for a, b in zip(cm, want[(which, i)][0])), (which, i)
            assert all(NC.bits_equal(a, b) for a, b in zip(rows, want[(which, i)][1])), (which, i)
            one.set_norm(pk.NormSpec("none"))                                  # poison every buffer in between
            one.set_features([np.full(x.shape, np.nan, np.float32) for x in sets["large"]], "raw")
            one.score(0.1)
            assert all(np.isnan(r).all() for r in fetch_rows(one))
    one.close()
    # NaN and 1e30 utterances between healthy ones
    feats = sets["large"]
    mixed = [feats[0], np.full((650, Db), np.nan, np.float32), feats[2], np.full((3, Db), 1e30, np.float32), feats[3]]
    wide = pk.FeatureScorer(am, 5, cap + 653, deltas=spec)
    for i, n in enumerate(norms):
        wide.set_norm(n)
        wide.set_features(mixed, "raw")
        wide.score(0.1)
        cm, rows = want[("large", i)]
        for at, u in ((0, 0), (2, 2), (4, 3)):
            assert NC.bits_equal(wide.fetch_cmvn(at), cm[u]) and NC.bits_equal(wide.fetch(at).log_prob(), rows[u]), (i, at)
        assert np.isnan(wide.fetch(1).log_prob()).all()
    wide.close()
    am.close()


def test_an_existing_entry_batch_still_gives_its_bits():
    D = 39
    am, _, _ = tiny(D, 2, 1)
    raw = [NC.features(T, D, 20 + u) for u, T in enumerate((9, 0, 70))]
    norm = pk.NormSpec("utterance", True, True)

    def plain_run():
        fs = pk.FeatureScorer(am, 3, 100)
        fs.enable_timing(True)
        fs.set_norm(norm)
        fs.set_features(raw, "raw")
        fs.score(0.1)
        out = ([fs.fetch_cmvn(u) for u in range(3)], fetch_rows(fs), fs.timing(), fs.base_dim())
        fs.close()
        return out

    before = plain_run()
    fs = pk.FeatureScorer(am, 3, 100, deltas=pk.DeltaSpec(2, 2))               # the same 39-dim model as 13 + deltas
    fs.set_norm(norm)
    base = [x[:, :13].copy() for x in raw]
    fs.set_features(base, "raw")
    fs.score(0.1)
    assert NC.bits_equal(fs.fetch_cmvn(2), pk.add_deltas(NC.normalize(base[2], "utterance", True, True)[0], pk.DeltaSpec(2, 2)))
    after = plain_run()
    fs.close()
    assert before[3] == after[3] == D
    assert all(NC.bits_equal(a, b) for a, b in zip(before[0] + before[1], after[0] + after[1]))
    assert all(NC.bits_equal(c, NC.normalize(x, "utterance", True, True)[0]) for c, x in zip(after[0], raw))
    assert [v[1] for v in before[2].values()] == [v[1] for v in after[2].values()]          # launch for launch
    am.close()


# ---------------------------------------------------------------- f16x3

def test_f16x3_at_120_within_the_contract_of_the_oracle():
    """Measured on an MI355X: max |err| / max(|ref|, 1) = 3.725e-07 against the contract's 1e-4 (the printed
    DELTA_F16X3_MAX_ERR line; DESIGN.md section 21 records it)."""
    Db, L, R = 40, 2, 1
    spec = pk.DeltaSpec(2, 2)
    am, layers, prior = tiny(spec.dim(Db), L, R, precision="f16x3")
    raw = [NC.features(T, Db, 80 + u) for u, T in enumerate((701, 0, 130, 5))]
    fs = pk.FeatureScorer(am, len(raw), sum(x.shape[0] for x in raw), deltas=spec)
    fs.set_norm(pk.NormSpec("utterance", True, True))
    fs.set_features(raw, "raw")
    fs.calibrate()
    fs.score(0.1)
    nn = O.Nnet(layers)
    worst = 0.0
    for u, x in enumerate(raw):
        got = fs.fetch(u).log_prob()
        if x.shape[0] == 0:
            assert got.shape[0] == 0
            continue
        want = DC.add_deltas(NC.normalize(x, "utterance", True, True)[0], 2, 2)
        assert NC.bits_equal(fs.fetch_cmvn(u), want), u                          # f32, in front of the split
        ref = nn.am_compute(want, prior, L, R, 0.1)
        worst = max(worst, float((np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)).max()))
        assert_loglik_close(got, ref)
    print("DELTA_F16X3_MAX_ERR %.3e (contract 1e-4)" % worst)
    fs.close()
    am.close()


# ---------------------------------------------------------------- failure codes

def test_failure_codes():
    Db = 13
    spec = pk.DeltaSpec(2, 2)
    am, _, _ = tiny(39, 2, 1)
    g = CA.stats_for(Db)
    fe = FA.SPECS[9]
    assert fe.dim == Db
    # the creation entry, before any device call
    for bad, word in ((pk.DeltaSpec(0, 2), "order"), (pk.DeltaSpec(4, 2), "order"), (pk.DeltaSpec(2, 0), "window"), (pk.DeltaSpec(2, 9), "window")):
        code, text = code_of(lambda: pk.FeatureScorer(am, 2, 100, deltas=bad))
        assert code == E_INVALID and text.startswith("deltas spec:") and word in text, text
    code, text = code_of(lambda: pk.FeatureScorer(am, 2, 100, deltas=pk.DeltaSpec(1, 2)))       # 39 / 2
    assert code == E_INVALID and "39" in text and "2 blocks" in text, text
    code, text = code_of(lambda: pk.BatchScorer(am, g, 2, 16000, frontend=FA.SPECS[1], deltas=spec))
    assert code == E_INVALID and "80" in text and "13" in text and "39" in text, text
    code, text = code_of(lambda: pk.BatchScorer(am, CA.stats_for(39), 2, 16000, frontend=fe, deltas=spec))
    assert code == E_INVALID and "40 entries" in text and "14" in text, text
    code, text = code_of(lambda: pk.FeatureScorer(am, 2, 100, global_stats=CA.stats_for(39), deltas=spec))
    assert code == E_INVALID and "40 entries" in text and "14" in text, text
    code, text = code_of(lambda: pk.BatchScorer(am, g, 2, 16000, frontend=pk.FrontendSpec(num_mel_bins=2), deltas=spec))
    assert code == E_INVALID and "num_mel_bins" in text, text
    for utts, cap in ((0, 100), (2, 0)):
        code, text = code_of(lambda: pk.FeatureScorer(am, utts, cap, deltas=spec))
        assert code == E_INVALID and "capacity" in text
    L = pk.lib()
    st = spec.struct()
    assert not L.pk_mi355_deltas_batch_create(am.handle, None, None, None, 0, 2, 100) and "null" in error_text()
    assert not L.pk_mi355_deltas_batch_create(am.handle, C.byref(st), C.byref(fe.struct()), None, 0, 2, 16000) and "null" in error_text()
    half, _, _ = tiny(39, 2, 1, precision="f16x3")
    code, text = code_of(lambda: pk.FeatureScorer(half, 2, 100, deltas=spec))
    assert code == E_INVALID and "multiple of 8" in text and "39" in text
    half.close()
    # the feature entries: RAW at Db, NORMALIZED at feat_dim
    fs = pk.FeatureScorer(am, 3, 100, deltas=spec)
    raw = [NC.features(T, Db, 20 + u) for u, T in enumerate((9, 0, 70))]
    code, text = code_of(lambda: fs.set_features(raw, "raw"))                  # no statistics, the sliding rule
    assert code == E_INVALID and "statistics" in text and "14" in text, text
    fs.set_norm(pk.NormSpec("none"))
    m39 = pk._as_matrix(np.zeros((4, 39), np.float32))
    assert L.pk_mi355_features_set(fs._h, C.byref(m39), 1, 1) == E_INVALID and "39 rows" in error_text() and "13" in error_text()
    m13 = pk._as_matrix(np.zeros((4, 13), np.float32))
    assert L.pk_mi355_features_set(fs._h, C.byref(m13), 1, 0) == E_INVALID and "13 rows" in error_text() and "39" in error_text()
    assert code_of(lambda: fs.set_features([np.zeros((4, 39), np.float32)], "raw"))[0] == E_INVALID      # refused in Python, by shape
    assert code_of(lambda: fs.set_features([np.zeros((101, 13), np.float32)], "raw"))[0] == E_INVALID    # capacity
    fs.set_features(raw, "raw")
    assert code_of(lambda: fs.fetch_cmvn(0))[0] == E_STATE                      # not scored
    fs.score(0.1)
    assert code_of(lambda: fs.norm_stats(0))[0] == E_STATE                      # mode none computes none
    fs.set_norm(pk.NormSpec())                                                  # back to sliding with raw rows set: nothing to slide with
    assert score_code(fs) == E_STATE and "statistics" in error_text()
    # speaker records and the online global record are at Db
    fs.set_norm(pk.NormSpec("speaker", True, True))
    assert code_of(lambda: fs.set_speaker_stats([np.ones((2, 40))] * 3))[0] == E_INVALID
    fs.set_speaker_stats([NC.accumulate(raw[0])] * 3)
    fs.score(0.1)
    assert NC.bits_equal(fs.fetch_cmvn(2), pk.add_deltas(NC.normalize(raw[2], "speaker", True, True, stats=NC.accumulate(raw[0]))[0], spec))
    assert code_of(lambda: fs.set_norm(pk.OnlineCmvnSpec(8, 600, 200, False), np.ones((2, 40))))[0] == E_INVALID
    fs.set_norm(pk.OnlineCmvnSpec(8, 600, 200, False), NC.accumulate(raw[2]))
    fs.score(0.1)
    # every utterance frameless: nothing launched
    fs.set_norm(pk.NormSpec("utterance"))
    fs.set_features([raw[1], raw[1]], "raw")
    fs.score(0.1)
    assert NC.bits_equal(fs.norm_stats(1), np.zeros((2, Db + 1))) and fs.fetch_cmvn(1).shape == (0, 39)
    # a features-only deltas batch takes no audio
    assert code_of(lambda: fs.set_waves([np.zeros(1600, np.float32)], rates=[16000]))[0] == E_STATE
    fs.close()
    am.close()
