"""The normalisation spec on the GPU: NormKernel in front of FeatureLayoutKernel in every kind of
batch scorer, against the numpy restatement of the rule (tests/norm_cases.py).
  * Every mode and switch pair at every dimension and context, ragged batches with frameless utterances first, in the
    middle and last: fetch_cmvn equals the restatement as bits, norm_stats as doubles; the log-likelihoods equal the same
    scorer's NORMALIZED ones on the restatement's output, host and device entry, both softmax modes.
  * Speaker mode on an utterance call's own records is that call bit for bit; on the summed records of two utterances it
    is the restatement on the sum; `none` is NORMALIZED on the same input; set_norm(sliding) is an untouched scorer.
  * Audio: the 40-dim scorer, an 80-bin front-end, a 13-of-23 MFCC.
  * NaN, +inf and -0.0 stay in their column and utterance; one frame meets the variance floor; poisoned neighbours and
    reuse change no bit; speaker statistics are consumed once; f16x3 at D = 80 at 1e-4 max(|ref|, 1).
  * Failure codes, before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import pocketkaldi_amd as pk
from oracle import oracle as O

import frontend_any_cases as FA
import norm_cases as NC
from test_gpu_cmvn_any import DeviceCopy, fetch_rows, tiny
from test_gpu_parity import assert_loglik_close

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
DIMS = [1, 39, 40, 41, 64, 65, 80, 130]
CONTEXTS = [(0, 0), (2, 1), (5, 5)]
FRAMES = (0, 1, 2, 7, 8, 9, 0, 63, 64, 65, 601, 1307, 0)        # frameless first, in the middle and last
BIG = 11                                                        # the utterance every speaker record below is summed with
COMBOS = [("none", True, False)] + [(m, a, b) for m in ("utterance", "speaker") for a, b in NC.SWITCHES]

_cases = {}


def case(D):
    """(raw utterances, their records, the speaker records: each utterance's summed with the longest one's) at dimension D:
    computed once, shared, left unchanged."""
    if D not in _cases:
        raw = [NC.features(T, D, 7 + u) for u, T in enumerate(FRAMES)]
        rec = [NC.accumulate(x) for x in raw]
        _cases[D] = (raw, rec, [r + rec[BIG] for r in rec])
    return _cases[D]


def wanted(raw, spk, mode, means, variances):
    return [NC.normalize(x, mode, means, variances, stats=spk[u])[0] for u, x in enumerate(raw)]


def score_code(fs):
    return pk.lib().pk_mi355_batch_score(fs._h, C.c_float(0.1), 1)


def error_text():
    return pk.lib().pk_mi355_last_error().decode()


def same_but_nan(got, want):
    """Equal NaN pattern, equal bits everywhere else (a NaN's payload is the arithmetic's own)."""
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    ok = ~np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got.view(u)[ok], want.view(u)[ok])


# ---------------------------------------------------------------- every mode, dimension and context

@pytest.mark.parametrize("D", DIMS)
def test_every_mode_is_the_restatement_and_the_pads_hold_through_the_scores(D):
    raw, rec, spk = case(D)
    frames = [x.shape[0] for x in raw]
    dev = DeviceCopy(raw, D)
    try:
        for k, (L, R) in enumerate(CONTEXTS):
            am, _, _ = tiny(D, L, R, softmax=("stable", "reference")[k % 2])
            fs = pk.FeatureScorer(am, len(raw), sum(frames))                  # no statistics: RAW is the norm spec's alone
            fs.enable_timing(True)
            for mode, means, variances in COMBOS:
                what = "D=%d L=%d R=%d %s means=%d vars=%d" % (D, L, R, mode, means, variances)
                want = wanted(raw, spk, mode, means, variances)
                fs.set_norm(pk.NormSpec(mode, means, variances))
                for device in (False, True):
                    if mode == "speaker":
                        fs.set_speaker_stats(spk)
                    if device:
                        fs.set_features_device(dev.ptr, frames, "raw")
                    else:
                        fs.set_features(raw, "raw")
                    fs.score(0.1)
                    t = fs.timing()
                    assert t["fbank"][1] == 0 and t["cmvn"][1] == 1, t        # NormKernel and the layout share the CMVN slot
                    got = fetch_rows(fs)
                    for u, x in enumerate(raw):
                        assert fs.num_frames(u) == x.shape[0]
                        assert NC.bits_equal(fs.fetch_fbank(u), x), "%s utterance %d: fetch_fbank is not the input" % (what, u)
                        assert NC.bits_equal(fs.fetch_cmvn(u), want[u]), "%s utterance %d (%d frames) device=%d: rows differ" % (what, u, x.shape[0], device)
                        if mode == "utterance":
                            assert NC.bits_equal(fs.norm_stats(u), rec[u]), "%s utterance %d: statistics differ" % (what, u)
                    if not device:
                        rows = got
                        assert all(r.shape[0] == f for r, f in zip(rows, frames))
                    else:
                        assert all(NC.bits_equal(a, b) for a, b in zip(got, rows)), "%s: device entry, rows differ" % what
                fs.set_features(want, "normalized")                           # the same scorer on the restatement's output
                fs.score(0.1)
                for u, r in enumerate(fetch_rows(fs)):
                    assert NC.bits_equal(r, rows[u]) or frames[u] == 0, "%s utterance %d: RAW rows differ from NORMALIZED rows" % (what, u)
            fs.close()
            am.close()
    finally:
        dev.free()


def test_speaker_mode_on_an_utterance_calls_records_is_that_call():
    D = 65
    raw = [x for x in case(D)[0] if x.shape[0] > 0]
    am, _, _ = tiny(D, 2, 1)
    fs = pk.FeatureScorer(am, len(raw), sum(x.shape[0] for x in raw))
    for means, variances in NC.SWITCHES:
        fs.set_norm(pk.NormSpec("utterance", means, variances))
        fs.set_features(raw, "raw")
        fs.score(0.1)
        own = [fs.norm_stats(u) for u in range(len(raw))]
        cm, rows = [fs.fetch_cmvn(u) for u in range(len(raw))], fetch_rows(fs)
        fs.set_norm(pk.NormSpec("speaker", means, variances))
        fs.set_speaker_stats(own)
        fs.set_features(raw, "raw")
        fs.score(0.1)
        for u in range(len(raw)):
            assert NC.bits_equal(fs.fetch_cmvn(u), cm[u]) and NC.bits_equal(fs.fetch(u).log_prob(), rows[u]), (means, variances, u)
    fs.close()
    am.close()


# ---------------------------------------------------------------- the default is the parent's path

def test_set_norm_sliding_is_an_untouched_scorer():
    import cmvn_any_cases as CA
    # from features, at a dimension of the chain kernel and at 40
    for D in (41, 40):
        am, _, _ = tiny(D, 2, 1)
        g = CA.stats_for(D)
        raw = [CA.features(T, D, 30 + u) for u, T in enumerate((0, 650, 3))]
        plain, back = (pk.FeatureScorer(am, 3, 653, global_stats=g) for _ in range(2))
        back.set_norm(pk.NormSpec("utterance", True, True))
        back.set_features(raw, "raw")
        back.score(0.1)
        back.set_norm(pk.NormSpec())
        for fs in (plain, back):
            fs.enable_timing(True)
            fs.set_features(raw, "raw")
            fs.score(0.1)
        assert plain.timing()["cmvn"][1] == back.timing()["cmvn"][1] == 1
        for u in range(3):
            assert NC.bits_equal(back.fetch_cmvn(u), plain.fetch_cmvn(u)) and NC.bits_equal(back.fetch(u).log_prob(), plain.fetch(u).log_prob()), (D, u)
        assert NC.bits_equal(plain.fetch_cmvn(1), O.cmvn(g, raw[1]) if D == 40 else CA.cmvn_any(g, raw[1]))
        code = pk.lib().pk_mi355_norm_fetch_stats(back._h, 1, np.zeros(2 * (D + 1)).ctypes.data_as(C.POINTER(C.c_double)))
        assert code == E_STATE
        plain.close()
        back.close()
        am.close()
    # from audio
    am, _, _ = tiny(40, 2, 1)
    g = CA.stats_for(40)
    waves = [FA.wave_i16(n, 40 + u).astype(np.float32) for u, n in enumerate((399, 4321, 1237))]
    plain, back = (pk.BatchScorer(am, g, 3, 6000) for _ in range(2))
    back.set_norm(pk.NormSpec("none"))
    back.set_waves(waves)
    back.score(0.1)
    back.set_norm(pk.NormSpec("sliding", True, False))
    for bs in (plain, back):
        bs.set_waves(waves)
        bs.score(0.1)
    for u in range(3):
        assert NC.bits_equal(back.fetch_cmvn(u), plain.fetch_cmvn(u)) and NC.bits_equal(back.fetch(u).log_prob(), plain.fetch(u).log_prob()), u
    plain.close()
    back.close()
    am.close()


# ---------------------------------------------------------------- audio

AUDIO = [("batch40", None), ("fbank80", FA.SPECS[1]), ("mfcc13of23", FA.SPECS[9])]


@pytest.mark.parametrize("name, spec", AUDIO, ids=[a[0] for a in AUDIO])
def test_audio_through_every_mode(name, spec):
    D = 40 if spec is None else spec.dim
    am, _, _ = tiny(D, 2, 1)
    g = np.concatenate([np.full(D, 10.0 * 2500.0), [2500.0]]).astype(np.float32)
    waves = [FA.wave_i16(n, 50 + u).astype(np.float32) for u, n in enumerate((399, 1237, 0, 4321, 159, 2000))]
    bs = pk.BatchScorer(am, g, len(waves), sum(w.size for w in waves) + 1, frontend=spec)
    bs.set_waves(waves)
    bs.score(0.1)
    rows = [bs.fetch_fbank(u) for u in range(len(waves))]                     # the front-end's rows, pinned by its own tests
    assert [r.shape[0] for r in rows] == [pk.num_frames(w.size) for w in waves]
    if spec is not None:
        fe = pk.Frontend(spec)
        assert all(NC.bits_equal(r, fe.compute(w).reshape(r.shape)) for r, w in zip(rows, waves))
    rec = [NC.accumulate(r) for r in rows]
    total = sum(rec)
    spk = [r + total for r in rec]
    for mode, means, variances in COMBOS:
        want = wanted(rows, spk, mode, means, variances)
        bs.set_norm(pk.NormSpec(mode, means, variances))
        if mode == "speaker":
            bs.set_speaker_stats(spk)
        bs.set_waves(waves)
        bs.score(0.1)
        ll = fetch_rows(bs)
        for u in range(len(waves)):
            assert NC.bits_equal(bs.fetch_cmvn(u), want[u]), (name, mode, means, variances, u)
            if mode == "utterance":
                assert NC.bits_equal(bs.norm_stats(u), rec[u]), (name, u)
        bs.set_features(want, "normalized")
        bs.score(0.1)
        for u, r in enumerate(fetch_rows(bs)):
            assert NC.bits_equal(r, ll[u]) or rows[u].shape[0] == 0, (name, mode, means, variances, u)
    bs.close()
    am.close()


# ---------------------------------------------------------------- edge values, isolation, reuse

def test_edge_values_stay_in_their_column_and_utterance():
    D = 65
    am, _, _ = tiny(D, 2, 1)
    x = NC.features(700, D, 90)
    x[300, 5], x[350, 64], x[100, 7] = np.nan, np.inf, -0.0
    clean, one = NC.features(130, D, 91), NC.features(1, D, 92)
    raw = [clean, x, one, clean]
    touched = np.zeros(D, bool)
    touched[[5, 64]] = True
    fs = pk.FeatureScorer(am, 4, 961)
    for means, variances in NC.SWITCHES:
        want = [NC.normalize(r, "utterance", means, variances) for r in raw]
        # (the +inf column: NaN with both switches; means only, its offset is -inf; variance only, its scale is 0)
        assert np.isnan(want[1][0][:, 5]).all() and np.isnan(want[1][0][350, 64]) and np.isfinite(want[1][0][:, ~touched]).all()
        fs.set_norm(pk.NormSpec("utterance", means, variances))
        fs.set_features(raw, "raw")
        fs.score(0.1)
        for u in range(4):
            assert same_but_nan(fs.fetch_cmvn(u), want[u][0]), (means, variances, u)
            assert same_but_nan(fs.norm_stats(u), want[u][1]), (means, variances, u)
        assert NC.bits_equal(fs.fetch_cmvn(0), fs.fetch_cmvn(3)) and NC.bits_equal(fs.fetch(0).log_prob(), fs.fetch(3).log_prob())
        assert np.isfinite(fs.fetch(0).log_prob()).all()
        if means and variances:                                                 # one frame: the variance floor
            offs, scale = NC.finalize(want[2][1], means, variances)
            assert (scale == np.float32(1e10)).all() and NC.bits_equal(fs.fetch_cmvn(2), want[2][0])
    fs.close()
    am.close()


def test_poisoned_neighbours_and_reuse_change_no_bit():
    D, L, R = 41, 2, 1
    am, _, _ = tiny(D, L, R)
    sets = {"large": [NC.features(T, D, 60 + u) for u, T in enumerate((700, 0, 64, 1))], "small": [NC.features(T, D, 70 + u) for u, T in enumerate((5, 130))]}
    cap = 765
    recs = {k: [NC.accumulate(x) + NC.accumulate(v[0]) for x in v] for k, v in sets.items()}
    specs = [pk.NormSpec("utterance", True, True), pk.NormSpec("speaker", True, True), pk.NormSpec("none"), pk.NormSpec("utterance", True, False),
             pk.NormSpec("speaker", False, True)]

    def run(fs, which, spec):
        fs.set_norm(spec)
        if spec.mode == pk.NORM_MODES["speaker"]:
            fs.set_speaker_stats(recs[which])
        fs.set_features(sets[which], "raw")
        fs.score(0.1)
        return [fs.fetch_cmvn(u) for u in range(len(sets[which]))], fetch_rows(fs)

    def fresh(which, spec):
        fs = pk.FeatureScorer(am, 4, cap)
        out = run(fs, which, spec)
        fs.close()
        return out

    want = {(which, i): fresh(which, s) for which in sets for i, s in enumerate(specs)}
    for (which, i), (cm, _) in want.items():                                      # (and the fresh results are the restatement)
        s = specs[i]
        mode = [m for m, v in pk.NORM_MODES.items() if v == s.mode][0]
        assert all(NC.bits_equal(c, NC.normalize(x, mode, s.norm_means, s.norm_vars, stats=r)[0]) for c, x, r in zip(cm, sets[which], recs[which]))
    one = pk.FeatureScorer(am, 4, cap)
    for which in ("large", "small", "large"):
        for i, s in enumerate(specs):                                            # the modes in turn on one object
            cm, rows = run(one, which, s)
            assert all(NC.bits_equal(a, b) for a, b in zip(cm, want[(which, i)][0])), (which, i)
            assert all(NC.bits_equal(a, b) for a, b in zip(rows, want[(which, i)][1])), (which, i)
            one.set_norm(pk.NormSpec("none"))                                    # poison every buffer in between
            one.set_features([np.full(x.shape, np.nan, np.float32) for x in sets["large"]], "raw")
            one.score(0.1)
            assert all(np.isnan(r).all() for r in fetch_rows(one))
    one.close()
    # NaN and 1e30 utterances between healthy ones
    feats = sets["large"]
    mixed = [feats[0], np.full((650, D), np.nan, np.float32), feats[2], np.full((3, D), 1e30, np.float32), feats[3]]
    pairs = ((0, 0), (2, 2), (4, 3))
    wide = pk.FeatureScorer(am, 5, cap + 653)
    for i in (0, 1):
        wide.set_norm(specs[i])
        if i == 1:
            stats = [np.ones((2, D + 1))] * 5
            for at, u in pairs:
                stats[at] = recs["large"][u]
            wide.set_speaker_stats(stats)
        wide.set_features(mixed, "raw")
        wide.score(0.1)
        cm, rows = want[("large", i)]
        for at, u in pairs:
            assert NC.bits_equal(wide.fetch_cmvn(at), cm[u]) and NC.bits_equal(wide.fetch(at).log_prob(), rows[u]), (i, at)
        assert np.isnan(wide.fetch(1).log_prob()).all()
    wide.close()
    am.close()


def test_speaker_statistics_are_consumed_by_one_score():
    D = 39
    raw, rec, spk = case(D)
    raw, spk = raw[7:10], spk[7:10]
    am, _, _ = tiny(D, 2, 1)
    fs = pk.FeatureScorer(am, 3, 200)
    fs.set_norm(pk.NormSpec("speaker", True, True))
    fs.set_speaker_stats(spk)
    fs.set_features(raw, "raw")
    fs.score(0.1)
    first = [fs.fetch_cmvn(u) for u in range(3)]
    assert all(NC.bits_equal(a, NC.normalize(x, "speaker", True, True, stats=s)[0]) for a, x, s in zip(first, raw, spk))
    assert score_code(fs) == E_STATE and "speaker" in error_text()              # consumed
    fs.set_speaker_stats(spk)                                                   # set before the features: they wait for the score
    fs.set_features(raw, "raw")
    assert score_code(fs) == 0
    assert all(NC.bits_equal(fs.fetch_cmvn(u), first[u]) for u in range(3))
    fs.set_speaker_stats(spk[:2])                                               # another count than the call's utterances
    assert score_code(fs) == E_STATE and "2" in error_text() and "3" in error_text()
    assert score_code(fs) == E_STATE                                            # ... and gone with the refusal
    fs.set_speaker_stats(spk)
    fs.set_norm(pk.NormSpec("speaker", True, False))                            # a new spec drops records finalised under the old one
    assert score_code(fs) == E_STATE
    fs.close()
    am.close()


# ---------------------------------------------------------------- f16x3

def test_f16x3_at_80_within_the_contract_of_the_oracle():
    """Measured on an MI355X: max |err| / max(|ref|, 1) = 4.768e-07 against the contract's 1e-4 (the printed
    NORM_F16X3_MAX_ERR line; DESIGN.md section 19 records it)."""
    D, L, R = 80, 2, 1
    am, layers, prior = tiny(D, L, R, precision="f16x3")
    raw = [NC.features(T, D, 80 + u) for u, T in enumerate((701, 0, 130, 5))]
    fs = pk.FeatureScorer(am, len(raw), sum(x.shape[0] for x in raw))
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
        want, rec = NC.normalize(x, "utterance", True, True)
        assert NC.bits_equal(fs.fetch_cmvn(u), want) and NC.bits_equal(fs.norm_stats(u), rec), u      # f32, in front of the split
        ref = nn.am_compute(want, prior, L, R, 0.1)
        worst = max(worst, float((np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)).max()))
        assert_loglik_close(got, ref)
    print("NORM_F16X3_MAX_ERR %.3e (contract 1e-4)" % worst)
    # speaker mode keeps its records through the calibration passes
    spk = [NC.accumulate(x) + NC.accumulate(raw[0]) for x in raw]
    fs.set_norm(pk.NormSpec("speaker", True, True))
    fs.set_speaker_stats(spk)
    fs.set_features(raw, "raw")
    fs.calibrate()
    fs.score(0.1)
    assert NC.bits_equal(fs.fetch_cmvn(2), NC.normalize(raw[2], "speaker", True, True, stats=spk[2])[0])
    fs.close()
    am.close()


# ---------------------------------------------------------------- failure codes

def code_of(call):
    with pytest.raises(pk.PkCodeError) as e:
        call()
    return e.value.code, str(e.value)


def test_failure_codes():
    import cmvn_any_cases as CA
    D = 41
    raw = [NC.features(T, D, 20 + u) for u, T in enumerate((9, 0, 70))]
    rec = [NC.accumulate(x) + NC.accumulate(raw[0]) for x in raw]
    am, _, _ = tiny(D, 2, 1)
    fs = pk.FeatureScorer(am, 3, 100)
    dp = C.POINTER(C.c_double)
    out = np.zeros((2, D + 1))
    # a bad spec, by field; the scorer keeps the spec it had
    for spec, word in ((pk.NormSpec(9), "mode"), (pk.NormSpec("sliding", True, True), "norm_vars"), (pk.NormSpec("utterance", False, False), "use mode none")):
        code, text = code_of(lambda: fs.set_norm(spec))
        assert code == E_INVALID and word in text
    assert pk.lib().pk_mi355_norm_set(fs._h, None) == E_INVALID
    # RAW without statistics is the norm spec's alone
    code, text = code_of(lambda: fs.set_features(raw, "raw"))
    assert code == E_INVALID and "statistics" in text
    assert code_of(lambda: fs.set_speaker_stats(rec))[0] == E_STATE             # not in mode speaker
    fs.set_norm(pk.NormSpec("none"))
    fs.set_features(raw, "raw")
    assert code_of(lambda: fs.norm_stats(0))[0] == E_STATE                      # not scored
    fs.score(0.1)
    assert code_of(lambda: fs.norm_stats(0))[0] == E_STATE                      # mode none computes none
    fs.set_norm(pk.NormSpec())                                                  # back to sliding with raw rows set: nothing to slide with
    assert score_code(fs) == E_STATE and "statistics" in error_text()
    # speaker mode
    fs.set_norm(pk.NormSpec("speaker", True, True))
    assert score_code(fs) == E_STATE and "pk_mi355_norm_set_speaker_stats" in error_text()
    for count in (0.0, -1.0, np.nan, np.inf):
        bad = [r.copy() for r in rec]
        bad[2][0, D] = count
        code, text = code_of(lambda: fs.set_speaker_stats(bad))
        assert code == E_INVALID and "utterance 2" in text and "count" in text, text
    assert score_code(fs) == E_STATE                                            # a refused call hands nothing over
    code, text = code_of(lambda: fs.set_speaker_stats(rec + rec))
    assert code == E_INVALID and "too many" in text
    assert code_of(lambda: fs.set_speaker_stats([r[:, :-1] for r in rec]))[0] == E_INVALID          # the shape, refused in Python
    assert pk.lib().pk_mi355_norm_set_speaker_stats(fs._h, None, 3) == E_INVALID
    fs.set_speaker_stats(rec)
    fs.score(0.1)
    assert code_of(lambda: fs.norm_stats(0))[0] == E_STATE                      # mode speaker computes none
    # utterance mode: the records are there after a score on raw rows, not after one on normalised features
    fs.set_norm(pk.NormSpec("utterance"))
    fs.set_features(raw, "raw")
    fs.score(0.1)
    assert NC.bits_equal(fs.norm_stats(2), NC.accumulate(raw[2]))
    assert pk.lib().pk_mi355_norm_fetch_stats(fs._h, 3, out.ctypes.data_as(dp)) == E_INVALID
    assert pk.lib().pk_mi355_norm_fetch_stats(fs._h, -1, out.ctypes.data_as(dp)) == E_INVALID
    assert pk.lib().pk_mi355_norm_fetch_stats(fs._h, 0, None) == E_INVALID
    fs.set_features(raw, "normalized")
    fs.score(0.1)
    assert code_of(lambda: fs.norm_stats(0))[0] == E_STATE
    assert NC.bits_equal(fs.fetch_cmvn(2), raw[2])                              # normalised features pass the norm by
    # every utterance frameless: records of zeros, nothing launched
    fs.set_features([raw[1], raw[1]], "raw")
    fs.score(0.1)
    assert NC.bits_equal(fs.norm_stats(1), np.zeros((2, D + 1)))
    fs.close()
    # a scorer with statistics keeps its sliding RAW path beside the spec
    g = CA.stats_for(D)
    fs = pk.FeatureScorer(am, 3, 100, global_stats=g)
    fs.set_norm(pk.NormSpec("utterance", True, True))
    fs.set_features(raw, "raw")
    fs.score(0.1)
    assert NC.bits_equal(fs.fetch_cmvn(2), NC.normalize(raw[2], "utterance", True, True)[0])
    fs.set_norm(pk.NormSpec())
    fs.score(0.1)
    assert NC.bits_equal(fs.fetch_cmvn(2), CA.cmvn_any(g, raw[2]))
    fs.close()
    am.close()
