"""Online CMVN on the GPU: OnlineCmvnKernel in front of FeatureLayoutKernel in every kind of batch
scorer, against the numpy restatement of the rule (tests/online_cmvn_cases.py).
  * Every dimension and context at W = 8, a ragged batch with frameless utterances first, in the middle and last and
    frame counts on the window's and the look-ahead group's edges (32 frames: 31, 32, 33, 63, 64, 65), on the
    `norm_cases` inputs and on the wide ones, with and without variance, with and without speaker records (counts 37 and
    0 mixed), host and device entry: fetch_cmvn equals the restatement as bits; the log-likelihoods equal the same
    scorer's NORMALIZED ones on the restatement's output, both softmax modes.  One case at the defaults (W = 600).
  * Audio: the 40-dim scorer and an 80-bin front-end.
  * NaN, +inf and -0.0 stay in their column and utterance; poisoned neighbours and reuse change no bit; speaker records
    are consumed once; a later set_norm(sliding) is an untouched scorer; one `cmvn` launch record per score; f16x3 at
    D = 80 at 1e-4 max(|ref|, 1).
  * Failure codes, before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import pocketkaldi_amd as pk
from oracle import oracle as O

import frontend_any_cases as FA
import norm_cases as NC
import online_cmvn_cases as OC
from test_gpu_cmvn_any import DeviceCopy, fetch_rows, tiny
from test_gpu_norm import code_of, error_text, same_but_nan, score_code
from test_gpu_parity import assert_loglik_close

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
DIMS = [1, 39, 40, 41, 64, 65, 80, 130]
CONTEXTS = [(0, 0), (2, 1), (5, 5)]
FRAMES = (0, 1, 2, 7, 8, 9, 17, 0, 31, 32, 33, 63, 64, 65, 130, 0)       # frameless first, in the middle and last
SPEC = (8, 3, 2)                                                        # (cmn_window, speaker_frames, global_frames)
INPUTS = {"norm_cases": OC.features, "wide": OC.wide}

_cases = {}


def case(name, D, frames=FRAMES):
    """(raw utterances, the global record, the speaker records: counts 37 and 0 in turn) of one input family at
    dimension D: computed once, shared, left unchanged."""
    key = (name, D, frames)
    if key not in _cases:
        make = INPUTS[name]
        raw = [make(T, D, 7 + u) for u, T in enumerate(frames)]
        spk = [OC.record(make(50, D, 100 + u), OC.SPEAKER_COUNT if u % 3 else 0) for u in range(len(frames))]
        _cases[key] = (raw, OC.record(make(300, D, 3)), spk)
    return _cases[key]


def wanted(raw, spec, variances, glob, spk):
    W, sf, gf = spec
    return [OC.online_cmvn(x, W, sf, gf, variances, glob if gf else None, None if spk is None else spk[u])[0] for u, x in enumerate(raw)]


# ---------------------------------------------------------------- every dimension and context

@pytest.mark.parametrize("D", DIMS)
def test_the_kernel_is_the_restatement_and_the_pads_hold_through_the_scores(D):
    for k, (L, R) in enumerate(CONTEXTS):
        am, _, _ = tiny(D, L, R, softmax=("stable", "reference")[k % 2])
        fs = pk.FeatureScorer(am, len(FRAMES), sum(FRAMES))                   # no statistics: RAW is the norm spec's alone
        fs.enable_timing(True)
        for name in sorted(INPUTS):
            raw, glob, spk = case(name, D)
            frames = [x.shape[0] for x in raw]
            dev = DeviceCopy(raw, D)
            try:
                for variances in (False, True):
                    fs.set_norm(pk.OnlineCmvnSpec(*SPEC, variances), glob)
                    for records in (None, spk):
                        what = "D=%d L=%d R=%d %s vars=%d speaker=%d" % (D, L, R, name, variances, records is not None)
                        want = wanted(raw, SPEC, variances, glob, records)
                        for device in (False, True):
                            if records is not None:
                                fs.set_speaker_stats(records)
                            if device:
                                fs.set_features_device(dev.ptr, frames, "raw")
                            else:
                                fs.set_features(raw, "raw")
                            fs.score(0.1)
                            t = fs.timing()
                            assert t["fbank"][1] == 0 and t["cmvn"][1] == 1, t    # the kernel and the layout share the CMVN slot
                            got = fetch_rows(fs)
                            for u, x in enumerate(raw):
                                assert fs.num_frames(u) == x.shape[0]
                                assert NC.bits_equal(fs.fetch_fbank(u), x), "%s utterance %d: fetch_fbank is not the input" % (what, u)
                                assert NC.bits_equal(fs.fetch_cmvn(u), want[u]), "%s utterance %d (%d frames) device=%d: rows differ" % (what, u, x.shape[0], device)
                            if not device:
                                rows = got
                                assert all(r.shape[0] == f for r, f in zip(rows, frames))
                            else:
                                assert all(NC.bits_equal(a, b) for a, b in zip(got, rows)), "%s: device entry, rows differ" % what
                        fs.set_features(want, "normalized")                       # the same scorer on the restatement's output
                        fs.score(0.1)
                        for u, r in enumerate(fetch_rows(fs)):
                            assert NC.bits_equal(r, rows[u]) or frames[u] == 0, "%s utterance %d: RAW rows differ from NORMALIZED rows" % (what, u)
            finally:
                dev.free()
        fs.close()
        am.close()


def test_the_defaults_at_80():
    D, frames = 80, (599, 0, 600, 601, 1307)
    am, _, _ = tiny(D, 2, 1)
    fs = pk.FeatureScorer(am, len(frames), sum(frames))
    for name in sorted(INPUTS):
        raw, glob, spk = case(name, D, frames)
        for variances in (False, True):
            spec = pk.OnlineCmvnSpec(norm_vars=variances)
            fs.set_norm(spec, glob)
            for records in (None, spk):
                if records is not None:
                    fs.set_speaker_stats(records)
                fs.set_features(raw, "raw")
                fs.score(0.1)
                want = wanted(raw, (600, 600, 200), variances, glob, records)
                for u in range(len(raw)):
                    assert NC.bits_equal(fs.fetch_cmvn(u), want[u]), (name, variances, records is not None, u)
                    assert NC.bits_equal(want[u], pk.cmvn_online(raw[u], spec, glob, None if records is None else records[u]))
    fs.close()
    am.close()


# ---------------------------------------------------------------- the default is the parent's path

def test_a_later_set_norm_sliding_is_an_untouched_scorer():
    import cmvn_any_cases as CA
    for D in (41, 40):
        am, _, _ = tiny(D, 2, 1)
        g = CA.stats_for(D)
        raw = [CA.features(T, D, 30 + u) for u, T in enumerate((0, 650, 3))]
        plain, back = (pk.FeatureScorer(am, 3, 653, global_stats=g) for _ in range(2))
        back.set_norm(pk.OnlineCmvnSpec(8, 3, 2, True), OC.record(raw[1]))
        back.set_features(raw, "raw")
        back.score(0.1)
        assert NC.bits_equal(back.fetch_cmvn(1), OC.online_cmvn(raw[1], 8, 3, 2, True, OC.record(raw[1]))[0])
        back.set_norm(pk.NormSpec())
        for fs in (plain, back):
            fs.enable_timing(True)
            fs.set_features(raw, "raw")
            fs.score(0.1)
        assert plain.timing()["cmvn"][1] == back.timing()["cmvn"][1] == 1
        for u in range(3):
            assert NC.bits_equal(back.fetch_cmvn(u), plain.fetch_cmvn(u)) and NC.bits_equal(back.fetch(u).log_prob(), plain.fetch(u).log_prob()), (D, u)
        assert NC.bits_equal(plain.fetch_cmvn(1), O.cmvn(g, raw[1]) if D == 40 else CA.cmvn_any(g, raw[1]))
        # ... and a NormSpec after it is that NormSpec
        back.set_norm(pk.NormSpec("utterance", True, True))
        back.set_features(raw, "raw")
        back.score(0.1)
        assert NC.bits_equal(back.fetch_cmvn(1), NC.normalize(raw[1], "utterance", True, True)[0])
        plain.close()
        back.close()
        am.close()


# ---------------------------------------------------------------- audio

AUDIO = [("batch40", None), ("fbank80", FA.SPECS[1])]


@pytest.mark.parametrize("name, spec", AUDIO, ids=[a[0] for a in AUDIO])
def test_audio(name, spec):
    D = 40 if spec is None else spec.dim
    am, _, _ = tiny(D, 2, 1)
    g = np.concatenate([np.full(D, 10.0 * 2500.0), [2500.0]]).astype(np.float32)
    waves = [FA.wave_i16(n, 50 + u).astype(np.float32) for u, n in enumerate((399, 1237, 0, 4321, 159, 2000))]
    bs = pk.BatchScorer(am, g, len(waves), sum(w.size for w in waves) + 1, frontend=spec)
    bs.set_waves(waves)
    bs.score(0.1)
    rows = [bs.fetch_fbank(u) for u in range(len(waves))]                     # the front-end's rows, pinned by its own tests
    assert [r.shape[0] for r in rows] == [pk.num_frames(w.size) for w in waves]
    glob = sum(NC.accumulate(r) for r in rows)
    spk = [NC.accumulate(rows[3])] * len(waves)
    for variances in (False, True):
        for records in (None, spk):
            want = wanted(rows, SPEC, variances, glob, records)
            bs.set_norm(pk.OnlineCmvnSpec(*SPEC, variances), glob)
            if records is not None:
                bs.set_speaker_stats(records)
            bs.set_waves(waves)
            bs.score(0.1)
            ll = fetch_rows(bs)
            for u in range(len(waves)):
                assert NC.bits_equal(bs.fetch_cmvn(u), want[u]), (name, variances, records is not None, u)
            bs.set_features(want, "normalized")
            bs.score(0.1)
            for u, r in enumerate(fetch_rows(bs)):
                assert NC.bits_equal(r, ll[u]) or rows[u].shape[0] == 0, (name, variances, u)
    bs.close()
    am.close()


# ---------------------------------------------------------------- edge values, isolation, reuse

def test_edge_values_stay_in_their_column_and_utterance():
    D = 65
    am, _, _ = tiny(D, 2, 1)
    x = NC.features(130, D, 90).copy()
    x[30, 5], x[35, 64], x[10, 7] = np.nan, np.inf, -0.0
    clean, one = NC.features(70, D, 91), NC.features(1, D, 92)
    raw = [clean, x, one, clean]
    glob = OC.record(NC.features(300, D, 3))
    touched = np.zeros(D, bool)
    touched[[5, 64]] = True
    fs = pk.FeatureScorer(am, 4, 271)
    for variances in (False, True):
        want = wanted(raw, SPEC, variances, glob, None)
        assert np.isnan(want[1][30:, 5]).all() and not np.isfinite(want[1][35:, 64]).any() and np.isfinite(want[1][:, ~touched]).all()
        assert np.isfinite(want[1][:30, 5]).all() and np.isfinite(want[1][:35, 64]).all()
        fs.set_norm(pk.OnlineCmvnSpec(*SPEC, variances), glob)
        fs.set_features(raw, "raw")
        fs.score(0.1)
        for u in range(4):
            assert same_but_nan(fs.fetch_cmvn(u), want[u]), (variances, u)
        assert NC.bits_equal(fs.fetch_cmvn(0), fs.fetch_cmvn(3)) and NC.bits_equal(fs.fetch(0).log_prob(), fs.fetch(3).log_prob())
        assert np.isfinite(fs.fetch(0).log_prob()).all()
    fs.close()
    am.close()


def test_poisoned_neighbours_and_reuse_change_no_bit():
    D, L, R = 41, 2, 1
    am, _, _ = tiny(D, L, R)
    sets = {"large": [NC.features(T, D, 60 + u) for u, T in enumerate((130, 0, 64, 1))], "small": [NC.features(T, D, 70 + u) for u, T in enumerate((5, 33))]}
    cap = 195
    glob = OC.record(NC.features(300, D, 3))
    recs = {k: [OC.record(x if x.shape[0] else v[0], OC.SPEAKER_COUNT) for x in v] for k, v in sets.items()}
    specs = [(pk.OnlineCmvnSpec(*SPEC, True), True), (pk.OnlineCmvnSpec(*SPEC, False), False), (pk.OnlineCmvnSpec(33, 5, 0, True), True),
             (pk.NormSpec("utterance", True, True), False)]

    def run(fs, which, i):
        spec, speaker = specs[i]
        if isinstance(spec, pk.OnlineCmvnSpec):
            fs.set_norm(spec, glob if spec.global_frames else None)
        else:
            fs.set_norm(spec)
        if speaker:
            fs.set_speaker_stats(recs[which])
        fs.set_features(sets[which], "raw")
        fs.score(0.1)
        return [fs.fetch_cmvn(u) for u in range(len(sets[which]))], fetch_rows(fs)

    def fresh(which, i):
        fs = pk.FeatureScorer(am, 4, cap)
        out = run(fs, which, i)
        fs.close()
        return out

    want = {(which, i): fresh(which, i) for which in sets for i in range(len(specs))}
    for (which, i), (cm, _) in want.items():                                      # (and the fresh results are the restatement)
        s, speaker = specs[i]
        if isinstance(s, pk.OnlineCmvnSpec):
            ref = wanted(sets[which], (s.cmn_window, s.speaker_frames, s.global_frames), s.norm_vars, glob, recs[which] if speaker else None)
            assert all(NC.bits_equal(c, r) for c, r in zip(cm, ref)), (which, i)
    one = pk.FeatureScorer(am, 4, cap)
    for which in ("large", "small", "large"):
        for i in range(len(specs)):                                              # the specs in turn on one object
            cm, rows = run(one, which, i)
            assert all(NC.bits_equal(a, b) for a, b in zip(cm, want[(which, i)][0])), (which, i)
            assert all(NC.bits_equal(a, b) for a, b in zip(rows, want[(which, i)][1])), (which, i)
            one.set_norm(pk.NormSpec("none"))                                    # poison every buffer in between
            one.set_features([np.full(x.shape, np.nan, np.float32) for x in sets["large"]], "raw")
            one.score(0.1)
            assert all(np.isnan(r).all() for r in fetch_rows(one))
    one.close()
    # NaN and 1e30 utterances between healthy ones
    feats = sets["large"]
    mixed = [feats[0], np.full((70, D), np.nan, np.float32), feats[2], np.full((3, D), 1e30, np.float32), feats[3]]
    pairs = ((0, 0), (2, 2), (4, 3))
    wide = pk.FeatureScorer(am, 5, cap + 73)
    wide.set_norm(specs[0][0], glob)
    stats = [np.full((2, D + 1), np.nan)] * 5
    for at, u in pairs:
        stats[at] = recs["large"][u]
    stats[1], stats[3] = np.ones((2, D + 1)), np.full((2, D + 1), 1e300)
    wide.set_speaker_stats(stats)
    wide.set_features(mixed, "raw")
    wide.score(0.1)
    cm, rows = want[("large", 0)]
    for at, u in pairs:
        assert NC.bits_equal(wide.fetch_cmvn(at), cm[u]) and NC.bits_equal(wide.fetch(at).log_prob(), rows[u]), at
    assert np.isnan(wide.fetch(1).log_prob()).all()
    wide.close()
    am.close()


def test_speaker_statistics_are_optional_and_consumed_by_one_score():
    D = 39
    raw, glob, spk = case("norm_cases", D)
    raw, spk = raw[8:11], [OC.record(x, OC.SPEAKER_COUNT) for x in raw[8:11]]
    am, _, _ = tiny(D, 2, 1)
    fs = pk.FeatureScorer(am, 3, 200)
    fs.set_norm(pk.OnlineCmvnSpec(*SPEC, True), glob)
    with_records, without = wanted(raw, SPEC, True, glob, spk), wanted(raw, SPEC, True, glob, None)
    assert not any(NC.bits_equal(a, b) for a, b in zip(with_records, without))
    fs.set_speaker_stats(spk)
    fs.set_features(raw, "raw")
    fs.score(0.1)
    assert all(NC.bits_equal(fs.fetch_cmvn(u), with_records[u]) for u in range(3))
    fs.score(0.1)                                                               # consumed: the next score has no speaker prior
    assert all(NC.bits_equal(fs.fetch_cmvn(u), without[u]) for u in range(3))
    fs.set_speaker_stats(spk)                                                   # set before the features: they wait for the score
    fs.set_features(raw, "raw")
    fs.score(0.1)
    assert all(NC.bits_equal(fs.fetch_cmvn(u), with_records[u]) for u in range(3))
    fs.set_speaker_stats(spk[:2])                                               # another count than the call's utterances
    assert score_code(fs) == E_STATE and "2" in error_text() and "3" in error_text()
    assert score_code(fs) == 0                                                  # ... and gone with the refusal
    assert all(NC.bits_equal(fs.fetch_cmvn(u), without[u]) for u in range(3))
    fs.set_speaker_stats(spk)
    fs.set_norm(pk.OnlineCmvnSpec(*SPEC, True), glob)                           # a new spec drops the records handed over under the old one
    fs.score(0.1)
    assert all(NC.bits_equal(fs.fetch_cmvn(u), without[u]) for u in range(3))
    fs.close()
    am.close()


# ---------------------------------------------------------------- f16x3

def test_f16x3_at_80_within_the_contract_of_the_oracle():
    """Measured on an MI355X: max |err| / max(|ref|, 1) = 3.576e-07 against the contract's 1e-4 (the printed
    ONLINE_CMVN_F16X3_MAX_ERR line; DESIGN.md section 20 records it)."""
    D, L, R = 80, 2, 1
    am, layers, prior = tiny(D, L, R, precision="f16x3")
    raw = [NC.features(T, D, 80 + u) for u, T in enumerate((131, 0, 64, 5))]
    glob = OC.record(NC.features(300, D, 3))
    fs = pk.FeatureScorer(am, len(raw), sum(x.shape[0] for x in raw))
    fs.set_norm(pk.OnlineCmvnSpec(*SPEC, True), glob)
    fs.set_features(raw, "raw")
    fs.calibrate()
    fs.score(0.1)
    nn = O.Nnet(layers)
    worst = 0.0
    want = wanted(raw, SPEC, True, glob, None)
    for u, x in enumerate(raw):
        got = fs.fetch(u).log_prob()
        if x.shape[0] == 0:
            assert got.shape[0] == 0
            continue
        assert NC.bits_equal(fs.fetch_cmvn(u), want[u]), u                      # f32, in front of the split
        ref = nn.am_compute(want[u], prior, L, R, 0.1)
        worst = max(worst, float((np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)).max()))
        assert_loglik_close(got, ref)
    print("ONLINE_CMVN_F16X3_MAX_ERR %.3e (contract 1e-4)" % worst)
    # the speaker records stay through the calibration passes
    spk = [OC.record(raw[0], OC.SPEAKER_COUNT)] * len(raw)
    fs.set_speaker_stats(spk)
    fs.set_features(raw, "raw")
    fs.calibrate()
    fs.score(0.1)
    assert NC.bits_equal(fs.fetch_cmvn(2), OC.online_cmvn(raw[2], *SPEC, True, glob, spk[2])[0])
    fs.close()
    am.close()


# ---------------------------------------------------------------- failure codes

def test_failure_codes():
    D = 41
    raw = [NC.features(T, D, 20 + u) for u, T in enumerate((9, 0, 70))]
    glob = OC.record(NC.features(300, D, 3))
    rec = [OC.record(raw[0], OC.SPEAKER_COUNT)] * 3
    am, _, _ = tiny(D, 2, 1)
    fs = pk.FeatureScorer(am, 3, 100)
    # a bad spec, by field; the scorer keeps the norm it had (sliding, without statistics: RAW is refused)
    for spec, g, word in ((pk.OnlineCmvnSpec(0), glob, "cmn_window"), (pk.OnlineCmvnSpec(6001), glob, "cmn_window"),
                          (pk.OnlineCmvnSpec(8, -1, 2), glob, "speaker_frames"), (pk.OnlineCmvnSpec(8, 3, -1), glob, "global_frames"),
                          (pk.OnlineCmvnSpec(8, 3, 2, 2), glob, "norm_vars"), (pk.OnlineCmvnSpec(8, 3, 2), None, "global_frames")):
        code, text = code_of(lambda: fs.set_norm(spec, g))
        assert code == E_INVALID and word in text, text
    for count in (0.0, -1.0, np.nan, np.inf):
        bad = glob.copy()
        bad[0, D] = count
        code, text = code_of(lambda: fs.set_norm(pk.OnlineCmvnSpec(8, 3, 2), bad))
        assert code == E_INVALID and "count" in text, text
    assert code_of(lambda: fs.set_norm(pk.OnlineCmvnSpec(8, 3, 2), glob[:, :-1]))[0] == E_INVALID       # the shape, refused in Python
    assert code_of(lambda: fs.set_norm(pk.NormSpec("none"), glob))[0] == E_INVALID
    assert pk.lib().pk_mi355_norm_set_online_cmvn(fs._h, None, None) == E_INVALID
    code, text = code_of(lambda: fs.set_features(raw, "raw"))
    assert code == E_INVALID and "statistics" in text
    assert code_of(lambda: fs.set_speaker_stats(rec))[0] == E_STATE             # neither mode speaker nor online CMVN
    # online CMVN: RAW goes, no statistics come back
    fs.set_norm(pk.OnlineCmvnSpec(8, 3, 0), None)                               # global_frames = 0 needs no record
    fs.set_features(raw, "raw")
    fs.score(0.1)
    assert NC.bits_equal(fs.fetch_cmvn(2), OC.online_cmvn(raw[2], 8, 3, 0, False)[0])
    assert code_of(lambda: fs.norm_stats(0))[0] == E_STATE
    for count in (-1.0, np.nan, np.inf):
        bad = [r.copy() for r in rec]
        bad[2][0, D] = count
        code, text = code_of(lambda: fs.set_speaker_stats(bad))
        assert code == E_INVALID and "utterance 2" in text and "count" in text, text
    assert score_code(fs) == 0                                                  # a refused call hands nothing over
    assert NC.bits_equal(fs.fetch_cmvn(2), OC.online_cmvn(raw[2], 8, 3, 0, False)[0])
    code, text = code_of(lambda: fs.set_speaker_stats(rec + rec))
    assert code == E_INVALID and "too many" in text
    assert pk.lib().pk_mi355_norm_set_speaker_stats(fs._h, None, 3) == E_INVALID
    # normalised features pass the norm by; every utterance frameless launches nothing
    fs.set_features(raw, "normalized")
    fs.score(0.1)
    assert NC.bits_equal(fs.fetch_cmvn(2), raw[2])
    fs.set_features([raw[1], raw[1]], "raw")
    fs.score(0.1)
    assert fs.num_frames(0) == 0
    # mode speaker after online CMVN needs its records again
    fs.set_speaker_stats([rec[0], rec[0]])
    fs.set_norm(pk.NormSpec("speaker", True, True))
    fs.set_features(raw, "raw")
    assert score_code(fs) == E_STATE and "pk_mi355_norm_set_speaker_stats" in error_text()
    fs.close()
    am.close()
