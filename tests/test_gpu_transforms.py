"""Feature transforms on the GPU: TransformKernel between the normalisation (or the deltas) and
FeatureLayoutKernel in a batch scorer made with transform=, against the numpy restatement of the rule
(tests/transform_cases.py).
  * Every in_dim, context, row count (the edges of a 64-output block, three blocks), affine and linear, each axis swept
    with the others at a middle value plus mixed cases and the widest accepted spec; ragged batches with frameless
    utterances first, in the middle and last and frame counts around the contexts and the kernel's run of G frames:
    fetch_cmvn equals the restatement as bits, the log-likelihoods equal a plain FeatureScorer's on the host result fed
    as NORMALIZED, host and device entry, both softmax modes.
  * Every norm mode and deltas in front; the global matrix alone, per-utterance matrices alone, both; audio through a
    13-of-23 MFCC; NaN, inf x 0; poisoned neighbours and reused buffers; one object walked through its cells in two
    orders; batches of the existing entries beside a transform batch, bit for bit and launch for launch; f16x3 at
    feat_dim = 40 within the contract; every failure code."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pocketkaldi_amd as pk
from oracle import oracle as O

import cmvn_any_cases as CA
import frontend_any_cases as FA
import norm_cases as NC
import transform_cases as XC
from test_gpu_cmvn_any import DeviceCopy, fetch_rows, tiny
from test_gpu_parity import assert_loglik_close

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
G = int(re.search(r"kTransformFrames\s*=\s*(\d+)", open(os.path.join(REPO, "pocketkaldi_amd", "csrc", "pk_transform_kernel.h")).read()).group(1))
MID = (13, 3, 3, 40, True)            # (in_dim, L, R, rows, affine): the middle value of every axis
SHAPES = ([(d, 3, 3, 40, True) for d in (1, 40, 63, 64, 65)] + [(13, L, R, 40, True) for L, R in ((0, 0), (1, 2), (0, 16), (8, 8))] +
          [(13, 3, 3, r, True) for r in (1, 63, 64, 65, 130)] + [MID, (13, 3, 3, 40, False)] +
          [(65, 0, 16, 130, False), (64, 8, 8, 65, True), (1, 0, 0, 1, True), (63, 1, 2, 63, False), (512, 8, 8, 3, False)])


def frame_list(L, R):
    """Frameless first, in the middle and last; T in {1, 2, L, R, L + R, L + R + 1, G - 1, G, G + 1, 2 G + 1}."""
    ts = sorted({1, 2, L, R, L + R, L + R + 1, G - 1, G, G + 1, 2 * G + 1} - {0})
    half = len(ts) // 2
    return [0] + ts[:half] + [0] + ts[half:] + [0]


_raw = {}


def raw_case(Dp, frames):
    """The utterances of a shape: computed once, shared, left unchanged."""
    key = (Dp, tuple(frames))
    if key not in _raw:
        _raw[key] = [NC.features(T, Dp, 7 + u) if u % 2 else XC.wide(T, Dp, 7 + u) for u, T in enumerate(frames)]
    return _raw[key]


def score_code(fs):
    return pk.lib().pk_mi355_batch_score(fs._h, C.c_float(0.1), 1)


def error_text():
    return pk.lib().pk_mi355_last_error().decode()


def code_of(call):
    with pytest.raises(pk.PkCodeError) as e:
        call()
    return e.value.code, str(e.value)


def utt_matrices(n, D, affine=True, seed=40):
    return [XC.matrix(D, 0, 0, D, affine, seed=seed + u) for u in range(n)]


# ---------------------------------------------------------------- every shape

@pytest.mark.parametrize("shape", SHAPES, ids=["%d-%d-%d-%d-%s" % (s[0], s[1], s[2], s[3], "affine" if s[4] else "linear") for s in SHAPES])
def test_every_shape_is_the_restatement_and_the_scores_are_the_normalized_ones(shape):
    Dp, L, R, rows, affine = shape
    m = XC.matrix(*shape)
    spec = pk.TransformSpec(m, L, R, in_dim=Dp)
    frames = frame_list(L, R)
    raw = raw_case(Dp, frames)
    want = [XC.transform(x, m, L, R) for x in raw]
    dev = DeviceCopy(raw, Dp)
    try:
        for softmax in (("stable", "reference") if shape == MID else (("stable", "reference")[SHAPES.index(shape) % 2],)):
            am, _, _ = tiny(rows, 2, 1, softmax=softmax)
            fs = pk.FeatureScorer(am, len(raw), sum(frames), transform=spec)
            plain = pk.FeatureScorer(am, len(raw), sum(frames))
            assert (fs.in_dim(), fs.base_dim(), fs.feat_dim(), plain.in_dim()) == (Dp, Dp, rows, rows)
            fs.set_norm(pk.NormSpec("none"))
            fs.enable_timing(True)
            plain.set_features(want, "normalized")
            plain.score(0.1)
            ll = fetch_rows(plain)
            for device in (False, True):
                if device:
                    fs.set_features_device(dev.ptr, frames, "raw")
                else:
                    fs.set_features(raw, "raw")
                fs.score(0.1)
                t = fs.timing()
                assert t["fbank"][1] == 0 and t["cmvn"][1] == 1, t              # TransformKernel and the layout share the CMVN slot
                got = fetch_rows(fs)
                for u, x in enumerate(raw):
                    what = "%s utterance %d (%d frames) device=%d" % (shape, u, x.shape[0], device)
                    assert fs.num_frames(u) == x.shape[0]
                    assert NC.bits_equal(fs.fetch_fbank(u), x), what + ": fetch_fbank is not the input"
                    assert NC.bits_equal(fs.fetch_cmvn(u), want[u]), what + ": rows differ"
                    assert NC.bits_equal(got[u], ll[u]) or frames[u] == 0, what + ": scores differ from NORMALIZED"
            fs.set_features(want, "normalized")                                 # NORMALIZED passes every stage by
            fs.score(0.1)
            for u, r in enumerate(fetch_rows(fs)):
                assert NC.bits_equal(r, ll[u]) or frames[u] == 0
                assert NC.bits_equal(fs.fetch_cmvn(u), want[u])
            for o in (fs, plain, am):
                o.close()
    finally:
        dev.free()


# ---------------------------------------------------------------- every norm mode, and deltas, in front of the transform

NORMS = [("none", 13), ("utterance", 13), ("speaker", 65), ("online", 13), ("sliding", 40), ("sliding", 41)]


@pytest.mark.parametrize("mode, Db", NORMS, ids=["%s-%d" % n for n in NORMS])
def test_every_norm_mode_in_front_of_the_transform(mode, Db):
    L, R, rows = 2, 1, 40
    m = XC.matrix(Db, L, R, rows, True)
    spec = pk.TransformSpec(m, L, R)
    frames = [0, 5, 40, 0, 1, 33, 130, 0]
    raw = [CA.features(T, Db, 30 + u) for u, T in enumerate(frames)]
    g = CA.stats_for(Db) if mode == "sliding" else None
    rec = [NC.accumulate(x) for x in raw]
    spk = [r + rec[2] for r in rec]
    am_base, _, _ = tiny(Db, 2, 1)
    am, _, _ = tiny(rows, 2, 1)
    plain = pk.FeatureScorer(am_base, len(raw), sum(frames), global_stats=g)
    fs = pk.FeatureScorer(am, len(raw), sum(frames), global_stats=g, transform=spec)
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
        assert NC.bits_equal(fs.fetch_cmvn(u), XC.transform(base, m, L, R)), (mode, Db, u)
        assert NC.bits_equal(fs.fetch_fbank(u), x)
        if mode == "utterance":                                                 # the records are at Db
            assert fs.norm_stats(u).shape == (2, Db + 1) and NC.bits_equal(fs.norm_stats(u), rec[u]), u
    if mode == "utterance":
        assert NC.bits_equal(plain.fetch_cmvn(2), NC.normalize(raw[2], "utterance", True, True)[0])
    if mode == "sliding":
        assert NC.bits_equal(plain.fetch_cmvn(6), O.cmvn(g, raw[6]) if Db == 40 else CA.cmvn_any(g, raw[6]))
    for o in (plain, fs, am, am_base):
        o.close()


def test_deltas_in_front_of_the_transform():
    """13 -> 39 -> 39 affine: fMLLR's global stand-in on a delta system; then per-utterance matrices behind it."""
    import delta_cases as DC
    Db, D = 13, 39
    deltas = pk.DeltaSpec(2, 2)
    m = XC.matrix(D, 0, 0, D, True)
    am, _, _ = tiny(D, 2, 1)
    frames = [0, 1, 5, G + 1, 0, 2 * G + 1, 0]
    raw = [NC.features(T, Db, 60 + u) for u, T in enumerate(frames)]
    fs = pk.FeatureScorer(am, len(raw), sum(frames), deltas=deltas, transform=pk.TransformSpec(m, in_dim=D))
    assert (fs.in_dim(), fs.base_dim(), fs.feat_dim()) == (D, Db, D)
    fs.set_norm(pk.NormSpec("utterance", True, True))
    fs.set_features(raw, "raw")
    fs.score(0.1)
    mid = [DC.add_deltas(NC.normalize(x, "utterance", True, True)[0], 2, 2) for x in raw]
    for u in range(len(raw)):
        assert NC.bits_equal(fs.fetch_cmvn(u), XC.transform(mid[u], m, 0, 0)), u
    mats = utt_matrices(len(raw), D)
    fs.set_utt_transforms(mats)
    fs.score(0.1)
    for u in range(len(raw)):
        assert NC.bits_equal(fs.fetch_cmvn(u), XC.transform(XC.transform(mid[u], m, 0, 0), mats[u], 0, 0)), u
    # without a global matrix the deltas' rows go straight to the per-utterance stage
    only = pk.FeatureScorer(am, len(raw), sum(frames), deltas=deltas, transform=pk.TransformSpec(None, in_dim=D))
    only.set_norm(pk.NormSpec("utterance", True, True))
    only.set_features(raw, "raw")
    only.set_utt_transforms(mats)
    only.score(0.1)
    for u in range(len(raw)):
        assert NC.bits_equal(only.fetch_cmvn(u), XC.transform(mid[u], mats[u], 0, 0)), u
    for o in (fs, only, am):
        o.close()


# ---------------------------------------------------------------- the global matrix, per-utterance matrices, both

@pytest.mark.parametrize("affine", [True, False], ids=["affine", "linear"])
def test_global_alone_per_utterance_alone_and_both(affine):
    Dp, L, R, D = 13, 3, 3, 40
    m = XC.matrix(Dp, L, R, D, True)
    am, _, _ = tiny(D, 2, 1)
    frames = [0, 3, G, 0, 1, 2 * G + 1, 7, 0]
    raw = raw_case(Dp, frames)
    raw40 = raw_case(D, frames)
    mats = utt_matrices(len(frames), D, affine)               # all different: a wrong index shows
    glob = [XC.transform(x, m, L, R) for x in raw]
    both = XC.transform_utts(glob, mats)
    wrong = XC.transform_utts(glob, mats, neighbour=True)
    assert all(XC.outputs_differing(a, b) > 0 for a, b in zip(both, wrong) if a.size)

    def fresh():
        return pk.FeatureScorer(am, len(frames), sum(frames), transform=pk.TransformSpec(m, L, R))

    def rows_of(fs, feats, matrices):
        fs.set_norm(pk.NormSpec("none"))
        fs.set_features(feats, "raw")
        if matrices is not None:
            fs.set_utt_transforms(matrices)
        fs.score(0.1)
        return [fs.fetch_cmvn(u) for u in range(len(feats))], fetch_rows(fs)

    fs = fresh()
    first = rows_of(fs, raw, None)
    assert all(NC.bits_equal(a, b) for a, b in zip(first[0], glob))
    second = rows_of(fs, raw, mats)
    assert all(NC.bits_equal(a, b) for a, b in zip(second[0], both))
    third = rows_of(fs, raw, None)                              # the matrices were consumed: the stage does not run again
    ref = rows_of(fresh(), raw, None)
    assert all(NC.bits_equal(a, b) for a, b in zip(third[0] + third[1], ref[0] + ref[1]))
    assert all(NC.bits_equal(a, b) for a, b in zip(third[0] + third[1], first[0] + first[1]))
    # the scores behind both stages are those of the host result fed as NORMALIZED
    plain = pk.FeatureScorer(am, len(frames), sum(frames))
    plain.set_features(both, "normalized")
    plain.score(0.1)
    assert all(NC.bits_equal(a, b) or T == 0 for a, b, T in zip(second[1], fetch_rows(plain), frames))
    # per-utterance matrices alone: no global stage
    only = pk.FeatureScorer(am, len(frames), sum(frames), transform=pk.TransformSpec(None, in_dim=D))
    assert (only.in_dim(), only.base_dim(), only.feat_dim()) == (D, D, D)
    got = rows_of(only, raw40, mats)
    assert all(NC.bits_equal(a, b) for a, b in zip(got[0], XC.transform_utts(raw40, mats)))
    got = rows_of(only, raw40, None)                            # and without them the rows as they are
    assert all(NC.bits_equal(a, b) for a, b in zip(got[0], raw40))
    # matrices for another number of utterances: the score call fails, and consumes them
    fs.set_features(raw, "raw")
    fs.set_utt_transforms(mats[:3])
    assert score_code(fs) == E_STATE and "3 utterances" in error_text() and "%d" % len(frames) in error_text()
    fs.score(0.1)
    assert all(NC.bits_equal(fs.fetch_cmvn(u), glob[u]) for u in range(len(frames)))
    for o in (fs, plain, only, am):
        o.close()


# ---------------------------------------------------------------- audio

def test_audio_through_an_mfcc_front_end():
    fe = FA.SPECS[9]                                                            # 13 of 23 MFCC
    Db, L, R, D = fe.dim, 3, 3, 40
    assert Db == 13
    m = XC.matrix(Db, L, R, D, True)
    spec = pk.TransformSpec(m, L, R)
    am_base, _, _ = tiny(Db, 2, 1)
    am, _, _ = tiny(D, 2, 1)
    g = np.concatenate([np.full(Db, 10.0 * 2500.0), [2500.0]]).astype(np.float32)
    waves = [FA.wave_i16(n, 50 + u).astype(np.float32) for u, n in enumerate((399, 1237, 0, 4321, 159, 2000))]
    cap = sum(w.size for w in waves) + 1
    plain = pk.BatchScorer(am_base, g, len(waves), cap, frontend=fe)
    bs = pk.BatchScorer(am, g, len(waves), cap, frontend=fe, transform=spec)
    assert (bs.in_dim(), bs.base_dim(), bs.feat_dim()) == (Db, Db, D)
    front = pk.Frontend(fe)
    for norm in (None, pk.NormSpec("utterance", True, True)):
        for o in (plain, bs):
            if norm is not None:
                o.set_norm(norm)
            o.set_waves(waves)
            o.score(0.1)
        for u, w in enumerate(waves):
            rows = bs.fetch_fbank(u)
            assert rows.shape == (pk.num_frames(w.size), Db) and NC.bits_equal(rows, front.compute(w).reshape(rows.shape)), u
            assert NC.bits_equal(bs.fetch_cmvn(u), XC.transform(plain.fetch_cmvn(u), m, L, R)), (norm, u)
            if norm is not None:
                assert NC.bits_equal(bs.norm_stats(u), NC.accumulate(rows)), u
    rows = [bs.fetch_fbank(u) for u in range(len(waves))]                       # the same rows as raw features: the audio's bits
    ll = fetch_rows(bs)
    bs.set_features(rows, "raw")
    bs.score(0.1)
    assert all(NC.bits_equal(a, b) or r.shape[0] == 0 for a, b, r in zip(fetch_rows(bs), ll, rows))
    for o in (plain, bs, am, am_base):
        o.close()


# ---------------------------------------------------------------- edge values, isolation, reuse

def test_edge_values_stay_in_their_frames_and_utterance():
    Dp, L, R, D = 13, 3, 2, 65
    m = XC.matrix(Dp, L, R, D, True)
    m[5, :] = 0.0                                                               # a zero row: inf x 0 is NaN, no tap is skipped
    am, _, _ = tiny(D, 2, 1)
    x = NC.features(60, Dp, 90)
    x[20, 5], x[45, 12], x[0, 0] = np.nan, np.inf, np.nan
    clean = NC.features(40, Dp, 91)
    raw = [clean, x, NC.features(1, Dp, 92), clean]
    fs = pk.FeatureScorer(am, 4, 141, transform=pk.TransformSpec(m, L, R))
    fs.set_norm(pk.NormSpec("none"))
    fs.set_features(raw, "raw")
    fs.score(0.1)
    want = [XC.transform(r, m, L, R) for r in raw]
    for u in range(4):
        assert XC.same_but_nan(fs.fetch_cmvn(u), want[u]), u
    got = fs.fetch_cmvn(1)
    nan_rows = np.isnan(got).all(axis=1)
    assert sorted(np.flatnonzero(nan_rows)) == sorted(set(range(0, L + 1)) | set(range(20 - R, 20 + L + 1)))     # [t - R, t + L]
    inf_rows = [t for t in range(45 - R, 45 + L + 1)]
    assert np.isnan(got[inf_rows, 5]).all() and np.isinf(got[inf_rows, 0]).all()                                 # the zero row meets the inf
    rest = np.ones(60, bool)
    rest[np.flatnonzero(nan_rows)] = False
    rest[inf_rows] = False
    assert np.isfinite(got[rest]).all()
    assert NC.bits_equal(fs.fetch_cmvn(0), fs.fetch_cmvn(3)) and NC.bits_equal(fs.fetch(0).log_prob(), fs.fetch(3).log_prob())
    assert np.isfinite(fs.fetch(0).log_prob()).all() and np.isfinite(fs.fetch(2).log_prob()).all()
    z = pk.FeatureScorer(am, 1, 4, transform=pk.TransformSpec(-np.abs(m), L, R))           # -0.0 cannot survive the +0.0f start
    z.set_norm(pk.NormSpec("none"))
    z.set_features([np.full((4, Dp), -0.0, np.float32)], "raw")
    z.score(0.1)
    zr = z.fetch_cmvn(0)
    assert NC.bits_equal(zr[:, 5], np.zeros(4, np.float32)) and NC.bits_equal(zr, XC.transform(np.full((4, Dp), -0.0, np.float32), -np.abs(m), L, R))
    for o in (fs, z, am):
        o.close()


def test_poisoned_neighbours_and_reuse_change_no_bit():
    Dp, L, R, D = 41, 2, 3, 40
    m = XC.matrix(Dp, L, R, D, True)
    spec = pk.TransformSpec(m, L, R)
    am, _, _ = tiny(D, 2, 1)
    sets = {"large": [NC.features(T, Dp, 60 + u) for u, T in enumerate((130, 0, 64, 1))],
            "small": [NC.features(T, Dp, 70 + u) for u, T in enumerate((5, 33))]}
    mats = {which: utt_matrices(len(v), D, seed=80) for which, v in sets.items()}
    cap = 195
    cells = [(pk.NormSpec("none"), False), (pk.NormSpec("utterance", True, True), True)]

    def run(fs, which, cell):
        fs.set_norm(cell[0])
        fs.set_features(sets[which], "raw")
        if cell[1]:
            fs.set_utt_transforms(mats[which])
        fs.score(0.1)
        return [fs.fetch_cmvn(u) for u in range(len(sets[which]))], fetch_rows(fs)

    def fresh(which, cell):
        fs = pk.FeatureScorer(am, 4, cap, transform=spec)
        out = run(fs, which, cell)
        fs.close()
        return out

    want = {(which, i): fresh(which, c) for which in sets for i, c in enumerate(cells)}
    for (which, i), (cm, _) in want.items():                                    # (and the fresh results are the restatement)
        mode = ("none", "utterance")[i]
        rows = [XC.transform(NC.normalize(x, mode, True, True)[0], m, L, R) for x in sets[which]]
        if cells[i][1]:
            rows = XC.transform_utts(rows, mats[which])
        assert all(NC.bits_equal(c, r) for c, r in zip(cm, rows)), (which, i)
    one = pk.FeatureScorer(am, 4, cap, transform=spec)
    poison = [np.full(x.shape, np.nan, np.float32) for x in sets["large"]]
    for which in ("large", "small", "large"):
        for i, c in enumerate(cells):
            cm, rows = run(one, which, c)
            assert all(NC.bits_equal(a, b) for a, b in zip(cm, want[(which, i)][0])), (which, i)
            assert all(NC.bits_equal(a, b) for a, b in zip(rows, want[(which, i)][1])), (which, i)
            one.set_norm(pk.NormSpec("none"))                                  # poison every buffer in between
            one.set_features(poison, "raw")
            one.set_utt_transforms(utt_matrices(4, D, seed=99))
            one.score(0.1)
            assert all(np.isnan(r).all() for r in fetch_rows(one))
    one.close()
    # NaN and 1e30 utterances between healthy ones
    feats = sets["large"]
    mixed = [feats[0], np.full((77, Dp), np.nan, np.float32), feats[2], np.full((3, Dp), 1e30, np.float32), feats[3]]
    wide = pk.FeatureScorer(am, 5, cap + 80, transform=spec)
    wide.set_norm(pk.NormSpec("none"))
    wide.set_features(mixed, "raw")
    wide.score(0.1)
    cm, rows = want[("large", 0)]
    for at, u in ((0, 0), (2, 2), (4, 3)):
        assert NC.bits_equal(wide.fetch_cmvn(at), cm[u]) and NC.bits_equal(wide.fetch(at).log_prob(), rows[u]), at
    assert np.isnan(wide.fetch(1).log_prob()).all()
    wide.close()
    am.close()


def test_one_object_walked_through_its_cells_in_two_orders():
    Dp, L, R, D = 13, 1, 2, 40
    m = XC.matrix(Dp, L, R, D, False)
    spec = pk.TransformSpec(m, L, R)
    am, _, _ = tiny(D, 2, 1)
    frames = [G + 1, 0, 3, 2 * G + 1]
    raw = raw_case(Dp, frames)
    done = [XC.normal(T, D, 5 + u) for u, T in enumerate(frames)]
    mats = utt_matrices(len(frames), D)
    g = CA.stats_for(Dp)
    cells = [(source, mode, utt) for source in ("raw", "normalized") for mode in ("sliding", "none", "utterance") for utt in (False, True)]

    def run(fs, cell):
        source, mode, utt = cell
        fs.set_norm(pk.NormSpec(mode, True, mode == "utterance"))
        fs.set_features(raw if source == "raw" else done, source)
        if utt:
            fs.set_utt_transforms(mats)
        fs.score(0.1)
        return [fs.fetch_cmvn(u) for u in range(len(frames))] + fetch_rows(fs)

    def fresh(cell):
        fs = pk.FeatureScorer(am, len(frames), sum(frames), global_stats=g, transform=spec)
        out = run(fs, cell)
        fs.close()
        return out

    want = {c: fresh(c) for c in cells}
    for c in cells:                                                             # NORMALIZED rows pass every stage by, matrices or not
        if c[0] == "normalized":
            assert all(NC.bits_equal(a, b) for a, b in zip(want[c][:len(frames)], done)), c
    one = pk.FeatureScorer(am, len(frames), sum(frames), global_stats=g, transform=spec)
    for order in (cells, cells[::-1]):
        for c in order:
            got = run(one, c)
            assert all(NC.bits_equal(a, b) for a, b in zip(got, want[c])), c
    one.close()
    am.close()


# ---------------------------------------------------------------- the existing entries beside a transform batch

def test_batches_of_the_existing_entries_are_unchanged_beside_a_transform_batch():
    fe = FA.SPECS[9]
    am40, _, _ = tiny(40, 2, 1)
    am13, _, _ = tiny(13, 2, 1)
    am39, _, _ = tiny(39, 2, 1)
    g40, g13 = CA.stats_for(40), CA.stats_for(13)
    waves = [FA.wave_i16(n, 50 + u).astype(np.float32) for u, n in enumerate((1237, 0, 2000))]
    cap = sum(w.size for w in waves) + 1
    f40 = [CA.features(T, 40, 3 + u) for u, T in enumerate((9, 0, 70))]
    f13 = [CA.features(T, 13, 3 + u) for u, T in enumerate((9, 0, 70))]
    entries = {
        "batch_create": (lambda: pk.BatchScorer(am40, g40, 3, cap), lambda b: b.set_waves(waves)),
        "features_batch_create": (lambda: pk.FeatureScorer(am40, 3, 100, global_stats=g40), lambda b: b.set_features(f40, "raw")),
        "features_batch_create_stats": (lambda: pk.FeatureScorer(am13, 3, 100, global_stats=g13), lambda b: b.set_features(f13, "raw")),
        "frontend_batch_create": (lambda: pk.BatchScorer(am13, g13, 3, cap, frontend=fe), lambda b: b.set_waves(waves)),
        "deltas_batch_create": (lambda: pk.FeatureScorer(am39, 3, 100, global_stats=g13, deltas=pk.DeltaSpec(2, 2)), lambda b: b.set_features(f13, "raw")),
    }

    def run_all():
        out = {}
        for name, (make, feed) in entries.items():
            b = make()
            b.enable_timing(True)
            feed(b)
            b.score(0.1)
            out[name] = ([b.fetch_cmvn(u) for u in range(3)] + fetch_rows(b), [v[1] for v in b.timing().values()], b.in_dim(), b.feat_dim())
            b.close()
        return out

    before = run_all()
    m = XC.matrix(13, 3, 3, 40, True)
    xf = pk.FeatureScorer(am40, 3, 100, global_stats=g13, transform=pk.TransformSpec(m, 3, 3))
    xf.set_features(f13, "raw")
    xf.set_utt_transforms(utt_matrices(3, 40))
    xf.score(0.1)
    after = run_all()
    xf.close()
    for name in entries:
        assert all(NC.bits_equal(a, b) for a, b in zip(before[name][0], after[name][0])), name
        assert before[name][1] == after[name][1], name                          # launch for launch
        assert before[name][2] == before[name][3] == after[name][2], name       # in_dim is feat_dim on every other batch
        b = entries[name][0]()
        assert pk.lib().pk_mi355_transform_set_utt(b._h, pk._fp(np.zeros((1, 40, 40), np.float32)), 40, 40, 1) == E_STATE, name
        assert "pk_mi355_transform_batch_create" in error_text()
        b.close()
    for o in (am40, am13, am39):
        o.close()


# ---------------------------------------------------------------- f16x3

def test_f16x3_at_40_within_the_contract_of_the_oracle():
    """Measured on an MI355X: max |err| / max(|ref|, 1) = 4.172e-07 against the contract's 1e-4 (the printed
    TRANSFORM_F16X3_MAX_ERR line; DESIGN.md section 25 records it)."""
    Dp, L, R, D = 13, 3, 3, 40
    m = XC.matrix(Dp, L, R, D, True)
    am, layers, prior = tiny(D, 2, 1, precision="f16x3")
    raw = [NC.features(T, Dp, 80 + u) for u, T in enumerate((130, 0, 33, 5))]
    mats = utt_matrices(len(raw), D)
    fs = pk.FeatureScorer(am, len(raw), sum(x.shape[0] for x in raw), transform=pk.TransformSpec(m, L, R))
    fs.set_norm(pk.NormSpec("utterance", True, True))
    fs.set_features(raw, "raw")
    fs.set_utt_transforms(mats)
    fs.calibrate()                                                              # (does not consume the matrices: the score behind it does)
    fs.score(0.1)
    nn = O.Nnet(layers)
    worst = 0.0
    for u, x in enumerate(raw):
        got = fs.fetch(u).log_prob()
        if x.shape[0] == 0:
            assert got.shape[0] == 0
            continue
        want = XC.transform(XC.transform(NC.normalize(x, "utterance", True, True)[0], m, L, R), mats[u], 0, 0)
        assert NC.bits_equal(fs.fetch_cmvn(u), want), u                          # f32, in front of the split
        ref = nn.am_compute(want, prior, 2, 1, 0.1)
        worst = max(worst, float((np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1.0)).max()))
        assert_loglik_close(got, ref)
    print("TRANSFORM_F16X3_MAX_ERR %.3e (contract 1e-4)" % worst)
    fs.close()
    am.close()


# ---------------------------------------------------------------- failure codes

def test_failure_codes():
    Dp, L, R, D = 13, 3, 3, 40
    m = XC.matrix(Dp, L, R, D, True)
    spec = pk.TransformSpec(m, L, R)
    am, _, _ = tiny(D, 2, 1)
    g = CA.stats_for(Dp)
    fe = FA.SPECS[9]
    lib = pk.lib()
    # the creation entry, in the order of its checks
    for bad, word in ((pk.TransformSpec(m, 17, 0, in_dim=13), "left_context"), (pk.TransformSpec(m, 3, 3, in_dim=12), "cols 92"),
                      (pk.TransformSpec(m, 3, 3, in_dim=0), "in_dim")):
        code, text = code_of(lambda: pk.FeatureScorer(am, 2, 100, transform=bad))
        assert code == E_INVALID and text.startswith("transform spec:") and word in text, text
    nonfinite = m.copy()
    nonfinite[7, 3] = np.inf
    code, text = code_of(lambda: pk.FeatureScorer(am, 2, 100, transform=pk.TransformSpec(nonfinite, L, R)))
    assert code == E_INVALID and "row 7, column 3" in text, text
    code, text = code_of(lambda: pk.FeatureScorer(am, 2, 100, deltas=pk.DeltaSpec(0, 2), transform=spec))       # the deltas spec comes first
    assert code == E_INVALID and text.startswith("deltas spec:"), text
    code, text = code_of(lambda: pk.FeatureScorer(am, 2, 100, deltas=pk.DeltaSpec(1, 2), transform=spec))       # 13 / 2
    assert code == E_INVALID and "13" in text and "2 blocks" in text, text
    code, text = code_of(lambda: pk.BatchScorer(am, g, 2, 16000, frontend=pk.FrontendSpec(num_mel_bins=2), transform=spec))
    assert code == E_INVALID and "num_mel_bins" in text, text
    code, text = code_of(lambda: pk.BatchScorer(am, g, 2, 16000, frontend=FA.SPECS[1], transform=spec))
    assert code == E_INVALID and "80" in text and "13" in text, text
    code, text = code_of(lambda: pk.BatchScorer(am, CA.stats_for(40), 2, 16000, frontend=fe, transform=spec))
    assert code == E_INVALID and "41 entries" in text and "14" in text, text
    code, text = code_of(lambda: pk.FeatureScorer(am, 2, 100, global_stats=CA.stats_for(40), transform=spec))
    assert code == E_INVALID and "41 entries" in text and "14" in text, text
    am39, _, _ = tiny(39, 2, 1)
    code, text = code_of(lambda: pk.FeatureScorer(am39, 2, 100, transform=spec))
    assert code == E_INVALID and "40" in text and "39" in text and "transform produces" in text, text
    code, text = code_of(lambda: pk.FeatureScorer(am39, 2, 100, transform=pk.TransformSpec(None, in_dim=40)))
    assert code == E_INVALID and "40" in text and "39" in text, text
    for utts, cap in ((0, 100), (2, 0)):
        code, text = code_of(lambda: pk.FeatureScorer(am, utts, cap, transform=spec))
        assert code == E_INVALID and "capacity" in text
    st = spec.struct()
    assert not lib.pk_mi355_transform_batch_create(am.handle, None, None, None, None, 0, 2, 100) and "null" in error_text()
    assert not lib.pk_mi355_transform_batch_create(am.handle, C.byref(st), None, C.byref(fe.struct()), None, 0, 2, 16000) and "null" in error_text()
    half, _, _ = tiny(39, 2, 1, precision="f16x3")
    code, text = code_of(lambda: pk.FeatureScorer(half, 2, 100, transform=pk.TransformSpec(XC.matrix(13, 3, 3, 39, True), 3, 3)))
    assert code == E_INVALID and "multiple of 8" in text and "39" in text
    half.close()
    am39.close()
    # the feature entries: RAW at Db, NORMALIZED at feat_dim
    fs = pk.FeatureScorer(am, 3, 100, transform=spec)
    raw = [NC.features(T, Dp, 20 + u) for u, T in enumerate((9, 0, 70))]
    code, text = code_of(lambda: fs.set_features(raw, "raw"))                  # no statistics, the sliding rule
    assert code == E_INVALID and "statistics" in text and "14" in text and "pk_mi355_transform_batch_create" in text, text
    fs.set_norm(pk.NormSpec("none"))
    m40 = pk._as_matrix(np.zeros((4, 40), np.float32))
    assert lib.pk_mi355_features_set(fs._h, C.byref(m40), 1, 1) == E_INVALID and "40 rows" in error_text() and "13" in error_text()
    m13 = pk._as_matrix(np.zeros((4, 13), np.float32))
    assert lib.pk_mi355_features_set(fs._h, C.byref(m13), 1, 0) == E_INVALID and "13 rows" in error_text() and "40" in error_text()
    assert code_of(lambda: fs.set_features([np.zeros((101, 13), np.float32)], "raw"))[0] == E_INVALID    # capacity
    # the per-utterance matrices
    good = utt_matrices(3, D)
    code, text = code_of(lambda: fs.set_utt_transforms([np.zeros((39, 40), np.float32)] * 3))
    assert code == E_INVALID and "39 rows" in text and "40" in text, text
    code, text = code_of(lambda: fs.set_utt_transforms([np.zeros((40, 42), np.float32)] * 3))
    assert code == E_INVALID and "42 columns" in text and "40" in text and "41" in text, text
    code, text = code_of(lambda: fs.set_utt_transforms(good * 2))
    assert code == E_INVALID and "too many utterances" in text, text
    spoiled = [g_.copy() for g_ in good]
    spoiled[2][4, 40] = np.nan
    code, text = code_of(lambda: fs.set_utt_transforms(spoiled))
    assert code == E_INVALID and "utterance 2" in text and "not finite" in text, text
    assert lib.pk_mi355_transform_set_utt(fs._h, None, 40, 41, 3) == E_INVALID and "null" in error_text()
    fs.set_features(raw, "raw")
    assert code_of(lambda: fs.fetch_cmvn(0))[0] == E_STATE                      # not scored
    fs.set_utt_transforms(good[:2])
    assert score_code(fs) == E_STATE and "2 utterances" in error_text() and "has 3" in error_text()
    fs.set_norm(pk.NormSpec())                                                  # back to sliding with raw rows set: nothing to slide with
    assert score_code(fs) == E_STATE and "statistics" in error_text()
    # every utterance frameless: nothing launched
    fs.set_norm(pk.NormSpec("utterance"))
    fs.set_features([raw[1], raw[1]], "raw")
    fs.set_utt_transforms(good[:2])
    fs.score(0.1)
    assert NC.bits_equal(fs.norm_stats(1), np.zeros((2, Dp + 1))) and fs.fetch_cmvn(1).shape == (0, 40)
    # a features-only transform batch takes no audio
    assert code_of(lambda: fs.set_waves([np.zeros(1600, np.float32)], rates=[16000]))[0] == E_STATE
    fs.close()
    am.close()
