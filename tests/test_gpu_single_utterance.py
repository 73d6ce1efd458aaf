"""pk_decodable_init and pk_mi355_am_calibrate are calls on a one-utterance features batch that the model owns (DESIGN.md
section 13).  What that must not change, where a host can see it: every owner of the model's mutex interleaved on one
model object returns the bits of a fresh model, whatever the owned buffers held and however they had to grow; a
calibration leaves the same exponents whichever scorer ran its passes; the rows handed to the layer stack end at the last
frame (the fused-tail row counts with their one-row last tile still mean one row); the failure texts are the ones the
entries had before."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth

import isolation_cases as IC
import tail_cases as TC

FRAMES = (0, 1, 3, 4, 5, 127, 128, 129, 4095, 4096, 4097, 8193)
# (entry, frames): pk.Decodable at every count, the other owners of am->mu between them
CALLS = ([("decodable", T) for T in FRAMES] + [("process", T) for T in (0, 1, 5, 129, 4097)] +
         [("propagate", T) for T in (0, 3, 128, 4096)] + [("calibrate", T) for T in (4, 127, 4095)])
ORDER = [CALLS[i] for i in np.random.default_rng(0x51A6).permutation(len(CALLS))]
_decodable_T = [T for op, T in ORDER if op == "decodable"]
assert sorted(_decodable_T) == list(FRAMES) and _decodable_T != sorted(_decodable_T) and _decodable_T != sorted(_decodable_T, reverse=True)
# the owned batch regrows (a longer utterance after a shorter one, past 4 096 frames), lays out a shorter one after a
# longer one, and meets an empty call
assert any(a < b and b > 4096 for a, b in zip(_decodable_T, _decodable_T[1:])) and any(a > b > 0 for a, b in zip(_decodable_T, _decodable_T[1:]))


def wave(T):
    return IC.healthy(7000 + T, T) if T > 0 else np.zeros(240, np.float32)


def call(am, op, T, L, R):
    """One entry on `am` -> what it returns (calibrate: the exponents it leaves)."""
    feats = IC.single_features(T, seed=3)
    if op == "decodable":
        d = pk.Decodable(am, 0.1, feats)
        out = d.log_prob()
        d.destroy()
        return out
    if op == "process":
        d = pk.process_acoustic(am, synth.global_cmvn_stats(), wave(T), 0.1)
        out = d.log_prob()
        d.destroy()
        return out
    if op == "propagate":
        return am.propagate(np.random.default_rng([0x9A, T]).standard_normal((T, 40 * (L + R + 1))).astype(np.float32))
    am.calibrate(feats)
    return np.concatenate(am.exponents())


@pytest.mark.parametrize("mode", ["f32", "f32_reference_softmax", "f16x3"])
def test_every_owner_of_the_model_mutex_interleaved_returns_a_fresh_models_bits(mode):
    layers, prior, L, R = IC.single_stack("softmax")
    precision = "f16x3" if mode == "f16x3" else "f32"

    def model():
        am = pk.AcousticModel(layers, prior, L, R, precision=precision)
        return am.set_softmax("reference") if mode == "f32_reference_softmax" else am

    am = model()
    if mode == "f16x3":
        am.calibrate(IC.single_features(600, seed=2))
    for i, (op, T) in enumerate(ORDER):
        if op == "calibrate" and mode != "f16x3":
            continue
        fresh = model()
        if mode == "f16x3":
            fresh.set_input_exponents(am.exponents()[1])
        want = call(fresh, op, T, L, R)
        fresh.close()
        got = call(am, op, T, L, R)
        assert got.shape == want.shape and (op == "calibrate" or got.shape[0] == T), (mode, i, op, T, got.shape, want.shape)
        assert IC.same_bits(got, want) if op != "calibrate" else np.array_equal(got, want), (mode, i, op, T)
    am.close()


@pytest.mark.parametrize("stack", IC.SINGLE_STACKS)
def test_calibration_does_not_depend_on_the_route(stack):
    """pk_mi355_am_calibrate (which holds am->mu while the owned batch runs its passes, and returns) and
    pk_mi355_batch_calibrate on a FeatureScorer fed the same features: the same integers."""
    layers, prior, L, R = IC.single_stack(stack)
    feats = IC.single_features(600, seed=2)
    a = pk.AcousticModel(layers, prior, L, R, precision="f16x3").calibrate(feats)
    b = pk.AcousticModel(layers, prior, L, R, precision="f16x3")
    fs = pk.FeatureScorer(b, 1, feats.shape[0])
    fs.set_features([feats])
    fs.calibrate()
    for x, y in zip(a.exponents(), b.exponents()):
        assert x.dtype == np.int32 and np.array_equal(x, y), (stack, a.exponents(), b.exponents())
    fs.close(); a.close(); b.close()


@pytest.mark.parametrize("n", [1024, 3072])
def test_rows_end_at_the_last_frame_one_row_in_the_last_tile(n, monkeypatch):
    """The designed model of test_gpu_tail_edges.py::test_fused_tail, ONE row in the last 128-row tile (and that tile
    full): the predicted bits.  A call that handed the layer stack RoundUp(T, 4) rows would put four rows there.
    3 072 columns: tail_cases.fused_row_counts, the fewest row tiles at which the last layer's launch finishes its rows
    itself.  1 024 columns: eight column tiles fuse from 48 row tiles on, more than one 4 096-row pass holds
    (fused_row_counts(1024) is empty, see test_gpu_tail_edges.py), so the same two shapes of the last tile are taken at the
    END of a pass, 3 969 and 4 096 rows, on the route the documented rules give there."""
    rows = TC.fused_row_counts(n) or [TC.SINGLE_PASS_ROWS - TC.TILE + 1, TC.SINGLE_PASS_ROWS]
    assert (n == 1024) == (not TC.fused_row_counts(n)) and rows[0] % TC.TILE == 1 and rows[1] % TC.TILE == 0
    for k, v in {"PK_MI355_FUSED_TAIL32": "1", "PK_MI355_FUSED_TAIL_MIN_TILES": "384"}.items():
        monkeypatch.setenv(k, v)
    case = TC.main_case(n)
    am = pk.AcousticModel(TC.layers(case, identity_first=True), TC.prior(n, "varied"), 0, 0)
    worst = 0.0
    for r in rows:
        assert (TC.fused_route(r, n) == "wave") == (n == 1024)
        d = pk.Decodable(am, 0.1, TC.features(case, r))
        got = d.log_prob()
        d.destroy()
        assert got.shape == (r, n)
        worst = max(worst, TC.check(case, got, 0.1, "varied", "wave", "%s, %d rows" % (TC.fused_route(r, n), r)))
    am.close()
    print("SINGLE_UTTERANCE_LAST_TILE_RATIO n=%d %.4f" % (n, worst))
    assert worst <= 1.0


def test_rows_of_a_two_utterance_batch_keep_their_places():
    """T = (5, 6), L + R = 4 >= 3 (compact rows): utterance 1 starts at row 8 of the log-likelihood rows and of the
    page-locked arena, although the rows now end at 8 + 6 = 14 and not at 16."""
    layers, prior, L, R = IC.single_stack("softmax")
    N = len(prior)
    am = pk.AcousticModel(layers, prior, L, R)
    feats = [IC.single_features(5, seed=4), IC.single_features(6, seed=5)]
    fs = pk.FeatureScorer(am, 2, 11)
    fs.set_features(feats)
    fs.score(0.1)
    assert fs.total_frames() == 11 and [fs.num_frames(u) for u in range(2)] == [5, 6]
    assert fs.loglik_device(1) - fs.loglik_device(0) == 8 * N * 4
    views = fs.fetch_all()
    base = C.cast(views[0]._d.log_prob.data, C.c_void_p).value
    assert C.cast(views[1]._d.log_prob.data, C.c_void_p).value - base == 8 * N * 4
    arena = np.ctypeslib.as_array(views[0]._d.log_prob.data, shape=(14, N))
    for u, (row0, f) in enumerate(zip((0, 8), feats)):
        d = pk.Decodable(am, 0.1, f)
        want = d.log_prob()
        d.destroy()
        assert IC.same_bits(arena[row0:row0 + f.shape[0]], want) and IC.same_bits(views[u].log_prob(), want), u
        assert IC.same_bits(fs.fetch(u).log_prob(), want), u
    for v in views:
        v.destroy()
    fs.close(); am.close()


# The texts of pk_decodable_init and pk_mi355_am_calibrate before they became calls on the owned batch, character for
# character (the entries answer before the batch is touched).
ROWS_INIT = "features have %d rows, the model expects %d"
ROWS_CALIBRATE = "calibration features have %d rows, the model expects %d"
MULTIPLE_OF_8 = "f16x3 / f16 precision needs a feature dimension that is a multiple of 8 (got %d)"


def last_error():
    return pk.lib().pk_mi355_last_error().decode()


def test_failure_texts_of_the_feature_entries():
    layers, prior, L, R = IC.single_stack("softmax")
    am = pk.AcousticModel(layers, prior, L, R, precision="f16x3")
    wrong = np.zeros((7, 39), np.float32)
    with pytest.raises(pk.PkError):
        pk.Decodable(am, 0.1, wrong)
    assert last_error() == ROWS_INIT % (39, 40)
    with pytest.raises(pk.PkError):
        am.calibrate(wrong)
    assert last_error() == ROWS_CALIBRATE % (39, 40)
    am.close()
    rng = np.random.default_rng(12)
    w, b = rng.standard_normal((16, 12)).astype(np.float32), np.zeros(16, np.float32)
    am12 = pk.AcousticModel([("linear", w, b), ("softmax",)], np.full(16, 1 / 16, np.float32), 0, 0, precision="f16x3")
    x = np.ones((7, 12), np.float32)
    with pytest.raises(pk.PkError):
        pk.Decodable(am12, 0.1, x)
    assert last_error() == MULTIPLE_OF_8 % 12
    with pytest.raises(pk.PkError):
        am12.calibrate(x)
    assert last_error() == MULTIPLE_OF_8 % 12
    am12.close()
