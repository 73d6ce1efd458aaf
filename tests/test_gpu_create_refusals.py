"""GPU: the refusals of the twelve create entries that read a finalized model, each with the text the
entry has always given, written out here from the format strings of csrc/pk_score.h and csrc/capi_batch.hip; the meetings
of two faults that the one check order changed behind a finalized model; and what a recognizer hands its scorer.  Tiny
synthetic models of 40 and of 39 = 13 x 3 features, two utterances or slots, 100 frames or 1600 samples.  Nothing is
scored.  (The refusals said without a device: tests/test_create_refusals_host.py.)"""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import pocketkaldi_amd as pk

import frontend_any_cases as FA
import refmodel_files as RF
import transform_cases as TC
from refmodel_text import load_text_model
from test_gpu_cmvn_any import tiny
from test_gpu_frontend_recognizer import DIR
from test_gpu_recognize_deltas import model_layers

pytestmark = pytest.mark.gpu

E_INVALID = -1
L, R = 2, 1
UNITS, FRAMES, SAMPLES = 2, 100, 1600
f32p = C.POINTER(C.c_float)
FE13, FE40, FE80 = FA.SPECS[9], FA.SPECS[0], FA.SPECS[1]
D1, D2 = pk.DeltaSpec(1, 2), pk.DeltaSpec(2, 2)                                  # 2 and 3 blocks
X13_40 = pk.TransformSpec(TC.matrix(13, 3, 3, 40, True), 3, 3)
X13_39 = pk.TransformSpec(TC.matrix(13, 3, 3, 39, True), 3, 3)
BAD_FE = FA.S(bins=129)
BAD_FE_WORDS = "front-end spec: num_mel_bins 129 is outside 3 .. 128"
KINDS = ("batch", "stream")


@pytest.fixture(scope="module")
def models():
    am40, am39 = tiny(40, L, R)[0], tiny(39, L, R)[0]
    yield {40: am40, 39: am39}
    am40.close()
    am39.close()


def refusal(kind, entry, am, *args):
    """(code, text) of pk_mi355_<entry>_<kind>_create(am, *args); specs are given as objects, statistics as a length (or
    None), and the two capacities last."""
    keep, out = [], []
    for a in args:
        if hasattr(a, "struct"):
            keep.append(a.struct())
            out.append(C.byref(keep[-1]))
        elif isinstance(a, tuple):                       # ("stats", n) -> the pointer and the length; ("stats41",) -> the pointer
            keep.append(np.zeros(a[1] if len(a) > 1 else 41, np.float32))
            out += [keep[-1].ctypes.data_as(f32p)] + ([a[1]] if len(a) > 1 else [])
        else:
            out.append(a)
    name = "pk_mi355_%s_create" % kind if entry == "" else ("pk_mi355_features_%s_create_stats" % kind if entry == "features_stats"
                                                             else "pk_mi355_%s_%s_create" % (entry, kind))
    lib = pk.lib()
    handle = getattr(lib, name)(am.handle, *out)
    assert not handle, (name, args)
    return lib.pk_mi355_last_error_code(), lib.pk_mi355_last_error().decode()


def stats(n):
    return ("stats", n)


STATS41, NO_STATS = ("stats41",), (None, 0)


@pytest.mark.parametrize("kind", KINDS)
def test_dimension_refusals_word_for_word(models, kind):
    am40, am39 = models[40], models[39]
    inv = lambda text: (E_INVALID, text)
    # deltas whose blocks do not divide: the model's features, the transform's in_dim
    assert refusal(kind, "deltas", am40, D2, None, *NO_STATS, UNITS, FRAMES) == inv(
        "deltas of order 2 make 3 blocks, which does not divide the model's 40-dim features")
    assert refusal(kind, "deltas", am40, D2, FE13, stats(14), UNITS, SAMPLES) == inv(
        "deltas of order 2 make 3 blocks, which does not divide the model's 40-dim features")
    assert refusal(kind, "transform", am40, X13_40, D1, None, *NO_STATS, UNITS, FRAMES) == inv(
        "deltas of order 1 make 2 blocks, which does not divide the transform's in_dim 13")
    # a front-end of another dimension, in its three wordings and the transform's own
    assert refusal(kind, "", am39, STATS41, UNITS, SAMPLES) == inv("the front-end produces 40-dim features, the model expects 39")
    assert refusal(kind, "frontend", am40, FE80, stats(81), UNITS, SAMPLES) == inv("the front-end spec produces 80-dim features, the model expects 40")
    assert refusal(kind, "deltas", am39, D2, FE80, stats(81), UNITS, SAMPLES) == inv(
        "the front-end spec produces 80-dim features, the model's 39 with deltas of order 2 need 13")
    assert refusal(kind, "transform", am40, X13_40, None, FE80, stats(81), UNITS, SAMPLES) == inv(
        "the front-end spec produces 80-dim features, the transform's in_dim 13 with 1 delta blocks needs 13")
    # statistics of another length, at the model's dimension and at a base dimension
    assert refusal(kind, "features_stats", am40, stats(14), UNITS, FRAMES) == inv(
        "the CMVN statistics have 14 entries, a 40-dim model needs 41 (the sums, then the count)")
    assert refusal(kind, "frontend", am40, FE40, stats(14), UNITS, SAMPLES) == inv(
        "the CMVN statistics have 14 entries, a 40-dim model needs 41 (the sums, then the count)")
    for front, cap in ((None, FRAMES), (FE13, SAMPLES)):
        assert refusal(kind, "deltas", am39, D2, front, stats(41), UNITS, cap) == inv(
            "the CMVN statistics have 41 entries, 13-dim base features need 14 (the sums, then the count)")
        assert refusal(kind, "transform", am40, X13_40, None, front, stats(41), UNITS, cap) == inv(
            "the CMVN statistics have 41 entries, 13-dim base features need 14 (the sums, then the count)")
    # a transform of another output dimension
    assert refusal(kind, "transform", am40, X13_39, None, None, *NO_STATS, UNITS, FRAMES) == inv(
        "the transform produces 39-dim features, the model expects 40")
    # 41 statistics for a model that is not 40-dim
    assert refusal(kind, "features", am39, STATS41, UNITS, FRAMES) == inv("the CMVN statistics are for 40-dim features, the model expects 39")


def good_calls(am40, am39):
    """Every entry with arguments it accepts, the two capacities left out: (entry, model, arguments, capacity in samples)."""
    return (("", am40, (STATS41,), True), ("features", am40, (STATS41,), False), ("features", am39, (None,), False),
            ("features_stats", am39, (stats(40),), False), ("frontend", am40, (FE40, stats(41)), True),
            ("deltas", am39, (D2, FE13, stats(14)), True), ("deltas", am39, (D2, None) + NO_STATS, False),
            ("transform", am40, (X13_40, None, FE13, stats(14)), True), ("transform", am40, (X13_40, None, None) + NO_STATS, False),
            ("transform", am40, (pk.TransformSpec(TC.matrix(39, 0, 0, 40, False), 0, 0, in_dim=39), D2, None, stats(14)), False))


@pytest.mark.parametrize("kind", KINDS)
def test_capacity_refusals(models, kind):
    am40, am39 = models[40], models[39]
    words = (E_INVALID, "bad %s capacity" % kind)
    for entry, am, args, audio in good_calls(am40, am39):
        cap = SAMPLES if audio else FRAMES
        for units, capacity in ((0, cap), (-1, cap), (UNITS, 0), (UNITS, -1)):
            assert refusal(kind, entry, am, *args, units, capacity) == words, (entry, units, capacity)
        if kind == "stream":            # a step's staging is indexed in 32 bits: 2^30 floats, a pushed frame the widest of model and base
            widest = 1 if audio else max(am.feat_dim(), 13 if entry in ("deltas", "transform") else 0)
            assert refusal(kind, entry, am, *args, UNITS, (1 << 30) // widest + 1) == words, entry
    # audio without statistics: the two entries that can be asked for it have always named it so
    assert refusal(kind, "", am40, None, UNITS, SAMPLES) == words


def test_the_meetings_of_two_faults_behind_a_finalized_model(models):
    """DESIGN.md section 28 lists them.  The batch entries say what they always said."""
    am40, am39 = models[40], models[39]
    # 3. 41 statistics for a 39-dim model and a refused capacity: the capacity (it was the statistics on the live entry)
    for capacity in (0, -1, (1 << 30) // 39 + 1):
        assert refusal("stream", "features", am39, STATS41, UNITS, capacity) == (E_INVALID, "bad stream capacity")
    assert refusal("stream", "features", am39, STATS41, 0, FRAMES) == (E_INVALID, "bad stream capacity")
    assert refusal("batch", "features", am39, STATS41, UNITS, 0) == (E_INVALID, "bad batch capacity")
    # 4. a bad front-end spec and deltas whose blocks do not divide: the spec's words on the live entries (it was the
    #    blocks'), the blocks' on the batch entries
    assert refusal("stream", "deltas", am40, D2, BAD_FE, stats(14), UNITS, SAMPLES) == (E_INVALID, BAD_FE_WORDS)
    assert refusal("stream", "transform", am40, X13_40, D1, BAD_FE, stats(14), UNITS, SAMPLES) == (E_INVALID, BAD_FE_WORDS)
    assert refusal("batch", "deltas", am40, D2, BAD_FE, stats(14), UNITS, SAMPLES) == (
        E_INVALID, "deltas of order 2 make 3 blocks, which does not divide the model's 40-dim features")
    assert refusal("batch", "transform", am40, X13_40, D1, BAD_FE, stats(14), UNITS, SAMPLES) == (
        E_INVALID, "deltas of order 1 make 2 blocks, which does not divide the transform's in_dim 13")
    # and a bad front-end spec alone, behind a finalized model: the spec's words everywhere
    for kind in KINDS:
        assert refusal(kind, "frontend", am40, BAD_FE, stats(41), UNITS, SAMPLES) == (E_INVALID, BAD_FE_WORDS)
        assert refusal(kind, "deltas", am39, D2, BAD_FE, stats(14), UNITS, SAMPLES) == (E_INVALID, BAD_FE_WORDS)
        assert refusal(kind, "transform", am40, X13_40, None, BAD_FE, stats(14), UNITS, SAMPLES) == (E_INVALID, BAD_FE_WORDS)


def words_of(call):
    with pytest.raises(pk.PkError) as e:
        call()
    return str(e.value)


def batch_shape(bs):
    """Dimensions, and the two capacities: the refusal of one utterance too many names the first; SAMPLES samples are
    taken and one more is refused."""
    wave = np.zeros(400, np.float32)
    bs.set_waves([np.zeros(SAMPLES, np.float32)])
    return (bs.feat_dim(), bs.base_dim(), bs.in_dim(), words_of(lambda: bs.set_waves([wave] * (UNITS + 1))),
            words_of(lambda: bs.set_waves([np.zeros(SAMPLES + 1, np.float32)])))


def stream_shape(sc):
    """Dimensions, and the two capacities as the refusals of one slot and one sample too many name them."""
    over = words_of(lambda: sc.open(UNITS))
    sc.open(0)
    return (sc.feat_dim(), sc.base_dim(), sc.in_dim(), over, words_of(lambda: sc.push(0, np.zeros(SAMPLES + 1, np.float32))))


@pytest.mark.parametrize("which", ["plain", "frontend", "deltas", "transform"])
def test_a_recognizer_hands_its_scorer_what_the_public_entry_would(which, tmp_path):
    D = {"plain": 40, "frontend": 13, "deltas": 39, "transform": 40}[which]
    Db = 40 if which == "plain" else 13
    g = np.concatenate([np.full(Db, 0.5 * 2500.0), [2500.0]]).astype(np.float32)
    layers, prior = model_layers(D, 31)
    tid2pdf = load_text_model()[4]
    conf = RF.write_model(tmp_path, layers, prior, L, R, tid2pdf=tid2pdf, cmvn_stats=g)
    for f in ("wordloop.fst", "wordloop_words.bin"):
        shutil.copy(os.path.join(DIR, f), str(tmp_path / f))
    with open(conf, "a") as f:
        f.write("fst = wordloop.fst\nsymbol_table = wordloop_words.bin\n")
    fe = None if which == "plain" else FE13
    deltas = D2 if which == "deltas" else None
    xform = X13_40 if which == "transform" else None
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    direct = pk.BatchScorer(am, g, UNITS, SAMPLES, frontend=fe, deltas=deltas, transform=xform)
    rec = pk.Recognizer(conf, max_utts=UNITS, max_total_samples=SAMPLES, frontend=fe, deltas=deltas, transform=xform)
    want = batch_shape(direct)
    assert want[:3] == (D, Db, 39 if which == "deltas" else 13 if which == "transform" else D)
    assert want[3:] == ("too many utterances (3 > 2)", "too many samples")
    assert batch_shape(rec.batch) == want
    rec.close()
    direct.close()
    if xform is None:
        live = pk.OnlineScorer(am, g, UNITS, SAMPLES, frontend=fe, deltas=deltas)
        online = pk.OnlineRecognizer(conf, max_streams=UNITS, max_step_samples=SAMPLES, frontend=fe, deltas=deltas)
    else:
        live = pk.OnlineScorer.with_transform(am, g, UNITS, SAMPLES, xform, frontend=fe)
        online = pk.OnlineRecognizer.with_transform(conf, xform, max_streams=UNITS, max_step_samples=SAMPLES, frontend=fe)
    want = stream_shape(live)
    assert want[:3] == (D, Db, 39 if which == "deltas" else 13 if which == "transform" else D)
    assert want[3:] == ("slot 2 out of range [0, 2)", "push of 1601 samples exceeds the step capacity (0 pending of 1600)")
    assert stream_shape(online.scorer) == want
    online.destroy()
    live.destroy()
    am.close()
