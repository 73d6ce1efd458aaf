"""CPU-only: feature transforms on the online objects -- the numpy restatement of the live rule
(tests/stream_transform_cases.py) held to the batch rule (tests/transform_cases.py) at every chunking; three wrong
variants of it shown to change outputs; the new entries' names in header, export list, binding and C++ header; the
refusals of pk_mi355_transform_stream_create, pk_mi355_stream_transform_set_slot and
pk_mi355_transform_online_recognizer_load that are said without a device; with_transform's argument errors.  The
refusals that read a finalized model, which needs a device, are in tests/test_gpu_stream_transforms.py, with the texts
of the batch entry."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import frontend_any_cases as FA
import stream_transform_cases as ST
import transform_cases as TC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
NEW_ENTRIES = ["pk_mi355_transform_stream_create", "pk_mi355_stream_in_dim", "pk_mi355_stream_transform_set_slot",
               "pk_mi355_transform_online_recognizer_load"]
f32p = C.POINTER(C.c_float)
# (in_dim, Lt, Rt, rows, affine)
SPECS = ((1, 0, 0, 1, True), (13, 3, 3, 40, True), (40, 0, 4, 40, False), (5, 5, 0, 7, True), (3, 8, 8, 65, False))


def last():
    return pk.lib().pk_mi355_last_error_code(), pk.lib().pk_mi355_last_error().decode()


def fp(a):
    return a.ctypes.data_as(f32p)


def model(precision=0):
    am = pk.lib().pk_mi355_am_create()
    assert am and pk.lib().pk_mi355_am_set_precision(am, precision) == 0
    return am


def closings(T, how, rng):
    """(chunks, close_delay): closed with the last push, and closed later."""
    return [(ST.chunks_of(T, how, rng), 0), (ST.chunks_of(T, how, rng), 2)]


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: "%dx(%d,%d)->%d%s" % (s[0], s[1], s[2], s[3], "a" if s[4] else "l"))
def test_live_rule_is_the_batch_rule_at_every_chunking(spec):
    Dp, L, R, rows, affine = spec
    m = TC.matrix(Dp, L, R, rows, affine)
    slot_m = TC.matrix(rows, 0, 0, rows, True, seed=9)
    rng = np.random.default_rng(21)
    for T in sorted({0, 1, 2, R, R + 1, L + R, L + R + 1, 2 * (L + R) + 1, 23}):
        x = TC.normal(T, Dp, seed=100 + T)
        want, want_slot = ST.batch_rows(x, m, L, R), ST.batch_rows(x, m, L, R, slot_m)
        for how in ST.CHUNKINGS:
            for chunks, delay in closings(T, how, rng):
                got, made = ST.stream_transform(x, m, L, R, chunks, delay)
                assert TC.bits_equal(got, want), (T, how, delay)
                steps = (list(chunks) or [0]) + [0] * delay
                assert sum(made) == T and len(made) == len(steps)
                pushed, final = np.cumsum(steps), np.cumsum(made)
                for k in range(len(steps) - 1):        # an open slot holds exactly Rt input frames back
                    assert final[k] == max(pushed[k] - R, 0), (T, how, delay, k)
        got, _ = ST.live_rows(x, m, L, R, ST.chunks_of(T, 7, rng), 1, slot_m)
        assert TC.bits_equal(got, want_slot), T


def test_matrixless_rows_pass_as_bits():
    x = TC.normal(19, 6, seed=4)
    x[3, 1] = -0.0
    x[5, 2] = np.inf
    x.view(np.uint32)[7, 0] = 0x7FC12345                # a NaN with a payload
    x.view(np.uint32)[8, 5] = 0xFFA00001                # a signalling one, negative
    rng = np.random.default_rng(2)
    for how in ST.CHUNKINGS:
        got, _ = ST.stream_transform(x, None, 0, 0, ST.chunks_of(19, how, rng), 1)
        assert got.tobytes() == x.tobytes(), how


@pytest.mark.parametrize("spec", ST.VARIANT_SPECS, ids=lambda s: "%dx(%d,%d)->%d" % s[:4])
@pytest.mark.parametrize("variant", ST.VARIANTS)
def test_wrong_variants_change_outputs(spec, variant):
    """A ring of C - 1 frames, the upper clamp applied while the slot is open, the ring read at the parity just written:
    each changes outputs at 7 frames a push.  (At C = 0 none of them can show: there is no ring and nothing is held back.)"""
    Dp, L, R, rows, affine = spec
    m = TC.matrix(Dp, L, R, rows, affine)
    x = TC.normal(33, Dp, seed=8)
    want = TC.transform(x, m, L, R)
    chunks = ST.chunks_of(33, 7, None)
    good, _ = ST.stream_transform(x, m, L, R, chunks, 1)
    assert TC.bits_equal(good, want)
    with np.errstate(all="ignore"):
        bad, _ = ST.stream_transform(x, m, L, R, chunks, 1, variant=variant)
    assert bad.shape == want.shape
    assert TC.outputs_differing(bad, want) > 0, variant


def test_accounting_and_lookahead():
    assert ST.advance(10, 0, 0, 3, 2, False) == (7, 5)
    assert ST.advance(10, 7, 5, 3, 2, True) == (10, 10)
    assert ST.advance(2, 0, 0, 3, 2, False) == (0, 0)
    assert ST.advance(0, 0, 0, 3, 2, True) == (0, 0)
    assert ST.advance(10, 9, 8, 3, 2, False) == (9, 8)       # never backwards
    assert ST.lookahead(4, 3, 5) == 12


def test_new_entries_in_header_map_exports_and_binding():
    header = open(os.path.join(REPO, "include", "pk_mi355.h")).read()
    vmap = open(os.path.join(REPO, "pocketkaldi_amd", "csrc", "libpk_mi355.map")).read()
    L = pk.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pk.EXPORTS and hasattr(L, name), name
    assert "pk_mi355_*;" in vmap
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    for name in NEW_ENTRIES:
        assert re.search(r" T %s$" % name, dyn, re.M), name
    hpp = open(os.path.join(REPO, "include", "pocketkaldi_amd.hpp")).read()
    for name in NEW_ENTRIES:
        assert name in hpp, name
    assert "take no transform yet" not in header
    assert L.pk_mi355_transform_stream_create.restype is C.c_void_p and L.pk_mi355_transform_online_recognizer_load.restype is C.c_void_p
    for cls in (pk.OnlineScorer, pk.OnlineFeatureScorer, pk.OnlineRecognizer):
        assert callable(getattr(cls, "with_transform"))
    assert callable(pk.OnlineScorer.set_slot_transform) and callable(pk.OnlineScorer.in_dim)


def test_stream_create_refusals_without_a_device():
    L = pk.lib()
    m = TC.matrix(13, 3, 3, 40, True)
    good = pk.TransformSpec(m, 3, 3).struct()
    dl = pk.DeltaSpec(2, 2).struct()
    fe, g = FA.SPECS[9].struct(), np.zeros(14, np.float32)
    assert not L.pk_mi355_transform_stream_create(None, C.byref(good), None, None, None, 0, 2, 100)
    assert last() == (E_STATE, "model not finalized")                           # the batch entry's words for a null model
    am = model()
    try:
        assert not L.pk_mi355_transform_stream_create(am, None, None, None, None, 0, 2, 100)
        assert last() == (E_INVALID, "null argument")                          # a null spec
        assert not L.pk_mi355_transform_stream_create(am, C.byref(good), None, C.byref(fe), None, 0, 2, 1600)
        assert last() == (E_INVALID, "null argument")                          # a front-end without statistics
        for order, window, field in ((4, 2, "order"), (2, 0, "window")):
            st = pk.DeltaSpec(order, window).struct()
            assert L.pk_mi355_deltas_check(C.byref(st)) == E_INVALID
            words = last()[1]
            assert words.startswith("deltas spec:") and field in words
            assert not L.pk_mi355_transform_stream_create(am, C.byref(good), C.byref(st), C.byref(fe), fp(g), 14, 2, 1600)
            assert last() == (E_INVALID, words)
        nonfinite = m.copy()
        nonfinite[2, 5] = np.inf
        for spec, field in ((pk.TransformSpec(m, 17, 0, in_dim=13), "left_context"), (pk.TransformSpec(m, 0, 17, in_dim=13), "right_context"),
                            (pk.TransformSpec(m, 9, 9, in_dim=13), "above"), (pk.TransformSpec(m, 3, 3, in_dim=600), "in_dim"),
                            (pk.TransformSpec(m, 3, 3, in_dim=12), "cols"), (pk.TransformSpec(None, 1, 0, in_dim=13), "null matrix"),
                            (pk.TransformSpec(nonfinite, 3, 3), "row 2, column 5")):
            st = spec.struct()
            assert L.pk_mi355_transform_check(C.byref(st)) == E_INVALID
            words = last()[1]
            assert words.startswith("transform spec:") and field in words, words
            assert not L.pk_mi355_transform_stream_create(am, C.byref(st), C.byref(dl), C.byref(fe), fp(g), 14, 2, 1600)
            assert last() == (E_INVALID, words)
            assert not L.pk_mi355_transform_stream_create(am, C.byref(st), None, None, None, 0, 2, 100)
            assert last() == (E_INVALID, words)
        assert not L.pk_mi355_transform_stream_create(am, C.byref(good), None, C.byref(fe), fp(g), 14, 2, 1600)      # f32, not finalized
        assert last() == (E_STATE, "model not finalized")
        assert not L.pk_mi355_transform_stream_create(am, C.byref(good), None, None, None, 0, 2, 100)
        assert last() == (E_STATE, "model not finalized")
    finally:
        L.pk_mi355_am_destroy(am)
    for precision in (1, 2):                     # PK_MI355_PRECISION_F16X3, _F16: refused, as on every online scorer
        am = model(precision)
        try:
            assert not L.pk_mi355_transform_stream_create(am, C.byref(good), None, C.byref(fe), fp(g), 14, 2, 1600)
            code, words = last()
            assert code == E_INVALID and "f32" in words
        finally:
            L.pk_mi355_am_destroy(am)
    assert L.pk_mi355_stream_in_dim(None) == E_INVALID and "null stream" in last()[1]
    assert L.pk_mi355_stream_transform_set_slot(None, 0, fp(m), 40, 40) == E_INVALID and "null stream" in last()[1]


def test_with_transform_argument_errors():
    am = pk.AcousticModel.__new__(pk.AcousticModel)
    am._h = model(1)
    m = TC.matrix(13, 3, 3, 40, True)
    spec = pk.TransformSpec(m, 3, 3)
    try:
        for make in (lambda t, **kw: pk.OnlineFeatureScorer.with_transform(am, 2, 100, t, **kw),
                     lambda t, **kw: pk.OnlineScorer.with_transform(am, np.zeros(14, np.float32), 2, 1600, t, frontend=FA.SPECS[9], **kw)):
            with pytest.raises(TypeError, match="TransformSpec"):
                make(None)
            with pytest.raises(TypeError, match="TransformSpec"):
                make(m)
            with pytest.raises(TypeError, match="DeltaSpec"):
                make(spec, deltas=(2, 2))
            with pytest.raises(pk.PkCodeError) as e:
                make(spec)
            assert e.value.code == E_INVALID and "f32" in str(e.value)
            with pytest.raises(pk.PkCodeError) as e:
                make(pk.TransformSpec(m, 9, 9, in_dim=13))
            assert e.value.code == E_INVALID and "above" in str(e.value)
            with pytest.raises(pk.PkCodeError) as e:
                make(spec, deltas=pk.DeltaSpec(4, 2))
            assert e.value.code == E_INVALID and "order" in str(e.value)
        with pytest.raises(TypeError, match="FrontendSpec"):
            pk.OnlineScorer.with_transform(am, np.zeros(14, np.float32), 2, 1600, spec, frontend="mfcc")
    finally:
        am.close()
    # the constructors themselves keep refusing the keyword (tests/test_transform_host.py pins that)
    for cls in (pk.OnlineScorer, pk.OnlineFeatureScorer, pk.OnlineRecognizer):
        with pytest.raises(TypeError):
            cls(None, None, 1, 1, transform=spec)


def test_online_recognizer_load_refusals(tmp_path):
    L = pk.lib()
    m = TC.matrix(13, 3, 3, 40, True)
    fe, good, dl = FA.SPECS[9].struct(), pk.TransformSpec(m, 3, 3).struct(), pk.DeltaSpec().struct()
    load = L.pk_mi355_transform_online_recognizer_load
    conf = str(tmp_path / "missing.conf").encode()
    assert not load(None, C.byref(fe), None, C.byref(good), 2, 1600, 0) and last() == (E_INVALID, "null argument")
    assert not load(conf, None, None, C.byref(good), 2, 1600, 0) and last() == (E_INVALID, "null argument")
    assert not load(conf, C.byref(fe), C.byref(dl), None, 2, 1600, 0) and last() == (E_INVALID, "null argument")
    bad = pk.DeltaSpec(2, 0).struct()
    assert not load(conf, C.byref(fe), C.byref(bad), C.byref(good), 2, 1600, 0)
    assert last()[0] == E_INVALID and "window" in last()[1]
    badx = pk.TransformSpec(m, 3, 3, in_dim=12).struct()
    assert not load(conf, C.byref(fe), None, C.byref(badx), 2, 1600, 0)
    assert last()[0] == E_INVALID and "cols" in last()[1]
    two = FA.S(bins=2).struct()
    assert not load(conf, C.byref(two), None, C.byref(good), 2, 1600, 0)
    assert last()[0] == E_INVALID and "num_mel_bins" in last()[1]
    for streams, cap, trace in ((0, 1600, 0), (2, 0, 0), (2, 1600, -1)):
        assert not load(conf, C.byref(fe), None, C.byref(good), streams, cap, trace)
        assert last() == (E_INVALID, "bad online recognizer capacity")
    assert not load(conf, C.byref(fe), None, C.byref(good), 2, 1600, 0)       # the files, before the device
    assert last()[0] != 0 and "missing.conf" in last()[1]
    with pytest.raises(pk.PkCodeError) as e:
        pk.OnlineRecognizer.with_transform(str(tmp_path / "missing.conf"), pk.TransformSpec(m, 3, 3), deltas=pk.DeltaSpec(4, 2))
    assert e.value.code == E_INVALID and "order" in str(e.value)
    with pytest.raises(TypeError, match="TransformSpec"):
        pk.OnlineRecognizer.with_transform(str(tmp_path / "missing.conf"), m)
