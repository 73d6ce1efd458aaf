"""CPU-only: delta features on the online objects -- the three entries' names in header, export
list, binding and C++ header, and the refusals of pk_mi355_deltas_stream_create and
pk_mi355_deltas_online_recognizer_load that are said without a device: a null model, null arguments, a bad deltas spec
by its field, an f16 model, a model that is not finalized.  The refusals that read a finalized model, which needs a
device -- a feat_dim that order + 1 does not divide, a front-end of another dimension than Db, another stats_len, a
capacity <= 0 -- are in tests/test_gpu_stream_deltas.py's failure-code test, with the texts of the batch entry."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import frontend_any_cases as FA

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
NEW_ENTRIES = ["pk_mi355_deltas_stream_create", "pk_mi355_stream_base_dim", "pk_mi355_deltas_online_recognizer_load"]
f32p = C.POINTER(C.c_float)


def last():
    return pk.lib().pk_mi355_last_error_code(), pk.lib().pk_mi355_last_error().decode()


def fp(a):
    return a.ctypes.data_as(f32p)


def model(precision=0):
    am = pk.lib().pk_mi355_am_create()
    assert am and pk.lib().pk_mi355_am_set_precision(am, precision) == 0
    return am


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
    assert "do not have deltas yet" not in header
    assert L.pk_mi355_deltas_stream_create.restype is C.c_void_p and L.pk_mi355_deltas_online_recognizer_load.restype is C.c_void_p


def test_stream_create_refusals_without_a_device():
    L = pk.lib()
    good = pk.DeltaSpec(2, 2).struct()
    fe, g = FA.SPECS[9].struct(), np.zeros(14, np.float32)
    assert not L.pk_mi355_deltas_stream_create(None, C.byref(good), None, None, 0, 2, 100)
    assert last() == (E_STATE, "model not finalized")                           # the batch entry's words for a null model
    am = model()
    try:
        assert not L.pk_mi355_deltas_stream_create(am, None, None, None, 0, 2, 100)
        assert last() == (E_INVALID, "null argument")                          # a null spec
        assert not L.pk_mi355_deltas_stream_create(am, C.byref(good), C.byref(fe), None, 0, 2, 1600)
        assert last() == (E_INVALID, "null argument")                          # a front-end without statistics
        for order, window, field in ((4, 2, "order"), (0, 2, "order"), (2, 0, "window"), (2, 9, "window")):
            st = pk.DeltaSpec(order, window).struct()
            assert L.pk_mi355_deltas_check(C.byref(st)) == E_INVALID
            words = last()[1]
            assert words.startswith("deltas spec:") and field in words
            assert not L.pk_mi355_deltas_stream_create(am, C.byref(st), C.byref(fe), fp(g), 14, 2, 1600)
            assert last() == (E_INVALID, words)
            assert not L.pk_mi355_deltas_stream_create(am, C.byref(st), None, None, 0, 2, 100)
            assert last() == (E_INVALID, words)
        assert not L.pk_mi355_deltas_stream_create(am, C.byref(good), C.byref(fe), fp(g), 14, 2, 1600)      # f32, not finalized
        assert last() == (E_STATE, "model not finalized")
        assert not L.pk_mi355_deltas_stream_create(am, C.byref(good), None, None, 0, 2, 100)
        assert last() == (E_STATE, "model not finalized")
    finally:
        L.pk_mi355_am_destroy(am)
    for precision in (1, 2):                     # PK_MI355_PRECISION_F16X3, _F16: refused, as on every online scorer
        am = model(precision)
        try:
            assert not L.pk_mi355_deltas_stream_create(am, C.byref(good), C.byref(fe), fp(g), 14, 2, 1600)
            code, words = last()
            assert code == E_INVALID and "f32" in words
        finally:
            L.pk_mi355_am_destroy(am)
    assert L.pk_mi355_stream_base_dim(None) == E_INVALID and "null stream" in last()[1]


def test_python_constructors_raise_with_the_code():
    am = pk.AcousticModel.__new__(pk.AcousticModel)
    am._h = model(1)
    try:
        for make in (lambda d: pk.OnlineFeatureScorer(am, 2, 100, deltas=d),
                     lambda d: pk.OnlineScorer(am, np.zeros(14, np.float32), 2, 1600, frontend=FA.SPECS[9], deltas=d),
                     lambda d: pk.OnlineScorer(am, np.zeros(41, np.float32), 2, 1600, deltas=d)):      # the default front-end
            with pytest.raises(pk.PkCodeError) as e:
                make(pk.DeltaSpec(2, 2))
            assert e.value.code == E_INVALID and "f32" in str(e.value)
            with pytest.raises(pk.PkCodeError) as e:
                make(pk.DeltaSpec(4, 2))
            assert e.value.code == E_INVALID and "order" in str(e.value)
    finally:
        am.close()


def test_online_recognizer_load_refusals(tmp_path):
    L = pk.lib()
    fe, good = FA.SPECS[9].struct(), pk.DeltaSpec().struct()
    conf = str(tmp_path / "missing.conf").encode()
    assert not L.pk_mi355_deltas_online_recognizer_load(None, C.byref(fe), C.byref(good), 2, 1600, 0) and last() == (E_INVALID, "null argument")
    assert not L.pk_mi355_deltas_online_recognizer_load(conf, None, C.byref(good), 2, 1600, 0) and last() == (E_INVALID, "null argument")
    assert not L.pk_mi355_deltas_online_recognizer_load(conf, C.byref(fe), None, 2, 1600, 0) and last() == (E_INVALID, "null argument")
    bad = pk.DeltaSpec(2, 0).struct()
    assert not L.pk_mi355_deltas_online_recognizer_load(conf, C.byref(fe), C.byref(bad), 2, 1600, 0)
    assert last()[0] == E_INVALID and "window" in last()[1]
    two = FA.S(bins=2).struct()
    assert not L.pk_mi355_deltas_online_recognizer_load(conf, C.byref(two), C.byref(good), 2, 1600, 0)
    assert last()[0] == E_INVALID and "num_mel_bins" in last()[1]
    for streams, cap, trace in ((0, 1600, 0), (2, 0, 0), (2, 1600, -1)):
        assert not L.pk_mi355_deltas_online_recognizer_load(conf, C.byref(fe), C.byref(good), streams, cap, trace)
        assert last() == (E_INVALID, "bad online recognizer capacity")
    assert not L.pk_mi355_deltas_online_recognizer_load(conf, C.byref(fe), C.byref(good), 2, 1600, 0)       # the files, before the device
    assert last()[0] != 0 and "missing.conf" in last()[1]
    with pytest.raises(pk.PkCodeError) as e:
        pk.OnlineRecognizer(str(tmp_path / "missing.conf"), deltas=pk.DeltaSpec(4, 2))
    assert e.value.code == E_INVALID and "order" in str(e.value)
