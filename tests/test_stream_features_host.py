"""CPU-only: live features at the online scorer.  The new entries are declared, exported and
bound; null and malformed arguments end in their status codes with nothing dereferenced; the Python wrappers refuse a
wrong shape or kind by name before the library is called; an F16 model is refused before the device is touched.
(What needs a stream object needs a device: tests/test_gpu_stream_features.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pocketkaldi_amd as pk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
ENTRIES = ["pk_mi355_features_stream_create", "pk_mi355_stream_open_features", "pk_mi355_stream_push_features",
           "pk_mi355_stream_feat_dim", "pk_mi355_stream_slot_kind",
           "pk_mi355_online_recognizer_open_features", "pk_mi355_online_recognizer_push_features"]
f32p = C.POINTER(C.c_float)


def stats():
    return np.zeros(41, np.float32).ctypes.data_as(f32p)


def test_entries_are_declared_exported_and_bound():
    import subprocess
    header = open(os.path.join(REPO, "include", "pk_mi355.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = pk.lib()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True).split()
    version_script = open(os.path.join(os.path.dirname(pk.lib_path()), "csrc", "libpk_mi355.map")).read()
    assert "pk_mi355_*;" in version_script                 # the map exports the header's prefix, entry by entry
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pk.EXPORTS and name in exported and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name


def test_null_handles_and_malformed_arguments_are_codes_not_crashes():
    L = pk.lib()
    x = np.zeros(80, np.float32)
    assert not L.pk_mi355_features_stream_create(None, None, 4, 100)
    assert L.pk_mi355_last_error_code() == E_INVALID
    assert not L.pk_mi355_features_stream_create(None, stats(), 4, 100)
    assert L.pk_mi355_last_error_code() == E_INVALID
    for kind in (0, 1, 2, -1):
        assert L.pk_mi355_stream_open_features(None, 0, kind) == E_INVALID
    assert L.pk_mi355_stream_push_features(None, 0, x.ctypes.data_as(f32p), 2) == E_INVALID
    assert L.pk_mi355_stream_push_features(None, 0, None, 0) == E_INVALID
    assert L.pk_mi355_stream_push_features(None, 0, None, -1) == E_INVALID
    assert L.pk_mi355_stream_feat_dim(None) == E_INVALID
    assert L.pk_mi355_stream_slot_kind(None, 0) == E_INVALID
    assert b"null stream" in L.pk_mi355_last_error()
    assert L.pk_mi355_online_recognizer_open_features(None, 0, 0) == E_INVALID
    assert L.pk_mi355_online_recognizer_push_features(None, 0, x.ctypes.data_as(f32p), 2) == E_INVALID
    assert b"null online recognizer" in L.pk_mi355_last_error()


def test_model_checks_come_before_the_device():
    L = pk.lib()
    for precision in (1, 2):                     # PK_MI355_PRECISION_F16X3, _F16
        am = L.pk_mi355_am_create()
        try:
            assert L.pk_mi355_am_set_precision(am, precision) == 0
            for g in (None, stats()):
                assert not L.pk_mi355_features_stream_create(am, g, 4, 100)
                assert L.pk_mi355_last_error_code() == E_INVALID
                assert b"f32" in L.pk_mi355_last_error()
        finally:
            L.pk_mi355_am_destroy(am)
    am = L.pk_mi355_am_create()                  # f32, not finalized
    try:
        assert not L.pk_mi355_features_stream_create(am, None, 4, 100)
        assert L.pk_mi355_last_error_code() == E_STATE
    finally:
        L.pk_mi355_am_destroy(am)


def unfinished_model(precision):
    am = pk.AcousticModel.__new__(pk.AcousticModel)
    am._h = pk.lib().pk_mi355_am_create()
    pk.lib().pk_mi355_am_set_precision(am._h, precision)
    return am


def test_python_constructor_raises_with_the_code():
    am = unfinished_model(1)
    try:
        with pytest.raises(pk.PkCodeError) as e:
            pk.OnlineFeatureScorer(am, 2, 100)
        assert e.value.code == E_INVALID
        with pytest.raises(pk.PkCodeError) as e:
            pk.OnlineFeatureScorer(am, 2, 100, global_stats=np.zeros(41, np.float32))
        assert e.value.code == E_INVALID
        with pytest.raises(pk.PkError, match="41"):
            pk.OnlineFeatureScorer(am, 2, 100, global_stats=np.zeros(40, np.float32))
    finally:
        am.close()
    assert issubclass(pk.OnlineFeatureScorer, pk.OnlineScorer)


def wrapper(cls, feat_dim, **fields):
    """A wrapper object without a handle: reaching the library with it would fail, so the refusals asked for below must
    come before that.  feat_dim is answered here."""
    sc = cls.__new__(cls)
    sc._h = None
    for k, v in fields.items():
        setattr(sc, k, v)
    sc.feat_dim = lambda: feat_dim
    return sc


def test_wrappers_refuse_a_wrong_shape_or_kind_by_name_before_the_library():
    sc = wrapper(pk.OnlineFeatureScorer, 13, _max_streams=2)
    for bad in (np.zeros(13, np.float32), np.zeros((4, 12), np.float32), np.zeros((2, 13, 1), np.float32), np.zeros((0, 14), np.float32)):
        with pytest.raises(pk.PkCodeError, match=r"shape .*expected \[n\]\[13\]") as e:
            sc.push_features(0, bad)
        assert e.value.code == E_INVALID
    with pytest.raises(pk.PkCodeError, match="not a float matrix"):
        sc.push_features(0, [["a", "b"]])
    for kind in ("cmvn", 0, None):
        with pytest.raises(pk.PkCodeError, match="feature kind") as e:
            sc.open_features(0, kind)
        assert e.value.code == E_INVALID
    for slot in (-1, 2):
        with pytest.raises(pk.PkCodeError, match="out of range") as e:
            sc.slot_kind(slot)
        assert e.value.code == E_INVALID
    rec = pk.OnlineRecognizer.__new__(pk.OnlineRecognizer)
    rec._h = None
    rec.scorer = wrapper(pk.OnlineScorer, 40)
    with pytest.raises(pk.PkCodeError, match=r"expected \[n\]\[40\]"):
        rec.push_features(0, np.zeros((3, 39), np.float32))
    with pytest.raises(pk.PkCodeError, match="feature kind"):
        rec.open_features(0, "fbank")
    rec.scorer = None
