"""CPU-only: the online scorer's entry points (pk_mi355_stream_*) report argument and call-order errors as status
codes before anything touches a device.  (Pushes to closed slots, steps without an open slot and pushes over the step
capacity need a stream object, which needs a device: tests/test_gpu_stream.py covers them.)"""
import ctypes as C

import numpy as np
import pytest

import pocketkaldi_amd as pk

E_INVALID, E_STATE = -1, -4


def stats():
    return np.zeros(41, np.float32).ctypes.data_as(C.POINTER(C.c_float))


def test_f16_models_are_refused_before_the_device():
    L = pk.lib()
    for precision in (1, 2):                     # PK_MI355_PRECISION_F16X3, _F16
        am = L.pk_mi355_am_create()
        try:
            assert L.pk_mi355_am_set_precision(am, precision) == 0
            assert not L.pk_mi355_stream_create(am, stats(), 4, 16000)
            assert L.pk_mi355_last_error_code() == E_INVALID
            assert b"f32" in L.pk_mi355_last_error()
        finally:
            L.pk_mi355_am_destroy(am)


def test_unfinalized_model_and_bad_capacity():
    L = pk.lib()
    am = L.pk_mi355_am_create()
    try:
        assert not L.pk_mi355_stream_create(am, stats(), 4, 16000)
        assert L.pk_mi355_last_error_code() == E_STATE
        assert not L.pk_mi355_stream_create(None, stats(), 4, 16000)
        assert L.pk_mi355_last_error_code() == E_INVALID
    finally:
        L.pk_mi355_am_destroy(am)


def test_null_stream_is_an_error_not_a_crash():
    L = pk.lib()
    x = np.zeros(16, np.float32)
    assert L.pk_mi355_stream_open(None, 0) == E_INVALID
    assert L.pk_mi355_stream_push(None, 0, x.ctypes.data_as(C.POINTER(C.c_float)), 16) == E_INVALID
    assert L.pk_mi355_stream_push_i16(None, 0, None, 0) == E_INVALID
    assert L.pk_mi355_stream_close(None, 0) == E_INVALID
    assert L.pk_mi355_stream_step(None, 0.1, 1) == E_INVALID
    assert L.pk_mi355_stream_synchronize(None) == E_INVALID
    first, count = C.c_int(7), C.c_int(7)
    assert not L.pk_mi355_stream_loglik_device(None, 0, C.byref(first), C.byref(count))
    assert first.value == 0 and count.value == 0
    d = pk.pk_decodable_t()
    assert L.pk_mi355_stream_fetch(None, 0, C.byref(d), None) == E_INVALID
    L.pk_mi355_stream_destroy(None)


def test_python_wrapper_raises_with_the_code():
    am = pk.AcousticModel.__new__(pk.AcousticModel)
    am._h = pk.lib().pk_mi355_am_create()
    try:
        pk.lib().pk_mi355_am_set_precision(am._h, 1)
        with pytest.raises(pk.PkCodeError) as e:
            pk.OnlineScorer(am, np.zeros(41, np.float32), 2, 1000)
        assert e.value.code == E_INVALID
        with pytest.raises(pk.PkError):
            pk.OnlineScorer(am, np.zeros(40, np.float32), 2, 1000)
    finally:
        am.close()
