"""The batch decoder's trace-gc entry points where no GPU is needed: a null decoder is refused.  (What they do on a
decoder -- pk_mi355_decoder_trace_stats before any call included, which needs a decoder and so a device -- is in
tests/test_gpu_decode_gc.py; tests/test_abi_loads.py covers the exports.)"""
import ctypes as C

import pocketkaldi_amd as pk

E_INVALID = -1


def test_trace_gc_entries_refuse_a_null_decoder():
    L = pk.lib()
    assert L.pk_mi355_decoder_set_trace_gc(None, 1) == E_INVALID
    assert L.pk_mi355_last_error_code() == E_INVALID and b"null decoder" in L.pk_mi355_last_error()
    peak, size, n = C.c_int64(7), C.c_int64(7), C.c_int(7)
    assert L.pk_mi355_decoder_trace_stats(None, 0, C.byref(peak), C.byref(size), C.byref(n)) == E_INVALID
    assert L.pk_mi355_decoder_trace_stats(None, 0, None, None, None) == E_INVALID
    assert (peak.value, size.value, n.value) == (7, 7, 7)          # nothing written on failure
    assert {"pk_mi355_decoder_set_trace_gc", "pk_mi355_decoder_trace_stats"} <= set(pk.EXPORTS)
