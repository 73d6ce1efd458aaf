"""Host-only: every entry of the online decoder's commit mode refuses a null object, through the library and without a
device; the command-line program refuses --commit without --online.  (That `committed` is zeros on a closed, fresh slot
needs a decoder, and a decoder needs a device: tests/test_gpu_online_commit.py holds it.)"""
import ctypes as C

import pocketkaldi_amd as pk

E_INVALID = -1


def test_null_objects_are_refused_without_a_device():
    L = pk.lib()
    ints = (C.c_int32 * 4)()
    a, b, c = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    n, m = C.c_int(7), C.c_int(7)
    assert L.pk_mi355_online_decoder_set_commit(None, 1) == E_INVALID and b"null online decoder" in L.pk_mi355_last_error()
    assert L.pk_mi355_online_decoder_set_commit(None, 0) == E_INVALID
    assert L.pk_mi355_online_decoder_committed(None, 0, ints, 4, C.byref(n), C.byref(m)) == E_INVALID
    assert b"null online decoder" in L.pk_mi355_last_error()
    assert L.pk_mi355_online_decoder_committed(None, 0, None, 0, None, None) == E_INVALID
    assert L.pk_mi355_online_decoder_trace_stats(None, 0, C.byref(a), C.byref(b), C.byref(c)) == E_INVALID
    assert b"null online decoder" in L.pk_mi355_last_error()
    assert L.pk_mi355_online_decoder_trace_stats(None, 0, None, None, None) == E_INVALID
    assert (n.value, m.value, a.value, b.value, c.value, list(ints)) == (7, 7, 7, 7, 7, [0] * 4)    # nothing written
    assert L.pk_mi355_online_recognizer_stable(None, 0) is None
    assert L.pk_mi355_last_error_code() == E_INVALID and b"null online recognizer" in L.pk_mi355_last_error()


def test_the_new_entries_are_exported():
    for name in ("pk_mi355_online_decoder_set_commit", "pk_mi355_online_decoder_committed",
                 "pk_mi355_online_decoder_trace_stats", "pk_mi355_online_recognizer_stable"):
        assert name in pk.EXPORTS and hasattr(pk.lib(), name)
    for cls, method in ((pk.OnlineDecoder, "set_commit"), (pk.OnlineDecoder, "committed"), (pk.OnlineDecoder, "trace_stats"),
                        (pk.OnlineRecognizer, "stable")):
        assert callable(getattr(cls, method))


def test_commit_flag_needs_online(capsys):
    from pocketkaldi_amd import recognize
    for argv in (["m.conf", "x.wav", "--commit"], ["m.conf", "x.wav", "--ctm", "--commit"]):
        assert recognize.main(argv) == 1
        assert capsys.readouterr().out.startswith("Usage:"), argv
