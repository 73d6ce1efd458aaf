"""Host-only: the graph reader (pk_mi355_fst_*, Fst::Read / CountArcs, fst.cc:29-110) and the decoder
entries' behaviour without a device.  No GPU needed."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth_graph as SG

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
E_INVALID, E_IO = -1, -3


def count_arcs(path):
    """Fst::CountArcs restated (as tests/test_gpu_decoder.py::read_fst does): (first, count) per state."""
    raw = open(path, "rb").read()
    ns, na = struct.unpack("<ii", raw[36:44])
    first = np.frombuffer(raw, np.int32, ns, 48 + 4 * ns)
    out = []
    for s in range(ns):
        if first[s] < 0:
            out.append((0, 0))
            continue
        nxt = [first[t] for t in range(s + 1, ns) if first[t] > 0]
        out.append((int(first[s]), int(nxt[0] if nxt else na) - int(first[s])))
    return out


def test_reads_the_reference_fixtures():
    f = pk.Fst(os.path.join(G, "testinput.fst"))
    assert (f.num_states(), f.num_arcs(), f.start()) == (3, 3, 0)
    assert [f.arc_range(s) for s in range(3)] == [(0, 2), (2, 1), (0, 0)]
    w = pk.Fst(os.path.join(G, "refmodel", "wordloop.fst"))
    assert w.start() == 0 and w.num_states() == 19
    assert sum(w.arc_range(s)[1] for s in range(19)) == 42 == w.num_arcs()


@pytest.mark.parametrize("name", ["testinput.fst", os.path.join("refmodel", "wordloop.fst")])
def test_arc_ranges_follow_count_arcs(name):
    path = os.path.join(G, name)
    f = pk.Fst(path)
    assert [f.arc_range(s) for s in range(f.num_states())] == count_arcs(path)


def raw_fst(ns, na, start, final, first, arcs, size=None, name=b"pk::fst_0"):
    body = struct.pack("<iii", ns, na, start) + np.asarray(final, "<f4").tobytes() + np.asarray(first, "<i4").tobytes()
    body += b"".join(struct.pack("<iiif", *a) for a in arcs)
    return name.ljust(32, b"\0") + struct.pack("<i", len(body) if size is None else size) + body


def test_count_arcs_quirk(tmp_path):
    """first = [0, 0, 2, -1, 3]: state 0's arcs end at the next first that is > 0 (state 2's), so states 0 and 1
    share arcs 0..1 -- the reference's `> 0`, not `>= 0`; state 3 has none; state 4 runs to the end."""
    arcs = [(1, 1, 0, 0.5), (2, 1, 0, 0.5), (3, 2, 0, 0.5), (4, 1, 0, 0.5), (0, 2, 0, 0.5)]
    p = tmp_path / "quirk.fst"
    p.write_bytes(raw_fst(5, 5, 0, [0.0] * 5, [0, 0, 2, -1, 3], arcs))
    f = pk.Fst(str(p))
    assert [f.arc_range(s) for s in range(5)] == [(0, 2), (0, 2), (2, 1), (0, 0), (3, 2)] == count_arcs(str(p))


def test_synth_graph_round_trips(tmp_path):
    g = SG.size_for_states(2000, seed=1)
    p = str(tmp_path / "g.fst")
    SG.write_fst(p, g["start"], g["final"], g["arcs"])
    f = pk.Fst(p)
    assert f.num_states() == len(g["arcs"]) and f.num_arcs() == sum(len(a) for a in g["arcs"])
    assert [f.arc_range(s)[1] for s in range(f.num_states())] == [len(a) for a in g["arcs"]]
    assert float(np.max(g["final"][np.isfinite(g["final"])]) - np.min(g["final"])) < 16.0


def test_rejects_malformed_and_senseless_graphs(tmp_path):
    good = open(os.path.join(G, "testinput.fst"), "rb").read()
    arcs = [(1, 1, 1, 0.5), (1, 2, 2, 1.5), (2, 3, 3, 2.5)]
    fin = [np.inf, np.inf, 3.5]
    cases = {
        "truncated": (good[:-5], E_IO),
        "header_only": (good[:40], E_IO),
        "name": (b"pk::fst_1" + good[9:], E_IO),
        "size": (good[:32] + struct.pack("<i", 1000) + good[36:], E_IO),
        "next": (raw_fst(3, 3, 0, fin, [0, 2, -1], [(1, 1, 1, 0.5), (3, 2, 2, 1.5), (2, 3, 3, 2.5)]), E_INVALID),
        "neg_next": (raw_fst(3, 3, 0, fin, [0, 2, -1], [(-1, 1, 1, 0.5), (1, 2, 2, 1.5), (2, 3, 3, 2.5)]), E_INVALID),
        "label": (raw_fst(3, 3, 0, fin, [0, 2, -1], [(1, -1, 1, 0.5), (1, 2, 2, 1.5), (2, 3, 3, 2.5)]), E_INVALID),
        "olabel": (raw_fst(3, 3, 0, fin, [0, 2, -1], [(1, 1, -4, 0.5), (1, 2, 2, 1.5), (2, 3, 3, 2.5)]), E_INVALID),
        "start": (raw_fst(3, 3, 3, fin, [0, 2, -1], arcs), E_INVALID),
        "neg_start": (raw_fst(3, 3, -1, fin, [0, 2, -1], arcs), E_INVALID),
        "range": (raw_fst(3, 3, 0, fin, [0, 7, -1], arcs), E_INVALID),
        "range_backwards": (raw_fst(3, 3, 0, fin, [2, 1, -1], arcs), E_INVALID),
        "nan_weight": (raw_fst(3, 3, 0, fin, [0, 2, -1], [(1, 1, 1, float("nan")), (1, 2, 2, 1.5), (2, 3, 3, 2.5)]),
                       E_INVALID),
        "inf_weight": (raw_fst(3, 3, 0, fin, [0, 2, -1], [(1, 1, 1, 0.5), (1, 2, 2, float("inf")), (2, 3, 3, 2.5)]),
                       E_INVALID),
        "nan_final": (raw_fst(3, 3, 0, [np.inf, float("nan"), 3.5], [0, 2, -1], arcs), E_INVALID),
    }
    for name, (data, code) in cases.items():
        p = tmp_path / (name + ".fst")
        p.write_bytes(data)
        with pytest.raises(pk.PkError) as e:
            pk.Fst(str(p))
        assert e.value.code == code, (name, str(e.value))
        rc_null = pk.lib().pk_mi355_fst_read(str(p).encode())
        assert not rc_null
    with pytest.raises(pk.PkError) as e:
        pk.Fst(str(tmp_path / "absent.fst"))
    assert e.value.code == E_IO
    assert not pk.lib().pk_mi355_fst_read(None) and pk.lib().pk_mi355_last_error_code() == E_INVALID
    L = pk.lib()
    f = pk.Fst(os.path.join(G, "testinput.fst"))
    import ctypes as C
    a, b = C.c_int(), C.c_int()
    assert L.pk_mi355_fst_arc_range(f.handle, 3, C.byref(a), C.byref(b)) == E_INVALID
    assert L.pk_mi355_fst_arc_range(f.handle, -1, C.byref(a), C.byref(b)) == E_INVALID


@pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0, reason="a GPU is present")
def test_decoder_entries_fail_loudly_without_gpu():
    L = pk.lib()
    f = pk.Fst(os.path.join(G, "testinput.fst"))
    am = L.pk_mi355_am_create()
    try:
        assert not L.pk_mi355_decoder_create(f.handle, am, 1, 0)            # model not finalized
        assert b"not finalized" in L.pk_mi355_last_error() and L.pk_mi355_last_error_code() == -4   # E_STATE
        assert not L.pk_mi355_decoder_create(None, am, 1, 0)
        assert L.pk_mi355_decoder_synchronize(None) == E_INVALID
        assert L.pk_mi355_decoder_decode(None, None, 0, 1) == E_INVALID
        assert L.pk_mi355_decoder_decode_batch(None, None, 1) == E_INVALID
        assert L.pk_mi355_decoder_set_beam(None, 16.0, 10) == E_INVALID
        assert L.pk_mi355_decoder_result(None, 0, None, 0, None, None) == E_INVALID
        assert L.pk_mi355_decoder_best_path_arcs(None, 0, None, 0) == E_INVALID
        assert L.pk_mi355_decoder_active_bound(None, 0) == E_INVALID
    finally:
        L.pk_mi355_am_destroy(am)
    with pytest.raises(pk.PkError):          # a model cannot even be finalized without a device
        pk.Decoder(f, pk.AcousticModel([("linear", np.eye(4, dtype=np.float32), np.zeros(4, np.float32))],
                                       prior=np.full(4, 0.25, np.float32)), 1)


def test_null_handles_are_invalid_in_every_decoder_entry():
    """Every pk_mi355_online_decoder_* entry, and the batch decoder's mode and alignment entries, given a null handle
    (tests/test_decode_gc_host.py has set_trace_gc and trace_stats): checked before any device is touched."""
    L = pk.lib()
    f = pk.Fst(os.path.join(G, "testinput.fst"))
    word, slot0, ll = pk.pk_mi355_word_t(), C.c_int(0), pk.pk_decodable_t()
    am = L.pk_mi355_am_create()
    try:
        for create in (L.pk_mi355_decoder_create, L.pk_mi355_online_decoder_create):
            for fst_h, am_h in ((None, am), (f.handle, None)):
                assert not create(fst_h, am_h, 1, 0)
                assert L.pk_mi355_last_error_code() == E_INVALID and b"null graph or model" in L.pk_mi355_last_error()
    finally:
        L.pk_mi355_am_destroy(am)
    L.pk_mi355_online_decoder_destroy(None)
    calls = [
        lambda: L.pk_mi355_online_decoder_set_beam(None, 16.0, 10),
        lambda: L.pk_mi355_online_decoder_open(None, 0),
        lambda: L.pk_mi355_online_decoder_advance(None, None, 1),
        lambda: L.pk_mi355_online_decoder_advance_host(None, C.byref(slot0), C.byref(ll), None, 1, 1),
        lambda: L.pk_mi355_online_decoder_synchronize(None),
        lambda: L.pk_mi355_online_decoder_partial(None, 0, None, 0, None),
        lambda: L.pk_mi355_online_decoder_result(None, 0, None, 0, None, None),
        lambda: L.pk_mi355_online_decoder_best_path_arcs(None, 0, None, 0),
        lambda: L.pk_mi355_online_decoder_word_segments(None, 0, C.byref(word), 1),
        lambda: L.pk_mi355_online_decoder_active_bound(None, 0),
        lambda: L.pk_mi355_decoder_set_trace_gc(None, 1),
        lambda: L.pk_mi355_decoder_set_alignment(None, 1),
        lambda: L.pk_mi355_decoder_alignment(None, 0, None, None, None, 0),
        lambda: L.pk_mi355_decoder_word_segments(None, 0, C.byref(word), 1),
    ]
    for i, call in enumerate(calls):
        assert call() == E_INVALID and L.pk_mi355_last_error_code() == E_INVALID, i
