"""The plain trace compaction (CompactTrace<., false> in csrc/decode.hip: DecodeKernel<true>'s and OnlineDecodeKernel's,
before an emitting frame of an arena more than half full) at the edges of its chunked scan.  The construction is
tests/commit_cases.py's two_chains: the arena holds exactly n records when the one compaction of the run fires, for n
around kDecThreads and twice that, the dead chain's records lie between the live ones, and n - DEAD_FROM survive
(tests/test_commit_model.py holds these counts on the host model).  Where records live changes no result."""
import pytest

import pocketkaldi_amd as pk

import commit_cases as CC
from test_gpu_decode_edges import outcome
from test_gpu_online_align import batch, full
from test_gpu_online_commit import make
from test_gpu_online_decode import ident_model, write_graph

pytestmark = pytest.mark.gpu
D = CC.DEAD_FROM
_cases = {}


def case(tmp_path, n):
    """two_chains(n) and the yardstick: the batch decoder, trace gc off, a large arena, alignment on.  Once per n."""
    if n not in _cases:
        g, ll, cap = CC.two_chains(n)
        fst, am = pk.Fst(write_graph(tmp_path, "two_%d.fst" % n, g)), ident_model(4)
        want = batch(fst, am, [ll], beam=CC.WIDE, max_active=1 << 30)
        assert want.result(0)[2] == 1 and len(want.best_path_arcs(0)) == ll.shape[0] == n - D + 4
        assert want.trace_stats(0) == (2 * D + (n - D + 4 - D), 1 << 20, 0)    # two records a frame, then one
        _cases[n] = fst, am, ll, cap, want
    return _cases[n]


@pytest.mark.parametrize("n", CC.EDGES)
def test_batch_trace_gc(tmp_path, n):
    fst, am, ll, cap, want = case(tmp_path, n)
    for align in (False, True):
        dec = pk.Decoder(fst, am, 1, trace_capacity=cap, trace_gc=True)
        dec.set_beam(CC.WIDE, 1 << 30)
        dec.set_alignment(align)
        dec.decode([ll])
        assert dec.trace_stats(0) == (n, cap, 1)
        assert outcome(dec, 0) == outcome(want, 0) and dec.best_path_arcs(0) == want.best_path_arcs(0)
        if align:
            assert full(dec, 0) == full(want, 0)


@pytest.mark.parametrize("n", CC.EDGES)
def test_online_commit_off(tmp_path, n):
    fst, am, ll, cap, want = case(tmp_path, n)
    for align in (False, True):
        dec = make(fst, am, 1, False, align, beam=CC.WIDE, max_active=1 << 30, cap=cap)
        dec.open(0)
        dec.advance_host({0: (ll, False)})
        assert dec.trace_stats(0)[0] == n - D + 4              # (n + 4 had nothing been compacted)
        assert dec.best_path_arcs(0) == want.best_path_arcs(0)
        dec.advance_host({0: (ll[:0], True)})
        if align:
            assert full(dec, 0) == full(want, 0)               # rec_ac moved with rec across the chunk edge
        else:
            assert outcome(dec, 0) == outcome(want, 0)


@pytest.mark.parametrize("n", CC.EDGES)
def test_online_commit_on(tmp_path, n):
    """The plain compaction and the commit in one launch."""
    fst, am, ll, cap, want = case(tmp_path, n)
    for align in (False, True):
        dec = make(fst, am, 1, True, align, beam=CC.WIDE, max_active=1 << 30, cap=cap)
        dec.open(0)
        dec.advance_host({0: (ll, False)})
        in_use, peak, capacity = dec.trace_stats(0)
        assert (in_use, peak, capacity) == (1, n, cap)         # one chain is left: all of it but its last arc is committed
        assert dec.committed(0)[1] == n - D + 3 and dec.best_path_arcs(0) == want.best_path_arcs(0)
        dec.advance_host({0: (ll[:0], True)})
        if align:
            assert full(dec, 0) == full(want, 0)
        else:
            assert outcome(dec, 0) == outcome(want, 0)
