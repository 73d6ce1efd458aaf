"""The online decoder's alignment mode (pk_mi355_online_decoder_set_alignment / _alignment / _num_frames:
csrc/capi_online_decoder.hip; OnlineDecodeKernel<true> in csrc/decode.hip keeps every trace record's acoustic cost
beside it, CompactTrace moves it, the path walk reads it out).  The mode changes no result; a finished slot's alignment
and word segments are the batch decoder's (AlignKernel) bit for bit, acoustic cost included; a live slot's are the
Python restatement of tests/test_gpu_align.py over best_path_arcs and the rows fed so far; compaction, N1, poisoned
neighbours, a slot that ran out of trace records and slot reuse change none of it."""
import math

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth_graph as SG

from test_gpu_align import TRACE, bits, check_alignment, got_segments, restate
from test_gpu_decode_edges import GRIDS, NANS, PDF, flat_list, graph, outcome
from test_gpu_online_decode import ident_model, split, write_graph

pytestmark = pytest.mark.gpu
E_STATE, E_CAPACITY = -4, -6
INF = np.inf
LENGTHS = [0, 1, 7, 40, 90, 130]
BLOCK = 512                                     # kDecThreads: CompactTrace renumbers the records in chunks of this many


def all_final(g, w=1.0):
    g["final"][:] = np.where(np.isinf(g["final"]), np.float32(w), g["final"])
    return g


def batch(fst, am, lls, beam=16.0, max_active=30000, trace=TRACE):
    """The yardstick: the batch decoder with alignment on, on the whole utterances."""
    dec = pk.Decoder(fst, am, len(lls), trace_capacity=trace)
    dec.set_beam(beam, max_active)
    dec.set_alignment(True)
    dec.decode(lls)
    return dec


def full(dec, u):
    """Everything a slot (utterance) ends with, as comparable values."""
    return outcome(dec, u), [a.tobytes() for a in dec.alignment(u)], got_segments(dec, u)


def feed(dec, lls, hows, seed=0, slots=None, after=None, tolerate=()):
    """Slot slots[u] of dec is opened and fed lls[u] in chunks split(hows[u]), then finished with an empty chunk;
    after(slot, u, frames fed) runs after every advance of a live slot.  -> the codes of the advances that raised."""
    rng = np.random.default_rng(seed)
    slots = list(range(len(lls))) if slots is None else slots
    plans = [split(ll.shape[0], h, rng) for ll, h in zip(lls, hows)]
    pos, codes = [0] * len(lls), []
    for s in slots:
        dec.open(s)
    step = 0
    while any(step <= len(p) for p in plans):
        chunks = {}
        for u, p in enumerate(plans):
            if step < len(p):
                chunks[slots[u]] = (lls[u][pos[u]:pos[u] + p[step]], False)
                pos[u] += p[step]
            elif step == len(p):
                chunks[slots[u]] = (lls[u][pos[u]:pos[u]], True)
        try:
            dec.advance_host(chunks)
        except pk.PkCodeError as e:
            assert e.code in tolerate, str(e)
            codes.append(e.code)
        if after:
            for u in range(len(lls)):
                if slots[u] in chunks and not chunks[slots[u]][1]:
                    after(slots[u], u, pos[u])
        step += 1
    return codes


def online(fst, am, n, align=True, beam=16.0, max_active=30000, cap=TRACE):
    dec = pk.OnlineDecoder(fst, am, n, trace_capacity=cap)
    dec.set_beam(beam, max_active)
    if align:
        dec.set_alignment(True)
    return dec


# ---------------------------------------------------------------- 1, 2: the mode changes no result; final = batch

_general = {}


def general(tmp_path, grid):
    """One general graph per grid, six utterances, decoded by the batch decoder and by the online one with the mode
    off and on under each chunking: computed once per grid, shared by the tests below."""
    if grid not in _general:
        k, eps_k = GRIDS[grid]
        g = all_final(SG.general(300, 8100 + k, k=k, eps_k=eps_k))
        fst, am = pk.Fst(write_graph(tmp_path, "g_%s.fst" % grid, g)), ident_model(g["num_pdfs"])
        lls = [SG.dyadic(T, g["num_pdfs"], 700 + u, k=k) for u, T in enumerate(LENGTHS)]
        want = batch(fst, am, lls)
        runs = {}
        for how in (1, "random", "whole"):
            for align in (False, True):
                dec = online(fst, am, len(lls), align)
                feed(dec, lls, [how] * len(lls), seed=3)
                runs[how, align] = dec
        _general[grid] = g, lls, want, runs
    return _general[grid]


@pytest.mark.parametrize("grid", ["coarse", "fine"])
def test_the_mode_changes_no_result(tmp_path, grid):
    g, lls, want, runs = general(tmp_path, grid)
    assert sum(want.result(u)[2] for u in range(len(lls))) == len(lls) and len(want.best_path_arcs(5)) >= 130
    for (how, align), dec in runs.items():
        for u in range(len(lls)):
            assert outcome(dec, u) == outcome(want, u), (how, align, u)


@pytest.mark.parametrize("grid", ["coarse", "fine"])
def test_final_alignment_equals_the_batch_decoders(tmp_path, grid):
    g, lls, want, runs = general(tmp_path, grid)
    arcs = flat_list(g)
    for how in (1, "random", "whole"):
        dec = runs[how, True]
        for u, ll in enumerate(lls):
            assert dec.num_frames(u) == ll.shape[0]
            assert full(dec, u) == full(want, u), (how, u)
            assert check_alignment(dec, u, arcs, ll) == ll.shape[0]            # and both are the restatement


# ---------------------------------------------------------------- 3: a live slot

@pytest.mark.parametrize("grid", ["coarse", "fine"])
def test_live_alignment(tmp_path, grid):
    k, eps_k = GRIDS[grid]
    g = all_final(SG.general(300, 8200 + k, k=k, eps_k=eps_k))
    fst, am = pk.Fst(write_graph(tmp_path, "g.fst", g)), ident_model(g["num_pdfs"])
    lls = [SG.dyadic(T, g["num_pdfs"], 900 + u, k=k) for u, T in enumerate([40, 90])]
    arcs = flat_list(g)
    dec = online(fst, am, 2)
    checked = []

    def after(slot, u, fed):
        path = dec.best_path_arcs(slot)
        ids, tids, ac = dec.alignment(slot)
        words, cost = dec.partial(slot)
        if not path:
            assert len(ids) == 0 and fed == 0
            return
        assert dec.num_frames(slot) == fed == len(ids) == len(tids) == len(ac)
        want_ids, want_tids, want_ac, want_segs = restate(arcs, path, lls[u][:fed], PDF)
        assert ids.tolist() == want_ids and tids.tolist() == want_tids and ac.tobytes() == want_ac.tobytes(), (u, fed)
        segs = dec.word_segments(slot)
        assert got_segments(dec, slot) == want_segs, (u, fed)
        assert [s.word for s in segs if s.word] == words
        if grid == "coarse":                    # every sum is exact on the 2^-2 grid: the two halves are the partial's cost
            assert sum(float(s.graph_cost) for s in segs) + sum(float(s.acoustic_cost) for s in segs) == float(cost), (u, fed)
        checked.append(fed)

    feed(dec, lls, [1, "random"], seed=5, after=after)
    assert len(checked) > 40 + 5


# ---------------------------------------------------------------- 4: compaction carries the costs

def probe_capacity(fst, am, ll, beam, max_active, candidates):
    """The first of `candidates` (records per utterance) that the batch decoder's trace gc -- the same compaction rule,
    not the code under test -- decodes ll in, with at least one compaction."""
    for cap in candidates:
        dec = pk.Decoder(fst, am, 1, trace_capacity=cap, trace_gc=True)
        dec.set_beam(beam, max_active)
        try:
            dec.decode([ll])
        except pk.PkCodeError as e:
            assert e.code == E_CAPACITY, str(e)
            continue
        assert dec.trace_stats(0)[2] >= 1
        return cap
    raise AssertionError("no capacity below half the records fits: %r" % (candidates,))


@pytest.mark.parametrize("case", ["pruned", "unpruned"])
def test_compaction_carries_the_costs(tmp_path, case):
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    fst, am = pk.Fst(write_graph(tmp_path, "w.fst", g)), ident_model(g["num_tids"])
    lls = [SG.planted(g, 120 if case == "pruned" else 150, seed=1)[0], SG.planted(g, 150, seed=2)[0]]
    beam, max_active = (16.0, 30000) if case == "pruned" else (INF, 1 << 30)
    want = batch(fst, am, lls, beam, max_active, trace=1 << 23)
    alone = []
    for ll in lls:                              # the records each utterance writes, decoded alone with gc off
        d = pk.Decoder(fst, am, 1, trace_capacity=1 << 23)
        d.set_beam(beam, max_active)
        d.decode([ll])
        alone.append(d.trace_stats(0)[0])
    least = min(alone)
    candidates = [least // 4, least // 3, least * 2 // 5, least * 9 // 20]
    if case == "pruned":
        candidates = [least // 8, least // 6] + candidates
    cap = max(probe_capacity(fst, am, ll, beam, max_active, candidates) for ll in lls)
    print("records alone %r, records per slot %d" % (alone, cap))
    assert cap < least // 2                     # so every slot compacts at least once
    if case == "unpruned":
        # Nothing is pruned, so a frame's token list is every state it touched, and on a word loop (every state on a
        # cycle through the loop state, every log-likelihood finite) a state once alive stays alive.  A short prefix
        # already touches as many states as any later frame, more than one chunk of CompactTrace; the first
        # compaction comes after it (the prefix writes fewer than cap / 2 records); and every token of a list holds
        # a record of its own.  So more than 512 records are alive at every compaction.
        for u, ll in enumerate(lls):
            assert want.active_bound(u) > BLOCK
            for frames in (5, 10, 15, 20):
                d = pk.Decoder(fst, am, 1, trace_capacity=1 << 23)
                d.set_beam(beam, max_active)
                d.decode([ll[:frames]])
                if d.active_bound(0) == want.active_bound(u):
                    break
            assert d.active_bound(0) == want.active_bound(u) and d.trace_stats(0)[0] < cap // 2, (u, frames)
    dec = online(fst, am, 2, True, beam, max_active, cap=cap)
    feed(dec, lls, [1, "random"], seed=8)
    arcs = flat_list(g)
    for u, ll in enumerate(lls):
        assert full(dec, u) == full(want, u), u
        assert check_alignment(dec, u, arcs, ll) == ll.shape[0]


# ---------------------------------------------------------------- 5: edges

def test_zero_frames_on_an_epsilon_path_and_one_frame(tmp_path):
    # the graph of test_gpu_align: T = 0 reaches the only final state over three epsilon arcs, two of them with words
    g = graph([INF, INF, INF, 0.25, 0.0], [[(1, 0, 4, 0.5)], [(2, 0, 0, 0.25)], [(3, 0, 5, 0.125), (4, 1, 6, 0.5)], [], []])
    fst, am = pk.Fst(write_graph(tmp_path, "e.fst", g)), ident_model(8)
    one = SG.dyadic(1, 8, 3, k=2)
    lls = [np.zeros((0, 8), np.float32), one]
    want = batch(fst, am, lls)
    dec = online(fst, am, 2)
    feed(dec, lls, ["whole", "whole"])
    assert dec.result(0)[0] == [4, 5] and dec.best_path_arcs(0) == [0, 1, 2] and dec.num_frames(0) == 0
    assert all(len(a) == 0 for a in dec.alignment(0))
    assert got_segments(dec, 0) == [(4, 0, 0, bits(0.75), bits(0.0)), (5, 0, 0, bits(0.125), bits(0.0))]
    assert dec.best_path_arcs(1) == [0, 1, 3] and dec.num_frames(1) == 1
    assert check_alignment(dec, 1, flat_list(g), one) == 1
    assert dec.alignment(1)[0].tolist() == [3] and dec.alignment(1)[1].tolist() == [1]
    for u in range(2):
        assert full(dec, u) == full(want, u)


def test_nan_off_the_path_changes_nothing(tmp_path):
    # as test_gpu_align: no pruning, a grid where ties are rare; NaN or -inf on pdfs the path does not read at that frame
    k, eps_k = GRIDS["fine"]
    g = all_final(SG.general(100, 7200, k=k, eps_k=eps_k))
    fst, am = pk.Fst(write_graph(tmp_path, "g.fst", g)), ident_model(g["num_pdfs"])
    clean = [SG.dyadic(40, g["num_pdfs"], 30 + u, k=k) for u in range(3)]
    dec = online(fst, am, 3, beam=INF, max_active=1 << 30)
    feed(dec, clean, [1, "random", "whole"], seed=2)
    arcs = flat_list(g)
    before = [full(dec, u) for u in range(3)]
    dirty = []
    for u, ll in enumerate(clean):
        assert check_alignment(dec, u, arcs, ll) == 40
        on_path = dec.alignment(u)[1]
        x, rng = ll.copy(), np.random.default_rng(u)
        for t in range(40):
            for p in rng.choice([p for p in range(g["num_pdfs"]) if p != on_path[t]], 3, replace=False):
                x[t, p] = (NANS[0], NANS[1], np.float32(-np.inf))[int(rng.integers(3))]
        dirty.append(x)
    feed(dec, dirty, ["random", "whole", 1], seed=3)          # the same slots, used again
    for u, ll in enumerate(dirty):
        assert check_alignment(dec, u, arcs, ll) == 40
        assert full(dec, u)[0][:4] == before[u][0][:4] and full(dec, u)[1:] == before[u][1:], u


def test_poisoned_neighbours_in_32_slots(tmp_path):
    g = all_final(SG.general(200, 7100, k=2, eps_k=12))
    fst, am = pk.Fst(write_graph(tmp_path, "g.fst", g)), ident_model(g["num_pdfs"])
    ll = SG.dyadic(45, g["num_pdfs"], 17, k=2)
    want = batch(fst, am, [ll])
    poison = []
    for i, value in enumerate((NANS[0], np.float32(-np.inf), NANS[1], np.float32(1.0e30))):
        x = SG.dyadic(45, g["num_pdfs"], 40 + i, k=2)
        x[5 + i:, ::2] = value
        poison.append(x)
    dec = online(fst, am, 32)
    feed(dec, [poison[0], poison[1], ll, poison[2], poison[3]], ["random", 1, "random", "whole", "random"], seed=6,
         slots=[6, 8, 7, 0, 31])
    assert full(dec, 7) == full(want, 0)
    assert check_alignment(dec, 7, flat_list(g), ll) == 45
    for slot, x in zip((6, 8, 0, 31), poison):                # the neighbours are still themselves
        check_alignment(dec, slot, flat_list(g), x)


def test_a_slot_out_of_records_then_reopened(tmp_path):
    # test_full_arena_ends_one_slot_only with the mode on: slot 0 runs out of trace records, slot 1 goes on
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    fst, am = pk.Fst(write_graph(tmp_path, "w.fst", g)), ident_model(g["num_tids"])
    good = SG.planted(g, 40, seed=1, bonus=30.0, noise=0.5)[0]
    bad = SG.flat(good.shape[0], g["num_tids"], seed=2)
    want = batch(fst, am, [good])
    dec = online(fst, am, 2, cap=600)
    codes = feed(dec, [bad, good], [1, 1], tolerate=(E_CAPACITY,))
    assert codes and set(codes) == {E_CAPACITY}
    assert dec.result(0)[2] == 0 and all(len(a) == 0 for a in dec.alignment(0)) and dec.word_segments(0) == []
    assert 0 <= dec.num_frames(0) < bad.shape[0]
    assert full(dec, 1) == full(want, 0)
    # the slot that ended, reopened: a healthy utterance, then (slot reuse) a second one
    for seed, utt in enumerate((good, SG.planted(g, 25, seed=4, bonus=30.0, noise=0.5)[0])):
        assert feed(dec, [utt], ["random"], seed=seed, slots=[0]) == []
        assert full(dec, 0) == full(batch(fst, am, [utt]), 0), seed
        assert dec.result(0)[2] == 1 and check_alignment(dec, 0, flat_list(g), utt) == utt.shape[0]
    assert full(dec, 1) == full(want, 0)                       # (and the neighbour's finished result stays readable)


def test_a_reopened_slot_is_empty_until_its_own_first_launch(tmp_path):
    # Slot 0 finishes an utterance and is opened again; then only slot 1 advances.  Slot 0 has not been launched since
    # its open, so it reports nothing of its previous utterance -- with the mode on and with it off.
    g = all_final(SG.general(150, 7400, k=2, eps_k=12))
    fst, am = pk.Fst(write_graph(tmp_path, "g.fst", g)), ident_model(g["num_pdfs"])
    lls = [SG.dyadic(20, g["num_pdfs"], 80 + u, k=2) for u in range(2)]
    arcs = flat_list(g)
    for align in (True, False):
        dec = online(fst, am, 2, align)
        feed(dec, [lls[0]], ["whole"], slots=[0])
        assert dec.num_frames(0) == 20 and dec.result(0)[2] == 1 and dec.word_segments(0)
        dec.open(0)
        dec.open(1)
        for sync in (True, False):
            dec.advance_host({1: (lls[1][:5] if sync else lls[1][5:9], False)}, sync=sync)
            dec.synchronize()
            assert dec.num_frames(1) == (5 if sync else 9)
            assert dec.num_frames(0) == 0 and dec.best_path_arcs(0) == [] and dec.partial(0) == ([], 0.0)
            assert dec.word_segments(0) == []
            if align:
                assert all(len(a) == 0 for a in dec.alignment(0))
        dec.advance_host({0: (lls[1][:0], False), 1: (lls[1][9:12], False)})         # slot 0's first launch: no frame yet
        assert dec.num_frames(0) == 0 and dec.num_frames(1) == 12
        if align:
            assert all(len(a) == 0 for a in dec.alignment(0))
        dec.advance_host({0: (lls[1], True), 1: (lls[1][12:], True)})
        assert outcome(dec, 0) == outcome(dec, 1) and dec.num_frames(0) == 20
        if align:
            assert full(dec, 0) == full(dec, 1) and check_alignment(dec, 0, arcs, lls[1]) == 20


# ---------------------------------------------------------------- 6: mode rules

def test_mode_rules(tmp_path):
    g = all_final(SG.general(150, 7400, k=2, eps_k=12))
    fst, am = pk.Fst(write_graph(tmp_path, "g.fst", g)), ident_model(g["num_pdfs"])
    ll = SG.dyadic(20, g["num_pdfs"], 80, k=2)
    dec = pk.OnlineDecoder(fst, am, 2, trace_capacity=TRACE)
    with pytest.raises(pk.PkCodeError) as e:                   # off by default
        dec.alignment(0)
    assert e.value.code == E_STATE and "alignment is off" in str(e.value)
    dec.open(1)
    for on in (True, False):
        with pytest.raises(pk.PkCodeError) as e:
            dec.set_alignment(on)
        assert e.value.code == E_STATE and "slot 1 is open" in str(e.value)
    dec.advance_host({1: (ll, True)})
    plain = outcome(dec, 1)
    assert all(math.isnan(s.acoustic_cost) for s in dec.word_segments(1)) and dec.word_segments(1)
    dec.set_alignment(True)
    with pytest.raises(pk.PkCodeError) as e:                   # the slot was decoded with the mode off
        dec.alignment(1)
    assert e.value.code == E_STATE
    assert outcome(dec, 1) == plain                            # (its results stay readable)
    feed(dec, [ll], ["random"], slots=[1])
    assert outcome(dec, 1) == plain and check_alignment(dec, 1, flat_list(g), ll) == 20
    with_costs = got_segments(dec, 1)
    dec.set_alignment(False)
    with pytest.raises(pk.PkCodeError) as e:
        dec.alignment(1)
    assert e.value.code == E_STATE
    feed(dec, [ll], ["random"], slots=[1])                     # toggled off again: NaN costs as before
    segs = dec.word_segments(1)
    assert outcome(dec, 1) == plain and segs and all(math.isnan(s.acoustic_cost) for s in segs)
    assert [(s.word, s.start_frame, s.num_frames, bits(s.graph_cost)) for s in segs] == [w[:4] for w in with_costs]
