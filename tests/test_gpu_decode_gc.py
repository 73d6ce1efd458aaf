"""The batch decoder with trace gc on (pk_mi355_decoder_set_trace_gc in csrc/capi_decoder.hip, DecodeKernel<true> in
csrc/decode.hip): every utterance of a call owns trace_capacity // n backtrace records and compacts them as they fill.  Where the records
live must never show: words, weight bits, ok, best-path arcs and active_bound equal the mode-off decoder's, the host
model's (tests/decoder_model.py) and, where built, the reference decoder's -- at capacities the shared arena cannot
decode at all.  "Same" below is outcome() of test_gpu_decode_edges: all five."""
import os

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth_graph as SG

import decoder_model as M
from test_gpu_decode import HAVE_REF, ident_model, ref_decode, write_graph
from test_gpu_decode_edges import GRIDS, NANS, PDF, expect, graph, max_active_graph, outcome, with_ids
from test_gpu_decoder import G

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE, E_CAPACITY = -1, -4, -6
DEFAULT_TRACE = 1 << 27
INF = np.inf


def run(fst, am, lls, beam=16.0, max_active=30000, cap=0, gc=False, max_utts=None):
    dec = pk.Decoder(fst, am, max_utts or max(len(lls), 1), trace_capacity=cap, trace_gc=gc)
    dec.set_beam(beam, max_active)
    dec.decode(lls)
    return dec


def outcomes(dec, n):
    return [outcome(dec, u) for u in range(n)]


def stats(dec, n):
    return [dec.trace_stats(u) for u in range(n)]


def records_written(decode, n):
    """What each utterance of a call writes: decode(trace_capacity) -> a trace-gc decoder after the call.  At the default
    capacity a slice holds every record, nothing is compacted, and the high-water mark is the count."""
    roomy = decode(0)
    st = stats(roomy, n)
    assert all(s == DEFAULT_TRACE // n and c == 0 and p <= s for p, s, c in st)
    return roomy, [p for p, _, _ in st]


def tightest(decode, wrote, n, extra=0):
    """The smallest slice of max(wrote) / 8, / 4, / 2, / 1 (+ 1) records the call fits in (the last one holds all an
    utterance writes, so it always does); the smaller ones must end in PK_MI355_E_CAPACITY "after compaction".  How
    small a slice can be depends on what stays reachable (beam 0 keeps one path, and every record on it, alive), so
    the slice is searched, not derived; what is asserted is that results do not depend on it.
    -> (decoder, slice records)."""
    for shift in (3, 2, 1, 0):
        size = (max(wrote) >> shift) + 1
        try:
            dec = decode(size * n + extra)
        except pk.PkError as e:
            assert shift > 0 and e.code == E_CAPACITY and "after compaction" in str(e), (shift, str(e))
            continue
        st = stats(dec, n)
        assert all(s == size and p <= s for p, s, _ in st), st
        # an utterance that wrote more than its slice holds was compacted
        assert all(c >= 1 for w, (_, _, c) in zip(wrote, st) if w > size), (wrote, st)
        return dec, size


def check_model(tmp_path, g, lls, beam, max_active, name, extra=0):
    """Mode on at the tightest slice against the host model and against mode off.  -> compactions of the call."""
    path = write_graph(tmp_path, name, g)
    fst, am = pk.Fst(path), ident_model(g["num_pdfs"])
    n = len(lls)
    off = run(fst, am, lls, beam, max_active)
    _, wrote = records_written(lambda cap: run(fst, am, lls, beam, max_active, cap, True), n)
    assert sum(wrote) == off.trace_stats(0)[0]
    dec, _ = tightest(lambda cap: run(fst, am, lls, beam, max_active, cap, True), wrote, n, extra)
    fstm = with_ids(g)
    for u, ll in enumerate(lls):
        assert outcome(dec, u) == outcome(off, u), u
        expect(dec, u, g, ll, M.decode(fstm, ll, PDF, beam=beam, max_active=max_active), path)
    return sum(c for _, _, c in stats(dec, n))


# ---------------------------------------------------------------- 1. where the shared arena overflows

def test_word_loop_decodes_where_the_shared_arena_overflows(tmp_path):
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    fst = pk.Fst(write_graph(tmp_path, "w.fst", g))
    am = ident_model(g["num_tids"])
    lls = ([SG.planted(g, T, seed=s)[0] for s, T in enumerate((150, 1500, 1800, 2100))] +
           [SG.flat(150, g["num_tids"], seed=9)])
    n = len(lls)
    off = run(fst, am, lls)
    want = outcomes(off, n)
    total, size, c = off.trace_stats(0)
    assert (size, c) == (DEFAULT_TRACE, 0) and all(off.trace_stats(u) == (total, size, c) for u in range(n))
    roomy, wrote = records_written(lambda cap: run(fst, am, lls, cap=cap, gc=True), n)
    assert outcomes(roomy, n) == want and sum(wrote) == total
    # The capacity, from what mode off reports: active_bound x frames is the scale of an utterance's records (a frame
    # writes a record per winner, and per state the closure improves).  A slice is a 24th of the mean of that: a
    # fraction of what the long utterances write.  It must still hold twice what the flat utterance keeps reachable
    # plus one of its frames -- nearly all of the graph survives each of its frames, and a token's chain only joins
    # the others' a few frames back -- so, asserted, it is more than 12 of the largest per-frame count.
    bounds = [w[4] for w in want]
    records = sum(b * ll.shape[0] for b, ll in zip(bounds, lls))
    size = records // 24 // n
    cap = size * n
    print("bounds", bounds, "records bound", records, "wrote", wrote, "slice", size)
    assert max(bounds) * 12 < size
    with pytest.raises(pk.PkError) as e:                                   # (a) the shared arena cannot
        run(fst, am, lls, cap=cap)
    assert e.value.code == E_CAPACITY and "after compaction" not in str(e.value)
    on = run(fst, am, lls, cap=cap, gc=True)                               # (b) the slices can
    st = stats(on, n)
    print("stats", st)
    assert outcomes(on, n) == want
    over = [u for u in range(n) if wrote[u] > size]
    assert len(over) >= 4 and 0 not in over                                # all but the short one
    for u in range(n):
        peak, s, c = st[u]
        assert s == size and peak <= s                                     # (d)
        if u in over:
            assert c >= 2, (u, st[u], wrote[u])                            # (c)


# ---------------------------------------------------------------- 2. the host model

@pytest.mark.parametrize("grid", ["coarse", "fine"])
def test_general_graphs_match_the_model_while_compacting(tmp_path, grid):
    k, eps_k = GRIDS[grid]
    for seed, beam in enumerate([INF, 0.0, 4.0, 16.0, 2.0]):
        g = SG.general(100 + 50 * seed, 7000 + seed, k=k, eps_k=eps_k)
        lls = [SG.dyadic(T, g["num_pdfs"], 11 * seed + u, k=k) for u, T in enumerate((160, 5, 90, 1, 230))]
        c = check_model(tmp_path, g, lls, beam, 1 << 30 if beam == INF else 30000, "g%d.fst" % seed, extra=seed)
        print(grid, "beam", beam, "compactions", c)
        assert c > 0, beam                                 # at every beam the slices were small enough to compact


def test_max_active_binding_matches_the_model_while_compacting(tmp_path):
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    g["num_pdfs"] = g["num_tids"]
    lls = [SG.flat(40, g["num_tids"], seed=s) for s in range(4)]
    off = run(pk.Fst(write_graph(tmp_path, "w.fst", g)), ident_model(g["num_tids"]), lls, 16.0, 256)
    assert min(off.active_bound(u) for u in range(4)) > 256                # it binds
    assert check_model(tmp_path, g, lls, 16.0, 256, "w256.fst") > 0
    for case in ("negative", "straddle", "shared"):
        n = 40
        small, slls = max_active_graph(case, n)
        # max_active_graph's three frames, then nine more around the third layer's self-loops: frame 1 still starts
        # with exactly n tokens, and the call is long enough that the tightest slice fills more than once
        slls = [np.vstack([ll, SG.dyadic(9, 8, 200 + s, k=2, lo=-2.0, hi=0.0)]) for s, ll in enumerate(slls)]
        for ma in (n - 1, n, n + 1):
            assert check_model(tmp_path, small, slls, 8.0, ma, "%s%d.fst" % (case, ma), extra=1) > 0, (case, ma)


def test_the_inputs_the_shared_arena_fails_on_decode_with_slices(tmp_path):
    """test_gpu_decode_edges.test_reuse_after_trace_capacity_exhausted's call (healthy + [big], capacity 20000, beam
    inf), which mode off ends with PK_MI355_E_CAPACITY."""
    g = SG.general(200, 5000, k=2, eps_k=12)
    g["final"][:] = 0.0
    healthy = [SG.dyadic(3, g["num_pdfs"], u, k=2) for u in range(3)]
    big = SG.dyadic(400, g["num_pdfs"], 9, k=2)
    lls = healthy + [big]
    path = write_graph(tmp_path, "g.fst", g)
    fst, am = pk.Fst(path), ident_model(g["num_pdfs"])
    with pytest.raises(pk.PkError) as e:
        run(fst, am, lls, INF, 1 << 30, cap=20000)
    assert e.value.code == E_CAPACITY
    dec = run(fst, am, lls, INF, 1 << 30, cap=20000, gc=True)
    st = stats(dec, 4)
    print("stats", st)
    assert st[3][1] == 5000 and st[3][2] >= 2
    fstm = with_ids(g)
    for u, ll in enumerate(lls):
        expect(dec, u, g, ll, M.decode(fstm, ll, PDF, beam=INF, max_active=1 << 30), path)


# ---------------------------------------------------------------- 3. edges with the mode on

def test_ragged_batch_smaller_than_the_decoder_and_a_capacity_n_does_not_divide(tmp_path):
    g = SG.general(300, 7100, k=12, eps_k=12)
    path = write_graph(tmp_path, "g.fst", g)
    fst, am = pk.Fst(path), ident_model(g["num_pdfs"])
    lls = [SG.dyadic(T, g["num_pdfs"], 40 + u, k=12) for u, T in enumerate((0, 1, 7, 40, 90, 130, 33))]
    n = len(lls)
    off = run(fst, am, lls, max_utts=16)
    _, wrote = records_written(lambda cap: run(fst, am, lls, cap=cap, gc=True, max_utts=16), n)
    dec, size = tightest(lambda cap: run(fst, am, lls, cap=cap, gc=True, max_utts=16), wrote, n, extra=n - 2)
    assert (size * n + n - 2) % n and (size * n + n - 2) // 16 < size      # n, not max_utts, divides the arena
    assert sum(c for _, _, c in stats(dec, n)) > 0
    fstm = with_ids(g)
    for u, ll in enumerate(lls):
        assert outcome(dec, u) == outcome(off, u), u
        expect(dec, u, g, ll, M.decode(fstm, ll, PDF), path)
    assert dec.result(0)[2] == 1 and dec.best_path_arcs(0) == off.best_path_arcs(0)        # T = 0
    # fewer utterances on the same decoder: larger slices
    dec.decode(lls[4:6])
    assert [dec.trace_stats(u)[1] for u in range(2)] == [(size * n + n - 2) // 2] * 2
    assert outcomes(dec, 2) == [outcome(off, 4), outcome(off, 5)]
    dec.decode([])
    with pytest.raises(pk.PkError):
        dec.trace_stats(0)


def test_poisoned_utterances_in_a_batch_of_32(tmp_path):
    g = SG.size_for_states(20000, seed=23)
    fst = pk.Fst(write_graph(tmp_path, "g.fst", g))
    am = ident_model(g["num_tids"])
    lls = [SG.planted(g, 120 + 9 * u, seed=300 + u)[0] for u in range(32)]
    lls[7] = lls[7].copy()
    lls[7][4, :] = NANS[0]                                 # N2: a row without a finite cell ends the utterance
    lls[20] = lls[20].copy()
    lls[20][np.random.default_rng(1).random(lls[20].shape) < 0.05] = NANS[1]      # N1: NaN cells decode as -inf
    off = run(fst, am, lls)
    assert off.result(7) == ([], 0.0, 0) and off.result(20)[2] == 1
    _, wrote = records_written(lambda cap: run(fst, am, lls, cap=cap, gc=True), 32)
    dec, size = tightest(lambda cap: run(fst, am, lls, cap=cap, gc=True), wrote, 32)
    st = stats(dec, 32)
    assert sum(c for _, _, c in st) > 0 and st[7][2] == 0
    for u in range(32):
        assert outcome(dec, u) == outcome(off, u), u


def test_negative_epsilon_cycle_then_a_healthy_call(tmp_path):
    g = graph([INF, 0.0, 0.0, INF, INF],
              [[(1, 1, 1, 0.5), (2, 2, 2, 0.5), (0, 3, 0, 1.0)],
               [(1, 1, 0, 0.25), (0, 3, 3, 0.5), (0, 0, 0, 0.5)],
               [(3, 0, 0, 0.25), (2, 1, 0, 0.25)],
               [(4, 0, 0, -0.5), (2, 1, 0, 0.0)],
               [(3, 0, 0, 0.0)]])
    healthy = []
    for u in range(3):
        ll = SG.dyadic(60 + u, 8, u, k=2)
        ll[:, 2] = -np.inf
        healthy.append(ll)
    poisoned = SG.dyadic(6, 8, 7, k=2)
    path = write_graph(tmp_path, "g.fst", g)
    fst, am = pk.Fst(path), ident_model(8)
    again = [healthy[2], healthy[0], healthy[1], healthy[1]]
    _, wrote = records_written(lambda cap: run(fst, am, again, cap=cap, gc=True), 4)
    tight, size = tightest(lambda cap: run(fst, am, again, cap=cap, gc=True), wrote, 4)
    assert all(c > 0 for _, _, c in stats(tight, 4))       # the healthy call compacts in every slot at this slice
    dec = pk.Decoder(fst, am, 4, trace_capacity=4 * size, trace_gc=True)
    with pytest.raises(pk.PkError) as e:
        dec.decode([healthy[0], poisoned, healthy[1], healthy[2]])
    assert e.value.code == E_INVALID and "negative epsilon cycle" in str(e.value) and "utterance 1" in str(e.value)
    dec.decode(again)
    assert stats(dec, 4) == stats(tight, 4)
    fresh = run(fst, am, again)
    fstm = with_ids(g)
    for u, ll in enumerate(again):
        assert outcome(dec, u) == outcome(fresh, u), u
        expect(dec, u, g, ll, M.decode(fstm, ll, PDF), path)
        assert dec.result(u)[2] == 1


# ---------------------------------------------------------------- 4. a slice too small

def test_a_slice_smaller_than_one_frame_fails_and_the_decoder_recovers(tmp_path):
    g = SG.general(200, 5000, k=2, eps_k=12)
    g["final"][:] = 0.0
    path = write_graph(tmp_path, "g.fst", g)
    fst, am = pk.Fst(path), ident_model(g["num_pdfs"])
    big = SG.dyadic(60, g["num_pdfs"], 9, k=2)
    empty, one, two = big[:0], big[:1], big[:2]
    _, (w0, w1, w2, wbig) = records_written(lambda cap: run(fst, am, [empty, one, two, big], INF, 1 << 30, cap, True), 4)
    size = wbig // 60 // 2             # half the mean of big's 60 frames: its largest frame alone does not fit
    assert w0 <= size                  # (InitDecoding's records do: the utterances without frames pass)
    K = 64
    cap = K * size + 5
    dec = pk.Decoder(fst, am, K, trace_capacity=cap, trace_gc=True)
    dec.set_beam(INF, 1 << 30)
    with pytest.raises(pk.PkError) as e:
        dec.decode([empty, big] + [empty] * (K - 2))
    msg = str(e.value)
    assert e.value.code == E_CAPACITY and "utterance 1:" in msg and "after compaction" in msg and "%d records" % size in msg
    with pytest.raises(pk.PkError) as e:
        dec.trace_stats(0)
    assert e.value.code == E_STATE
    healthy = [one, two]               # the failed slot again; two utterances share the arena: 32 times the slice
    assert w2 <= cap // 2
    dec.decode(healthy)
    fresh = pk.Decoder(fst, am, K, trace_capacity=cap, trace_gc=True)
    fresh.set_beam(INF, 1 << 30)
    fresh.decode(healthy)
    assert outcomes(dec, 2) == outcomes(fresh, 2) and stats(dec, 2) == stats(fresh, 2)
    assert [s for _, s, _ in stats(dec, 2)] == [cap // 2] * 2
    fstm = with_ids(g)
    for u, ll in enumerate(healthy):
        expect(dec, u, g, ll, M.decode(fstm, ll, PDF, beam=INF, max_active=1 << 30), path)


# ---------------------------------------------------------------- 5. decode_batch

@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_decode_batch_refmodel(precision):
    from refmodel_text import DIR, load_text_model
    layers, prior, Lc, Rc, tid2pdf, cmvn41 = load_text_model()
    fst_path = os.path.join(DIR, "wordloop.fst")
    waves = [pk.read_wav(os.path.join(G, w)) for w in ("en-us-hello.wav", "en-us-cat.wav")]
    am = pk.AcousticModel(layers, prior, Lc, Rc, tid2pdf, precision=precision)
    bs = pk.BatchScorer(am, cmvn41, 2, sum(len(w) for w in waves))
    bs.set_waves(waves)
    if precision != "f32":
        bs.calibrate()
    bs.score(0.1)
    fst = pk.Fst(fst_path)

    def decode(cap, gc=True):
        dec = pk.Decoder(fst, am, 2, trace_capacity=cap, trace_gc=gc)
        dec.decode_batch(bs, sync=False)
        dec.synchronize()
        return dec

    off = decode(0, gc=False)
    _, wrote = records_written(decode, 2)
    assert sum(wrote) == off.trace_stats(0)[0]
    dec, size = tightest(decode, wrote, 2, extra=1)
    st = stats(dec, 2)
    print("wrote", wrote, "stats", st)
    assert sum(c for _, _, c in st) > 0
    for u, v in enumerate(bs.fetch_all()):
        assert outcome(dec, u) == outcome(off, u), u
        if HAVE_REF:
            rw, rweight, rok = ref_decode(fst_path, v.log_prob(), am.handle)
            words, weight, ok = dec.result(u)
            assert (words, np.float32(weight).tobytes(), ok) == (rw, np.float32(rweight).tobytes(), rok) and len(words) >= 1


# ---------------------------------------------------------------- 6. toggling, and the statistics of each mode

def test_toggling_on_one_decoder(tmp_path):
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    fst = pk.Fst(write_graph(tmp_path, "w.fst", g))
    am = ident_model(g["num_tids"])
    lls = [SG.planted(g, 150, seed=s)[0] for s in range(3)]
    base = run(fst, am, lls)
    want = outcomes(base, 3)
    cap = base.trace_stats(0)[0] * 3 // 2                  # the shared arena fits; a slice is half of what the call writes
    dec = pk.Decoder(fst, am, 3, trace_capacity=cap)
    with pytest.raises(pk.PkError) as e:                   # nothing decoded yet
        dec.trace_stats(0)
    assert e.value.code == E_STATE
    dec.decode(lls)                                        # off by default
    assert outcomes(dec, 3) == want
    total = dec.trace_stats(0)[0]
    assert 0 < total <= cap and all(dec.trace_stats(u) == (total, cap, 0) for u in range(3))
    seen = []
    for on in (True, False, True):
        dec.set_trace_gc(on)
        dec.decode(lls)
        assert outcomes(dec, 3) == want, on
        st = stats(dec, 3)
        if on:
            assert all(s == cap // 3 and p <= s for p, s, _ in st)
            seen.append(st)
        else:
            assert st == [(total, cap, 0)] * 3
    assert seen[0] == seen[1]
    # the mode belongs to the call: set after a call was queued, it does not reach that call
    dec.set_trace_gc(False)
    dec.decode(lls, sync=False)
    dec.set_trace_gc(True)
    dec.synchronize()
    assert stats(dec, 3) == [(total, cap, 0)] * 3 and outcomes(dec, 3) == want
