"""The best-path alignment (AlignKernel in csrc/decode.hip, queued by csrc/capi_decoder.hip:
pk_mi355_decoder_set_alignment / _alignment / _word_segments): per frame the emitting arc of the best path, its transition-id and its acoustic cost; per word a
segment with its frames and its two costs.  Every expectation is a Python restatement over best_path_arcs, the graph's
arcs as the test wrote them and the host log-likelihoods -- never the code under test: arc ids are the path's emitting
arcs in order, acoustic costs the bit patterns of -N1(ll[t, pdf]), segments the rule of include/pk_mi355.h with sums
in double rounded to float once."""
import os
import struct

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth_graph as SG

from test_gpu_decode import flat_arcs, ident_model, write_graph
from test_gpu_decode_edges import GRIDS, NANS, PDF, flat_list, graph, outcome, ragged_waves
from test_gpu_decoder import G

pytestmark = pytest.mark.gpu
TRACE = 1 << 20
E_INVALID, E_STATE = -1, -4
INF = np.inf
BLOCK = 512                                     # kDecThreads: AlignKernel walks a path in chunks of this many arcs


def bits(x):
    return struct.unpack("<I", np.float32(x).tobytes())[0]


def restate(arcs, path, ll, pdf_of):
    """arcs: (next, ilabel, olabel, weight) by arc id; path: arc ids; ll: [T][num_pdfs] host log-likelihoods.
    -> (arc ids, transition-ids, acoustic costs as float32, segments as (word, start, frames, graph bits, acoustic bits))"""
    ids, tids, ac = [], [], []
    for a in path:
        il = arcs[a][1]
        if il:
            x = ll[len(ids), pdf_of(il)]
            x = np.float32(-np.inf) if np.isnan(x) else np.float32(x)             # N1
            ids.append(a)
            tids.append(il)
            ac.append(np.float32(-x))
    segs, cur, frame = [], None, 0
    for a in path:
        _, il, ol, w = arcs[a]
        if ol or cur is None:
            if cur is not None:
                segs.append(cur)
            cur = [ol, frame, 0, 0.0, 0.0]
        cur[3] += float(np.float32(w))
        if il:
            cur[4] += float(ac[frame])
            cur[2] += 1
            frame += 1
    if cur is not None:
        segs.append(cur)
    return ids, tids, np.array(ac, np.float32), [(s[0], s[1], s[2], bits(s[3]), bits(s[4])) for s in segs]


def got_segments(dec, u):
    return [(s.word, s.start_frame, s.num_frames, bits(s.graph_cost), bits(s.acoustic_cost)) for s in dec.word_segments(u)]


def check_alignment(dec, u, arcs, ll, pdf_of=PDF):
    """Utterance u of dec's last call against the restatement.  -> the frames aligned."""
    words, weight, ok = dec.result(u)
    path = dec.best_path_arcs(u)
    ids, tids, ac = dec.alignment(u)
    if not ok or not path:
        assert len(ids) == len(tids) == len(ac) == 0 and dec.word_segments(u) == [], u
        return 0
    want_ids, want_tids, want_ac, want_segs = restate(arcs, path, ll, pdf_of)
    assert len(want_ids) == ll.shape[0], u                                       # one emitting arc per frame
    assert ids.tolist() == want_ids and tids.tolist() == want_tids, u
    assert ac.tobytes() == want_ac.tobytes(), u
    segs = got_segments(dec, u)
    assert segs == want_segs, u
    assert [s[0] for s in segs if s[0]] == words, u
    assert sum(s[2] for s in segs) == ll.shape[0] and all(s[1] == sum(p[2] for p in segs[:i]) for i, s in enumerate(segs)), u
    return len(ids)


def decoder(tmp_path, g, max_utts, name="g.fst", trace=TRACE, gc=False, align=True):
    path = write_graph(tmp_path, name, g)
    dec = pk.Decoder(pk.Fst(path), ident_model(g["num_pdfs"]), max_utts, trace_capacity=trace, trace_gc=gc)
    if align:
        dec.set_alignment(True)
    return dec


# ---------------------------------------------------------------- general graphs, both grids

@pytest.mark.parametrize("grid", ["coarse", "fine"])
def test_general_graphs(tmp_path, grid):
    k, eps_k = GRIDS[grid]
    aligned = 0
    for seed in range(3):
        g = SG.general(150 + 50 * seed, 7000 + seed, k=k, eps_k=eps_k)
        g["final"][:] = np.where(np.isinf(g["final"]), np.float32(2.0), g["final"])    # every state final: a path for every utterance
        lls = [SG.dyadic(30 + 10 * u, g["num_pdfs"], 90 * seed + u, k=k) for u in range(4)]
        dec = decoder(tmp_path, g, len(lls), "g%d.fst" % seed)
        dec.decode(lls)
        arcs = flat_list(g)
        for u, ll in enumerate(lls):
            assert dec.result(u)[2] == 1 and dec.best_path_arcs(u)
            aligned += check_alignment(dec, u, arcs, ll)
            if grid == "coarse":               # every sum is exact on this grid: the two cost halves and the final weight, counted
                segs = dec.word_segments(u)    # twice as BestPath counts it, are the hypothesis' weight
                end = arcs[dec.best_path_arcs(u)[-1]][0]
                total = sum(float(s.graph_cost) for s in segs) + sum(float(s.acoustic_cost) for s in segs) + 2.0 * float(g["final"][end])
                assert total == float(dec.result(u)[1]), (seed, u)
    assert aligned == 3 * (30 + 40 + 50 + 60)


# ---------------------------------------------------------------- chunk edges

def chain(length, eps, olabel_every=7):
    """One path of `length` arcs 0 -> 1 -> ... -> length; the arcs in `eps` are epsilon arcs, every olabel_every-th
    arc (epsilon or not) carries a word."""
    arcs, tid = [], 0
    for i in range(length):
        il = 0 if i in eps else 1 + tid % 7
        tid += 1
        arcs.append([(i + 1, il, (1 + i // olabel_every) if i % olabel_every == 0 else 0, 0.25 * (i % 5))])
    arcs.append([])
    return graph([INF] * length + [0.5], arcs)


@pytest.mark.parametrize("length", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1])
def test_paths_around_the_chunk_size(tmp_path, length):
    # epsilon arcs first, last, and in runs that straddle the first and the second chunk boundary
    eps = {0, length - 1} | set(range(BLOCK - 6, BLOCK + 7)) | set(range(2 * BLOCK - 3, 2 * BLOCK + 4))
    eps = {i for i in eps if i < length}
    g = chain(length, eps)
    T = length - len(eps)
    lls = [SG.dyadic(T, 8, length + u, k=2) for u in range(2)]
    dec = decoder(tmp_path, g, 2)
    dec.decode(lls)
    arcs = flat_list(g)
    for u, ll in enumerate(lls):
        assert dec.best_path_arcs(u) == list(range(length))
        assert check_alignment(dec, u, arcs, ll) == T
        assert dec.alignment(u)[0].tolist() == [i for i in range(length) if i not in eps]


def test_zero_frames_on_an_epsilon_path_and_one_frame(tmp_path):
    # T = 0: the start closure reaches the only final state over three epsilon arcs, two of them with words
    g = graph([INF, INF, INF, 0.25, 0.0], [[(1, 0, 4, 0.5)], [(2, 0, 0, 0.25)], [(3, 0, 5, 0.125), (4, 1, 6, 0.5)], [], []])
    dec = decoder(tmp_path, g, 2)
    one = SG.dyadic(1, 8, 3, k=2)
    dec.decode([np.zeros((0, 8), np.float32), one])
    assert dec.result(0)[0] == [4, 5] and dec.best_path_arcs(0) == [0, 1, 2]
    ids, tids, ac = dec.alignment(0)
    assert len(ids) == len(tids) == len(ac) == 0
    assert got_segments(dec, 0) == [(4, 0, 0, bits(0.75), bits(0.0)), (5, 0, 0, bits(0.125), bits(0.0))]
    # T = 1: one emitting arc, the last of the path
    assert dec.best_path_arcs(1) == [0, 1, 3]
    assert check_alignment(dec, 1, flat_list(g), one) == 1
    assert dec.alignment(1)[0].tolist() == [3] and dec.alignment(1)[1].tolist() == [1]


# ---------------------------------------------------------------- a ragged batch of 32

def test_ragged_batch_of_32(tmp_path):
    g = SG.general(200, 7100, k=2, eps_k=12)
    g["final"][:] = np.where(np.isinf(g["final"]), np.float32(1.0), g["final"])
    rng = np.random.default_rng(11)
    lls = [SG.dyadic(int(rng.integers(1, 61)), g["num_pdfs"], 400 + u, k=2) for u in range(32)]
    lls[0] = np.zeros((0, g["num_pdfs"]), np.float32)                            # no frame at all
    lls[5] = lls[5].copy()
    lls[5][min(4, len(lls[5]) - 1), :] = NANS[0]                                 # N2: ok = 0
    dec = decoder(tmp_path, g, 32)
    dec.decode(lls)
    arcs = flat_list(g)
    assert dec.result(5) == ([], 0.0, 0) and len(dec.alignment(5)[0]) == 0 and dec.word_segments(5) == []
    assert len(dec.alignment(0)[0]) == 0
    frames = [check_alignment(dec, u, arcs, ll) for u, ll in enumerate(lls)]     # every utterance against ITS log-likelihoods:
    assert frames == [0 if u in (0, 5) else ll.shape[0] for u, ll in enumerate(lls)]   # a wrong offset reads a neighbour's
    # the same utterances in another order and another batch size land at other offsets and give the same
    order = [31 - u for u in range(0, 32, 3)]
    dec.decode([lls[u] for u in order])
    for i, u in enumerate(order):
        assert check_alignment(dec, i, arcs, lls[u]) == frames[u]


def test_negative_epsilon_cycle_then_a_healthy_call(tmp_path):
    # the graph of test_reuse_after_negative_epsilon_cycle: the cycle 3 -> 4 -> 3 is reached only through pdf 2
    g = graph([INF, 0.0, 0.0, INF, INF],
              [[(1, 1, 1, 0.5), (2, 2, 2, 0.5), (0, 3, 0, 1.0)],
               [(1, 1, 0, 0.25), (0, 3, 3, 0.5), (0, 0, 0, 0.5)],
               [(3, 0, 0, 0.25), (2, 1, 0, 0.25)],
               [(4, 0, 0, -0.5), (2, 1, 0, 0.0)],
               [(3, 0, 0, 0.0)]])
    dec = decoder(tmp_path, g, 3)
    with pytest.raises(pk.PkError) as e:
        dec.decode([SG.dyadic(6, 8, 7, k=2)])
    assert e.value.code == E_INVALID and "negative epsilon cycle" in str(e.value)
    with pytest.raises(pk.PkError):
        dec.alignment(0)
    healthy = []
    for u in range(3):
        ll = SG.dyadic(6 + u, 8, u, k=2)
        ll[:, 2] = -np.inf
        healthy.append(ll)
    dec.decode(healthy)
    for u, ll in enumerate(healthy):
        assert dec.result(u)[2] == 1 and check_alignment(dec, u, flat_list(g), ll) == ll.shape[0]


# ---------------------------------------------------------------- non-finite log-likelihoods

def test_all_infinite_last_frame(tmp_path):
    g = SG.general(120, 4200, k=2, eps_k=12)
    lls = []
    for u, value in enumerate((np.float32(-np.inf), NANS[0], NANS[1])):
        ll = SG.dyadic(9, g["num_pdfs"], 9 + u, k=2)
        ll[-1, :] = value
        lls.append(ll)
    dec = decoder(tmp_path, g, len(lls))
    dec.decode(lls)
    for u in range(len(lls)):
        assert dec.result(u) == ([], 0.0, 1) and dec.best_path_arcs(u) == []
        assert len(dec.alignment(u)[0]) == 0 and dec.word_segments(u) == []


def test_nan_off_the_path_changes_nothing(tmp_path):
    # No pruning (beam inf) and a grid where ties are rare: worsening candidates that are not on the best path cannot
    # change it.  Every frame gets NaN or -inf on pdfs the path does not read at that frame.
    k, eps_k = GRIDS["fine"]
    g = SG.general(100, 7200, k=k, eps_k=eps_k)
    g["final"][:] = np.where(np.isinf(g["final"]), np.float32(1.0), g["final"])
    clean = [SG.dyadic(40, g["num_pdfs"], 30 + u, k=k) for u in range(3)]
    dec = decoder(tmp_path, g, 3)
    dec.set_beam(np.inf, 1 << 30)
    dec.decode(clean)
    arcs = flat_list(g)
    before = [(outcome(dec, u)[:4], [a.tobytes() for a in dec.alignment(u)], got_segments(dec, u)) for u in range(3)]
    dirty = []
    for u, ll in enumerate(clean):
        assert check_alignment(dec, u, arcs, ll) == 40
        on_path = dec.alignment(u)[1]                                             # identity map: the pdf read at each frame
        x, rng = ll.copy(), np.random.default_rng(u)
        for t in range(40):
            for p in rng.choice([p for p in range(g["num_pdfs"]) if p != on_path[t]], 3, replace=False):
                x[t, p] = (NANS[0], NANS[1], np.float32(-np.inf))[int(rng.integers(3))]
        dirty.append(x)
    dec.decode(dirty)
    for u, ll in enumerate(dirty):
        assert check_alignment(dec, u, arcs, ll) == 40
        assert (outcome(dec, u)[:4], [a.tobytes() for a in dec.alignment(u)], got_segments(dec, u)) == before[u], u


# ---------------------------------------------------------------- trace gc

def test_trace_gc_gives_the_same_alignment(tmp_path):
    g = SG.general(300, 7300, k=2, eps_k=12)
    g["final"][:] = np.where(np.isinf(g["final"]), np.float32(1.0), g["final"])
    lls = [SG.dyadic(60 + 5 * u, g["num_pdfs"], 60 + u, k=2) for u in range(4)]
    arcs, n = flat_list(g), len(lls)
    off = decoder(tmp_path, g, n)
    off.decode(lls)
    roomy = decoder(tmp_path, g, n, trace=0, gc=True)
    roomy.decode(lls)
    wrote = [roomy.trace_stats(u)[0] for u in range(n)]
    on = None
    for shift in (2, 1, 0):                       # the smallest of these slices the call fits in (test_gpu_decode_gc.tightest)
        size = (max(wrote) >> shift) + 1
        try:
            on = decoder(tmp_path, g, n, trace=size * n, gc=True)
            on.decode(lls)
            break
        except pk.PkError as e:
            assert shift > 0 and e.code == -6, str(e)
    compactions = sum(on.trace_stats(u)[2] for u in range(n))
    assert compactions >= 1, (wrote, size)
    for u, ll in enumerate(lls):
        assert check_alignment(on, u, arcs, ll) == check_alignment(off, u, arcs, ll) == ll.shape[0]
        assert outcome(on, u) == outcome(off, u) == outcome(roomy, u)
        for a, b, c in zip(on.alignment(u), off.alignment(u), roomy.alignment(u)):
            assert a.tobytes() == b.tobytes() == c.tobytes()
        assert got_segments(on, u) == got_segments(off, u) == got_segments(roomy, u)


# ---------------------------------------------------------------- the two entry points

def test_decode_batch_equals_decode_of_its_fetch_all():
    from refmodel_text import DIR, load_text_model
    layers, prior, Lc, Rc, tid2pdf, cmvn41 = load_text_model()
    am = pk.AcousticModel(layers, prior, Lc, Rc, tid2pdf)
    waves = [pk.read_wav(os.path.join(G, w)) for w in ("en-us-hello.wav", "en-us-cat.wav")] + ragged_waves()[:6]
    bs = pk.BatchScorer(am, cmvn41, len(waves), sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    fst_path = os.path.join(DIR, "wordloop.fst")
    fst = pk.Fst(fst_path)
    dec = pk.Decoder(fst, am, 16, trace_capacity=TRACE)                # more slots than the batch
    dec.set_alignment(True)
    dec.decode_batch(bs)
    lls = [v.log_prob() for v in bs.fetch_all()]
    host = pk.Decoder(fst, am, len(waves), trace_capacity=TRACE)
    host.set_alignment(True)
    host.decode(lls)
    arcs = flat_arcs(fst_path)
    assert lls[2].shape[0] == 0                                          # the 300-sample wave
    for u, ll in enumerate(lls):
        assert outcome(dec, u) == outcome(host, u), u
        assert check_alignment(dec, u, arcs, ll, lambda t: int(tid2pdf[t])) == check_alignment(host, u, arcs, ll, lambda t: int(tid2pdf[t]))
        for a, b in zip(dec.alignment(u), host.alignment(u)):
            assert a.tobytes() == b.tobytes()
        assert got_segments(dec, u) == got_segments(host, u)
    assert len(dec.alignment(0)[0]) == lls[0].shape[0] > 0 and dec.result(0)[0]


# ---------------------------------------------------------------- mode off

def test_mode_off_and_toggling(tmp_path):
    g = SG.general(150, 7400, k=2, eps_k=12)
    g["final"][:] = np.where(np.isinf(g["final"]), np.float32(1.0), g["final"])
    lls = [SG.dyadic(20 + u, g["num_pdfs"], 80 + u, k=2) for u in range(3)]
    arcs = flat_list(g)
    dec = decoder(tmp_path, g, 3, align=False)
    dec.decode(lls)
    plain = [outcome(dec, u) for u in range(3)]
    for call in (dec.alignment, dec.word_segments):
        with pytest.raises(pk.PkError) as e:
            call(0)
        assert e.value.code == E_STATE and "alignment off" in str(e.value)
    dec.set_alignment(True)
    with pytest.raises(pk.PkError) as e:          # the mode of the call that ran, not of the next one
        dec.alignment(0)
    assert e.value.code == E_STATE
    dec.decode(lls)
    for u, ll in enumerate(lls):
        assert outcome(dec, u) == plain[u]
        assert check_alignment(dec, u, arcs, ll) == ll.shape[0]
    dec.set_alignment(False)
    dec.decode(lls)
    assert [outcome(dec, u) for u in range(3)] == plain
    with pytest.raises(pk.PkError) as e:
        dec.word_segments(1)
    assert e.value.code == E_STATE
    dec.set_alignment(True)
    dec.decode(lls[::-1])
    for u, ll in enumerate(lls[::-1]):
        assert check_alignment(dec, u, arcs, ll) == ll.shape[0]
