"""The GPU decoder (kernels in csrc/decode.hip, host object in csrc/capi_decoder.hip) at its edges, against the host
model of its semantics (tests/decoder_model.py):
general graphs (synth_graph.general) in exact dyadic arithmetic -- a coarse grid where ties are everywhere and a
fine one where they are rare --, every tie rule, max-active at its boundaries, shapes that cross the 512-lane
chunks, beam 0 and beam inf, non-finite log-likelihoods (N1 / N2), reuse of a decoder after a
failed call, and decode_batch against decode.  Weight bits, ok and active_bound are compared for every input;
words and best-path arcs wherever the model says the path does not depend on the closure's order."""
import os

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth, synth_graph as SG

import decoder_model as M
from test_gpu_decode import HAVE_REF, check_self, ident_model, ref_decode, ref_decode_many, write_graph
from test_gpu_decoder import G

pytestmark = pytest.mark.gpu
TRACE = 1 << 22
PDF = lambda t: t          # noqa: E731  (identity tid2pdf)
GRIDS = {"coarse": (2, 12), "coarse_eps": (2, 2), "fine": (12, 12)}     # (k, eps_k): multiples of 2^-k


def with_ids(g):
    """The model's graph: arcs carry their file arc id."""
    by_state, k = [], 0
    for st in g["arcs"]:
        by_state.append([tuple(a) + (k + i,) for i, a in enumerate(st)])
        k += len(st)
    return g["start"], np.asarray(g["final"], np.float32), by_state


def flat_list(g):
    return [tuple(a) for st in g["arcs"] for a in st]


def no_nan(ll):
    return np.where(np.isnan(ll), np.float32(-np.inf), ll).astype(np.float32)


def gpu(tmp_path, g, lls, beam=16.0, max_active=30000, name="g.fst", trace=TRACE, max_utts=None):
    path = write_graph(tmp_path, name, g)
    dec = pk.Decoder(pk.Fst(path), ident_model(g["num_pdfs"]), max_utts or max(len(lls), 1), trace_capacity=trace)
    dec.set_beam(beam, max_active)
    dec.decode(lls)
    return dec, path


def outcome(dec, u):
    words, weight, ok = dec.result(u)
    return words, np.float32(weight).tobytes(), ok, dec.best_path_arcs(u), dec.active_bound(u)


def expect(dec, u, g, ll, want, path):
    words, weight, ok = dec.result(u)
    assert ok == want["ok"], u
    assert np.float32(weight).tobytes() == np.float32(want["weight"]).tobytes(), (u, weight, want["weight"])
    assert dec.active_bound(u) == want["active_bound"], u
    if want["determined"]:
        assert words == want["words"], u
        assert dec.best_path_arcs(u) == (want["path"] or []), u
    check_self(dec, u, path, no_nan(ll), PDF, g["final"], g["start"], flat_list(g))


def check(tmp_path, g, lls, beam=16.0, max_active=30000, **kw):
    """Decode lls on the GPU and compare every utterance with the model.  -> (decoder, the model's results)."""
    dec, path = gpu(tmp_path, g, lls, beam, max_active, **kw)
    fst = with_ids(g)
    wants = [M.decode(fst, ll, PDF, beam=beam, max_active=max_active) for ll in lls]
    for u, ll in enumerate(lls):
        expect(dec, u, g, ll, wants[u], path)
    return dec, wants


def graph(final, arcs_by_state, num_pdfs=8):
    return dict(start=0, final=np.array(final, np.float32), arcs=arcs_by_state, num_pdfs=num_pdfs)


INF = np.inf


# ---------------------------------------------------------------- random general graphs, both grids

@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_random_general_graphs(tmp_path, grid):
    k, eps_k = GRIDS[grid]
    det = n = 0
    for seed in range(12):
        rng = np.random.default_rng(1000 + seed)
        g = SG.general(int(rng.integers(10, 301)), 1000 + seed, k=k, eps_k=eps_k)
        lls = [SG.dyadic(int(rng.integers(0, 24)), g["num_pdfs"], 50 * seed + u, k=k) for u in range(5)]
        beam = [2.0, 4.0, 6.0, 16.0][seed % 4]
        _, wants = check(tmp_path, g, lls, beam=beam, name="g%d.fst" % seed)
        det += sum(w["determined"] for w in wants)
        n += len(wants)
    if grid != "coarse_eps":
        assert det >= 0.75 * n, (det, n)          # most paths are compared, not only weights


@pytest.mark.parametrize("grid", ["coarse", "fine"])
def test_beam_zero(tmp_path, grid):
    k, eps_k = GRIDS[grid]
    for seed in range(6):
        g = SG.general(60 + 40 * seed, 2000 + seed, k=k, eps_k=eps_k)
        lls = [SG.dyadic(12, g["num_pdfs"], 7 * seed + u, k=k) for u in range(4)]
        check(tmp_path, g, lls, beam=0.0, name="g%d.fst" % seed)


# ---------------------------------------------------------------- ties

def test_emitting_tie_goes_to_the_lowest_arc(tmp_path):
    # three equal-cost emitting candidates into state 1 (two twins, one through a better pdf); two into state 3
    # from state 2 at frame 1
    g = graph([INF, 0.0, INF, 0.0],
              [[(1, 1, 5, 1.0), (1, 1, 6, 1.0), (1, 2, 7, 0.75), (2, 1, 0, 0.0)],
               [],
               [(3, 1, 8, 0.5), (3, 3, 9, 0.25)],
               []])
    ll = np.zeros((1, 8), np.float32)
    ll[0, 2] = -0.25
    dec, wants = check(tmp_path, g, [ll])
    assert dec.result(0)[0] == [5] and dec.best_path_arcs(0) == [0]
    ll2 = np.zeros((2, 8), np.float32)
    ll2[1, 3] = -0.25
    dec, wants = check(tmp_path, g, [ll2])
    assert dec.result(0)[0] == [8] and dec.best_path_arcs(0) == [3, 4]


def test_emitting_beats_epsilon_at_equal_cost(tmp_path):
    # state 2: emitting arc 1 (cost 1) against 0 -> 1 -> 2 (emitting arc 0 + epsilon arc 0, cost 0.5 + 0.5);
    # the epsilon candidate has the LOWER arc index of its list, so only the epsilon bit decides
    g = graph([INF, INF, 0.25], [[(1, 1, 6, 0.5), (2, 1, 5, 1.0)], [(2, 0, 7, 0.5)], []])
    ll = np.zeros((1, 8), np.float32)
    dec, _ = check(tmp_path, g, [ll])
    assert dec.result(0) == ([5], 1.5, 1) and dec.best_path_arcs(0) == [1]
    g["arcs"][1] = [(2, 0, 7, 0.25)]                     # strictly cheaper through the epsilon arc
    dec, _ = check(tmp_path, g, [ll])
    assert dec.result(0) == ([6, 7], 1.25, 1) and dec.best_path_arcs(0) == [0, 2]


def test_epsilon_tie_goes_to_the_lowest_arc(tmp_path):
    # state 3 from 1 and from 2 at equal cost: epsilon arc 0 (from 1) wins over epsilon arc 1 (from 2)
    g = graph([INF, INF, INF, 0.0], [[(2, 1, 6, 0.5), (1, 1, 5, 0.75)], [(3, 0, 0, 0.25)], [(3, 0, 0, 0.5)], []])
    dec, wants = check(tmp_path, g, [np.zeros((1, 8), np.float32)])
    assert dec.result(0)[0] == [5] and dec.best_path_arcs(0) == [1, 2]


def test_equal_best_tokens_take_r0_from_the_lowest_state(tmp_path):
    # tokens 1 and 2 tie for best; R0 from state 1 admits candidates into 3, 4 and 5, from state 2 only into 4
    g = graph([INF, INF, INF, 0.0, 0.0, 0.0],
              [[(1, 1, 0, 1.0), (2, 1, 8, 1.0)], [(3, 1, 0, 0.0), (5, 1, 0, 2.0)], [(4, 2, 9, 0.0)], [], [], []])
    ll = np.zeros((2, 8), np.float32)
    ll[1, 2] = 4.0
    dec, wants = check(tmp_path, g, [ll], beam=3.0)
    assert dec.active_bound(0) == 3 and dec.result(0) == ([8, 9], -3.0, 1)


def test_equal_final_costs_go_to_the_lowest_state(tmp_path):
    # 2500 final states of equal cost, entered from the start in DECREASING state order (more than 1100 emitting
    # arcs on one state): the lowest state, 1, is the last arc and is touched late
    n = 2500
    g = graph([INF] + [0.5] * n, [[(n - i, 1, n - i, 1.0) for i in range(n)]] + [[] for _ in range(n)])
    lls = [np.full((1, 8), np.float32(v)) for v in (0.0, 0.25, -1.0, 2.0)]
    dec, _ = check(tmp_path, g, lls)
    for u in range(len(lls)):
        assert dec.result(u)[0] == [1] and dec.best_path_arcs(u) == [n - 1]


# ---------------------------------------------------------------- max-active

def max_active_graph(case, n=40):
    """start -> n states (the frame-1 token list, nL = n exactly), each with three emitting arcs into a third layer
    of final states with self-loops.  The frame-0 costs per `case`."""
    rng = np.random.default_rng(7)
    if case == "negative":          # all costs < 0: the log-likelihood is positive
        w, ll0 = [float(x) * 0.25 for x in rng.integers(0, 9, n)], 6.0
    elif case == "straddle":        # costs on both sides of 0
        w, ll0 = [float(x) * 0.25 for x in rng.integers(-6, 7, n)], 0.0
    elif case == "shared":          # the k-th cost shared by many tokens
        w, ll0 = [0.25, 0.25] + [1.0] * (n - 2), 0.0
    else:                           # "beyond": all but one token exactly at best + beam
        w, ll0 = [0.0] + [4.0] * (n - 1), 0.0
    arcs = [[(1 + i, 1, 1 + i, w[i]) for i in range(n)]]
    for i in range(n):
        arcs.append([(1 + n + 3 * i + j, 2 + j, 0, float(x) * 0.25) for j, x in enumerate(rng.integers(0, 17, 3))])
    for i in range(3 * n):
        arcs.append([(1 + n + i, 5, 0, 0.25)])
    final = [INF] * (1 + n) + [0.0] * (3 * n)
    lls = []
    for s in range(3):
        ll = SG.dyadic(3, 8, 100 + s, k=2, lo=-2.0, hi=0.0)
        ll[0, 1] = ll0
        lls.append(ll)
    return graph(final, arcs), lls


@pytest.mark.parametrize("case", ["negative", "straddle", "shared"])
def test_max_active_boundaries(tmp_path, case):
    n = 40
    g, lls = max_active_graph(case, n)
    unbound = check(tmp_path, g, lls, beam=8.0, max_active=1 << 30)[1]
    bound_somewhere = False
    for ma in (1, 2, n - 1, n, n + 1):
        _, wants = check(tmp_path, g, lls, beam=8.0, max_active=ma, name="g%d.fst" % ma)
        bound_somewhere |= any(w["active_bound"] != x["active_bound"] for w, x in zip(wants, unbound))
        if ma >= n:                                      # nL > max_active is strict
            assert [w["active_bound"] for w in wants] == [x["active_bound"] for x in unbound]
    assert bound_somewhere


def test_max_active_does_not_bind_at_or_past_the_beam(tmp_path):
    n = 40
    g, lls = max_active_graph("beyond", n)
    lls = [ll[:2] for ll in lls]                       # the cutoff of frame 1 only (later lists are longer)
    free, _ = gpu(tmp_path, g, lls, beam=4.0, max_active=1 << 30, name="free.fst")
    for ma in (2, 3, n - 1):
        dec, _ = check(tmp_path, g, lls, beam=4.0, max_active=ma, name="g%d.fst" % ma)
        for u in range(len(lls)):
            assert outcome(dec, u) == outcome(free, u)
    dec, wants = check(tmp_path, g, lls, beam=4.0, max_active=1, name="g1.fst")     # k = 1: best < best + beam binds
    assert any(outcome(dec, u) != outcome(free, u) for u in range(len(lls)))


# ---------------------------------------------------------------- chunk crossings

def test_many_tokens_alternating_between_no_and_many_emitting_arcs(tmp_path):
    n = 1200
    rng = np.random.default_rng(3)
    arcs = [[(1 + i, 1 + i % 7, 0, float(rng.integers(0, 9)) * 0.25) for i in range(n)]]
    for i in range(n):
        if i % 2:
            arcs.append([] if i % 4 == 1 else [(1 + int(rng.integers(n)), 0, 0, 0.5)])
        else:
            arcs.append([(1 + int(rng.integers(n)), 1 + int(rng.integers(7)), int(rng.integers(0, 3)),
                          float(rng.integers(0, 9)) * 0.25) for _ in range(6)])
    final = [INF] + [float(rng.integers(0, 5)) * 0.25 for _ in range(n)]
    g = graph(final, arcs)
    lls = [SG.dyadic(4, 8, s, k=2, lo=-1.0, hi=0.0) for s in range(3)]
    dec, wants = check(tmp_path, g, lls, beam=16.0)
    assert max(w["active_bound"] for w in wants) > 1100


def test_epsilon_fan_out_across_chunks(tmp_path):
    n = 1200
    rng = np.random.default_rng(4)
    arcs = [[(1, 1, 0, 0.0)], [(2 + i, 0, 1 + i % 40, float(rng.integers(0, 4096)) / 4096) for i in range(n)]]
    for i in range(n):
        arcs.append([(2 + i, 1 + int(rng.integers(7)), 0, float(rng.integers(0, 9)) * 0.25), (1, 2, 0, 0.5)])
    g = graph([INF, INF] + [float(rng.integers(0, 8)) * 0.25 for _ in range(n)], arcs)
    lls = [SG.dyadic(4, 8, 10 + s, k=2, lo=-1.0, hi=0.0) for s in range(3)]
    dec, wants = check(tmp_path, g, lls, beam=16.0)
    assert all(w["determined"] for w in wants) and min(w["active_bound"] for w in wants) > 1100


def test_long_epsilon_chain_stays_within_the_round_bound(tmp_path):
    # every frame re-walks a chain of n - 1 epsilon arcs (n states): n - 1 closure rounds against the bound n + 2
    n = 1500
    arcs = [[(0, 1, 0, 0.25), (1, 0, 0, -1.0 / 256)]]
    for i in range(1, n):
        arcs.append(([(i + 1, 0, i % 7, -1.0 / 256)] if i + 1 < n else []) + [(0, 2, 0, 0.5)])
    g = graph([INF] * (n - 1) + [0.0], arcs)
    lls = [SG.dyadic(T, 8, T, k=2, lo=-1.0, hi=0.0) for T in (0, 1, 3)]
    dec, wants = check(tmp_path, g, lls, beam=16.0)
    assert all(w["ok"] for w in wants) and wants[-1]["active_bound"] == n


def test_zero_weight_epsilon_cycles(tmp_path):
    # 1 -> 2 -> 3 -> 1 weighs 0; state 4 enters the cycle through an epsilon arc, so state 1 is won both by an
    # emitting arc (frame 0) and by epsilon arcs (later frames); a self-loop of weight 0 on 2
    g = graph([INF, 0.5, INF, 0.25, INF],
              [[(1, 1, 3, 0.5), (4, 2, 4, 0.25)],
               [(2, 0, 5, 0.0), (1, 3, 0, 0.75)],
               [(3, 0, 0, 0.0), (2, 0, 0, 0.0), (4, 1, 0, 0.5)],
               [(1, 0, 0, 0.0), (3, 2, 6, 0.25)],
               [(1, 0, 0, 0.0), (4, 3, 0, 0.25)]])
    lls = [SG.dyadic(T, 8, 20 + T, k=2) for T in (1, 2, 5, 9)]
    check(tmp_path, g, lls, beam=16.0)
    check(tmp_path, g, lls, beam=1.0, name="b1.fst")


# ---------------------------------------------------------------- exhaustive search

@pytest.mark.parametrize("grid", ["coarse", "fine"])
def test_infinite_beam_is_exhaustive_viterbi(tmp_path, grid):
    k, eps_k = GRIDS[grid]
    for seed in range(6):
        g = SG.general(30 + 30 * seed, 3000 + seed, k=k, eps_k=eps_k)
        lls = [SG.dyadic(10, g["num_pdfs"], 9 * seed + u, k=k) for u in range(4)]
        dec, path = gpu(tmp_path, g, lls, beam=np.inf, max_active=1 << 30, name="g%d.fst" % seed)
        for u, ll in enumerate(lls):
            expect(dec, u, g, ll, M.viterbi32(with_ids(g), ll, PDF), path)


# ---------------------------------------------------------------- non-finite log-likelihoods

def sprinkle(ll, frac, value, seed):
    rng = np.random.default_rng(seed)
    out = ll.copy()
    out.view(np.uint32)[rng.random(ll.shape) < frac] = np.float32(value).view(np.uint32) if np.isscalar(value) else value
    return out


NANS = [np.uint32(x).view(np.float32) for x in (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)]


def test_scattered_minus_inf_matches_the_model(tmp_path):
    for seed in range(4):
        g = SG.general(150, 4000 + seed, k=12, eps_k=12)
        lls = [sprinkle(SG.dyadic(16, g["num_pdfs"], u, k=12), 0.15, -np.inf, 99 + u) for u in range(5)]
        check(tmp_path, g, lls, beam=6.0, name="g%d.fst" % seed)


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/libpkref_decoder.so not built")
def test_scattered_minus_inf_matches_the_reference(tmp_path):
    g = SG.size_for_states(2000, seed=21)
    path = write_graph(tmp_path, "g.fst", g)
    am = ident_model(g["num_tids"])
    lls = [sprinkle(SG.planted(g, 80, seed=u)[0], 0.03, -np.inf, u) for u in range(8)]
    dec = pk.Decoder(pk.Fst(path), am, len(lls))
    dec.decode(lls)
    assert all(dec.result(u)[2] == 1 for u in range(len(lls)))   # a finite token every frame: safe for the reference
    refs = ref_decode_many(path, lls, am.handle)
    for u, ll in enumerate(lls):
        words, weight, ok = dec.result(u)
        assert (words, np.float32(weight).tobytes(), ok) == (refs[u][0], np.float32(refs[u][1]).tobytes(), refs[u][2]), u
        check_self(dec, u, path, ll, PDF, g["final"], 0)


@pytest.mark.parametrize("states", [150, 200])
def test_nan_decodes_as_minus_inf(tmp_path, states):
    g = SG.general(states, 4100, k=12, eps_k=12)
    base = [SG.dyadic(14, g["num_pdfs"], u, k=12) for u in range(3)]
    lls, ref = [], []
    for u, b in enumerate(base):
        mask = np.random.default_rng(u).random(b.shape) < 0.15
        for nan in NANS:
            x = b.copy()
            x[mask] = nan
            lls.append(x)
        ref.append(np.where(mask, np.float32(-np.inf), b))
    dec, _ = check(tmp_path, g, lls + ref, beam=6.0)
    for i in range(len(lls)):
        assert outcome(dec, i) == outcome(dec, len(lls) + i // len(NANS)), i


@pytest.mark.parametrize("row", ["-inf", "nan+", "nan-"])
def test_a_frame_without_finite_token_ends_the_utterance(tmp_path, row):
    value = {"-inf": np.float32(-np.inf), "nan+": NANS[0], "nan-": NANS[1]}[row]
    g = SG.general(120, 4200, k=2, eps_k=12)
    lls = []
    for u, t in enumerate((0, 3, 8, 12)):                  # mid-utterance: ok = 0, no words, weight 0
        ll = SG.dyadic(14, g["num_pdfs"], u, k=2)
        ll[t, :] = value
        lls.append(ll)
    last = SG.dyadic(9, g["num_pdfs"], 9, k=2)
    last[-1, :] = value                                    # the last frame: ok = 1, the empty hypothesis
    dec, wants = check(tmp_path, g, lls + [last], beam=6.0)
    for u in range(len(lls)):
        assert dec.result(u) == ([], 0.0, 0) and dec.best_path_arcs(u) == []
    assert dec.result(len(lls)) == ([], 0.0, 1) and dec.best_path_arcs(len(lls)) == []


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/libpkref_decoder.so not built")
def test_minus_inf_last_frame_matches_the_reference(tmp_path):
    g = SG.size_for_states(2000, seed=22)
    path = write_graph(tmp_path, "g.fst", g)
    am = ident_model(g["num_tids"])
    lls = [SG.planted(g, 30 + 5 * u, seed=u)[0] for u in range(4)]
    for ll in lls:
        ll[-1, :] = -np.inf
    dec = pk.Decoder(pk.Fst(path), am, len(lls))
    dec.decode(lls)
    for u, ll in enumerate(lls):
        assert dec.result(u) == ([], 0.0, 1)
        rw, rweight, rok = ref_decode(path, ll, am.handle)
        assert (rw, rweight, rok) == ([], 0.0, 1)


def test_one_poisoned_utterance_does_not_fail_the_batch(tmp_path):
    g = SG.size_for_states(20000, seed=23)
    path = write_graph(tmp_path, "g.fst", g)
    am = ident_model(g["num_tids"])
    lls = [SG.planted(g, 120 + 9 * u, seed=300 + u)[0] for u in range(32)]
    lls[7] = lls[7].copy()
    lls[7][4, :] = NANS[0]
    fst = pk.Fst(path)
    dec = pk.Decoder(fst, am, 32)
    dec.decode(lls)
    assert dec.result(7) == ([], 0.0, 0)
    clean = pk.Decoder(fst, am, 31)
    clean.decode(lls[:7] + lls[8:])
    for u in range(32):
        if u != 7:
            assert outcome(dec, u) == outcome(clean, u - (u > 7)), u
            assert dec.result(u)[2] == 1


def softmax_overflow_model(num_pdfs=24, hot=5):
    """One affine layer + softmax whose pdf `hot` has a bias of 95, above expf's 88.7: under the reference softmax
    that pdf is NaN in every frame (inf / inf) and the rest of the row the floor."""
    rng = np.random.default_rng(0)
    W = (rng.standard_normal((num_pdfs, 40)) * 0.05).astype(np.float32)
    b = np.zeros(num_pdfs, np.float32)
    b[hot] = 95.0
    return [("linear", W, b), ("softmax",)], np.full(num_pdfs, 1.0 / num_pdfs, np.float32)


def test_decode_batch_of_nan_rows_equals_decode_with_minus_inf(tmp_path):
    layers, prior = softmax_overflow_model()
    am = pk.AcousticModel(layers, prior, 0, 0).set_softmax("reference")
    waves = [synth.utterance(40 + u, 0.3 + 0.2 * u) for u in range(4)]
    bs = pk.BatchScorer(am, synth.global_cmvn_stats(), len(waves), sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    g = SG.general(150, 4300, k=12, eps_k=12, num_pdfs=am.num_pdfs())
    path = write_graph(tmp_path, "g.fst", g)
    dec = pk.Decoder(pk.Fst(path), am, len(waves))
    dec.decode_batch(bs)
    lls = [v.log_prob() for v in bs.fetch_all()]
    assert all(np.isnan(ll[:, 5]).all() and not np.isnan(np.delete(ll, 5, axis=1)).any() for ll in lls)
    host = pk.Decoder(pk.Fst(path), am, 2 * len(waves))
    host.decode(lls + [no_nan(ll) for ll in lls])
    fst = with_ids(g)
    for u, ll in enumerate(lls):
        assert outcome(dec, u) == outcome(host, u) == outcome(host, len(lls) + u), u
        want = M.decode(fst, ll, PDF)
        assert (dec.result(u)[2], np.float32(dec.result(u)[1]).tobytes()) == (want["ok"], np.float32(want["weight"]).tobytes())


# ---------------------------------------------------------------- reuse after a failed call

def test_reuse_after_trace_capacity_exhausted(tmp_path):
    g = SG.general(200, 5000, k=2, eps_k=12)
    g["final"][:] = 0.0
    healthy = [SG.dyadic(3, g["num_pdfs"], u, k=2) for u in range(3)]
    big = SG.dyadic(400, g["num_pdfs"], 9, k=2)
    path = write_graph(tmp_path, "g.fst", g)
    fst, am = pk.Fst(path), ident_model(g["num_pdfs"])
    dec = pk.Decoder(fst, am, 4, trace_capacity=20000)
    dec.set_beam(np.inf, 1 << 30)
    with pytest.raises(pk.PkError) as e:
        dec.decode(healthy + [big])
    assert e.value.code == -6
    again = [healthy[2], healthy[0], healthy[1], healthy[0]]          # a healthy one in the failed slot
    dec.decode(again)
    fresh = pk.Decoder(fst, am, 4, trace_capacity=20000)
    fresh.set_beam(np.inf, 1 << 30)
    fresh.decode(again)
    fstm = with_ids(g)
    for u, ll in enumerate(again):
        assert outcome(dec, u) == outcome(fresh, u), u
        expect(dec, u, g, ll, M.decode(fstm, ll, PDF, beam=np.inf, max_active=1 << 30), path)


def test_reuse_after_negative_epsilon_cycle(tmp_path):
    # the cycle 3 -> 4 -> 3 weighs -0.5 and is reached only through pdf 2; the healthy utterances make pdf 2 -inf
    g = graph([INF, 0.0, 0.0, INF, INF],
              [[(1, 1, 1, 0.5), (2, 2, 2, 0.5), (0, 3, 0, 1.0)],
               [(1, 1, 0, 0.25), (0, 3, 3, 0.5), (0, 0, 0, 0.5)],
               [(3, 0, 0, 0.25), (2, 1, 0, 0.25)],
               [(4, 0, 0, -0.5), (2, 1, 0, 0.0)],
               [(3, 0, 0, 0.0)]])
    healthy = []
    for u in range(3):
        ll = SG.dyadic(6 + u, 8, u, k=2)
        ll[:, 2] = -np.inf
        healthy.append(ll)
    poisoned = SG.dyadic(6, 8, 7, k=2)
    path = write_graph(tmp_path, "g.fst", g)
    fst, am = pk.Fst(path), ident_model(8)
    dec = pk.Decoder(fst, am, 4)
    with pytest.raises(pk.PkError) as e:
        dec.decode([healthy[0], poisoned, healthy[1], healthy[2]])
    assert e.value.code == -1 and "negative epsilon cycle" in str(e.value)
    again = [healthy[2], healthy[0], healthy[1], healthy[1]]
    dec.decode(again)
    fresh = pk.Decoder(fst, am, 4)
    fresh.decode(again)
    fstm = with_ids(g)
    for u, ll in enumerate(again):
        assert outcome(dec, u) == outcome(fresh, u), u
        expect(dec, u, g, ll, M.decode(fstm, ll, PDF), path)
        assert dec.result(u)[2] == 1


# ---------------------------------------------------------------- decode_batch against decode

def ragged_waves():
    hello, cat = (pk.read_wav(os.path.join(G, w)) for w in ("en-us-hello.wav", "en-us-cat.wav"))
    rng = np.random.default_rng(5)
    waves = [np.ascontiguousarray(hello[:300])]                       # shorter than one frame (400 samples)
    for u in range(23):
        src = (hello, cat)[u % 2]
        n = int(rng.integers(400, len(src)))
        o = int(rng.integers(0, len(src) - n + 1))
        waves.append(np.ascontiguousarray(src[o:o + n]))
    return waves


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_decode_batch_equals_decode_of_its_fetch_all(precision):
    from refmodel_text import DIR, load_text_model
    layers, prior, Lc, Rc, tid2pdf, cmvn41 = load_text_model()
    am = pk.AcousticModel(layers, prior, Lc, Rc, tid2pdf, precision=precision)
    waves = ragged_waves()
    bs = pk.BatchScorer(am, cmvn41, len(waves), sum(len(w) for w in waves))
    bs.set_waves(waves)
    if precision != "f32":
        bs.calibrate()
    bs.score(0.1)
    assert bs.num_frames(0) == 0
    fst = pk.Fst(os.path.join(DIR, "wordloop.fst"))
    dec = pk.Decoder(fst, am, 32)                               # more slots than the batch
    dec.decode_batch(bs)
    views = bs.fetch_all()
    host = pk.Decoder(fst, am, len(waves))
    host.decode([v.log_prob() for v in views])
    for u in range(len(waves)):
        assert outcome(dec, u) == outcome(host, u), u


def test_saturated_batch_fails_decode_batch_then_the_decoder_recovers(tmp_path):
    layers, prior, L, R = synth.model("tiny")
    lin = [i for i, l in enumerate(layers) if l[0] == "linear"]
    big = list(layers)
    big[lin[0]] = ("linear", layers[lin[0]][1] * np.float32(2.0 ** 15), layers[lin[0]][2] * np.float32(2.0 ** 15))
    big[lin[1]] = ("linear", layers[lin[1]][1] * np.float32(2.0 ** -15), layers[lin[1]][2])
    am = pk.AcousticModel(big, prior, L, R, precision="f16x3")
    waves = [synth.utterance(3, 1.0), synth.utterance(4, 0.6)]
    bs = pk.BatchScorer(am, synth.global_cmvn_stats(), 2, sum(len(w) for w in waves))
    bs.set_waves(waves)
    g = SG.general(100, 6000, k=12, eps_k=12, num_pdfs=am.num_pdfs())
    path = write_graph(tmp_path, "g.fst", g)
    dec = pk.Decoder(pk.Fst(path), am, 4)
    bs.score(0.1, sync=False)
    with pytest.raises(pk.PkError, match="saturated"):
        dec.decode_batch(bs)
    am.set_input_exponents([0, -14, 0])                        # back in range
    bs.score(0.1, sync=False)
    dec.decode_batch(bs)
    host = pk.Decoder(pk.Fst(path), am, 2)
    host.decode([v.log_prob() for v in bs.fetch_all()])
    for u in range(2):
        assert outcome(dec, u) == outcome(host, u), u
