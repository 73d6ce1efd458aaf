"""The host model of the decoder's semantics (tests/decoder_model.py), pinned on its own (no GPU): it is the oracle
of tests/test_gpu_decode_edges.py.  Hand-worked answers on graphs of a few states for every tie rule, N1 (a NaN
log-likelihood decodes as -inf) and N2 (a frame that starts without a finite token ends the utterance with ok = 0);
and agreement with the reference's own decoder on finite random inputs where oracle/_ref/libpkref_decoder.so exists."""
import ctypes as C
import os

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth_graph as SG

import decoder_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLIB = os.path.join(REPO, "oracle", "_ref", "libpkref_decoder.so")
INF = np.inf
PDF = lambda t: t          # noqa: E731
NAN_POS, NAN_NEG = (np.uint32(x).view(np.float32) for x in (0x7FC00000, 0xFFC00000))


def fst(final, arcs):
    """(start 0, final, arcs with their file arc ids)."""
    by_state, k = [], 0
    for st in arcs:
        by_state.append([a + (k + i,) for i, a in enumerate(st)])
        k += len(st)
    return 0, np.array(final, np.float32), by_state


def ll_rows(*rows, n=4):
    out = np.zeros((len(rows), n), np.float32)
    for t, r in enumerate(rows):
        for pdf, v in r.items():
            out[t, pdf] = v
    return out


def run(g, ll, **kw):
    r = M.decode(g, ll, PDF, **kw)
    return r["words"], r["weight"], r["ok"], r["path"], r["active_bound"]


def test_emitting_tie_goes_to_the_lowest_arc():
    g = fst([INF, 0.0], [[(1, 2, 6, 0.75), (1, 1, 5, 1.0), (1, 1, 7, 1.0)], []])
    # arc 0: 0.75 - (-0.25) = 1.0; arcs 1 and 2: 1.0 - 0 = 1.0
    assert run(g, ll_rows({2: -0.25})) == ([6], 1.0, 1, [0], 1)
    assert run(g, ll_rows({2: -0.5})) == ([5], 1.0, 1, [1], 1)


def test_emitting_beats_epsilon_at_equal_cost():
    g = fst([INF, INF, 0.25], [[(1, 1, 6, 0.5), (2, 1, 5, 1.0)], [(2, 0, 7, 0.5)], []])
    # state 2: emitting 1.0 against 0.5 + 0.5 through the epsilon arc; weight = 1.0 + 0.25, then + 0.25
    assert run(g, ll_rows({})) == ([5], 1.5, 1, [1], 2)
    g = fst([INF, INF, 0.25], [[(1, 1, 6, 0.5), (2, 1, 5, 1.0)], [(2, 0, 7, 0.25)], []])
    assert run(g, ll_rows({})) == ([6, 7], 1.25, 1, [0, 2], 2)


def test_epsilon_tie_goes_to_the_lowest_arc_and_is_flagged():
    g = fst([INF, INF, INF, 0.0], [[(2, 1, 6, 0.5), (1, 1, 5, 0.75)], [(3, 0, 0, 0.25)], [(3, 0, 0, 0.5)], []])
    r = M.decode(g, ll_rows({}), PDF)
    assert (r["words"], r["path"], r["weight"]) == ([5], [1, 2], 1.0)
    assert not r["determined"]              # state 3 has two epsilon candidates of its cost
    g = fst([INF, INF, INF, 0.0], [[(2, 1, 6, 0.5), (1, 1, 5, 0.75)], [(3, 0, 0, 0.25)], [(3, 0, 0, 0.75)], []])
    r = M.decode(g, ll_rows({}), PDF)
    assert (r["words"], r["determined"]) == ([5], True)


def test_equal_best_tokens_take_r0_from_the_lowest_state():
    # frame 1: tokens 1 and 2 both cost 1.  R0 from state 1: min(1, 3) + 3 = 4 admits 3 (1), 5 (3) and 4 (-3);
    # from state 2 it would be -3 + 3 = 0 and admit 4 alone.  F = -3 + 3 = 0 keeps 4.
    g = fst([INF, INF, INF, 0.0, 0.0, 0.0],
            [[(1, 1, 0, 1.0), (2, 1, 8, 1.0)], [(3, 1, 0, 0.0), (5, 1, 0, 2.0)], [(4, 2, 9, 0.0)], [], [], []])
    assert run(g, ll_rows({}, {2: 4.0}), beam=3.0) == ([8, 9], -3.0, 1, [1, 4], 3)


def test_best_path_takes_the_lowest_state_on_equal_final_cost():
    g = fst([INF, 0.5, 0.5], [[(2, 1, 4, 1.0), (1, 1, 3, 1.0)], [], []])
    assert run(g, ll_rows({})) == ([3], 2.0, 1, [1], 2)
    g = fst([INF, 0.75, 0.5], [[(2, 1, 4, 1.0), (1, 1, 3, 0.75)], [], []])
    assert run(g, ll_rows({})) == ([3], 2.25, 1, [1], 2)


def test_max_active_cutoff_is_the_exact_kth_cost():
    # frame 1 holds tokens at 0, 1, 1, 2 (states 1-4); max_active 2: the 2nd cost is 1, so state 4 (cost 2) does not
    # expand and the adaptive beam is (1 - 0) + 0.5: R0 = 0 + 0 + 1.5, F = 0 + 1.5 keeps 5 (0) and 6 (1), not 7 (1.5 + ...)
    arcs = [[(1, 1, 0, 0.0), (2, 1, 0, 1.0), (3, 1, 0, 1.0), (4, 1, 0, 2.0)],
            [(5, 1, 1, 0.0)], [(6, 1, 2, 0.0)], [(7, 1, 3, 1.0)], [(8, 1, 4, 0.0)], [], [], [], []]
    g = fst([INF] * 5 + [0.0] * 4, arcs)
    words, weight, ok, path, bound = run(g, ll_rows({}, {}), max_active=2)
    assert (words, weight, ok, bound) == ([1], 0.0, 1, 4)
    assert run(g, ll_rows({}, {}), max_active=4)[4] == 4                # nL = 4 = max_active: no binding
    assert run(g, ll_rows({}, {}), max_active=3)[0] == [1]


def test_nan_decodes_as_minus_inf():
    g = fst([INF, 0.0, 0.0], [[(1, 1, 1, 0.0), (2, 2, 2, 0.5)], [], []])
    for nan in (NAN_POS, NAN_NEG):
        assert run(g, ll_rows({1: nan})) == ([2], 0.5, 1, [1], 1)
        assert run(g, ll_rows({1: nan})) == run(g, ll_rows({1: -INF}))
        assert run(g, ll_rows({1: nan, 2: nan})) == ([], 0.0, 1, [], 2)   # the last frame: the empty hypothesis


def test_a_frame_without_finite_token_ends_the_utterance():
    g = fst([INF, 0.0], [[(0, 1, 0, 0.5), (1, 2, 7, 1.0)], [(1, 1, 0, 0.25)]])
    assert run(g, ll_rows({}, {1: -1.0}))[:3] == ([7], 1.5, 1)
    for bad in (-INF, NAN_POS, NAN_NEG):
        row = {1: bad, 2: bad, 3: bad}
        assert run(g, ll_rows(row, {}))[:3] == ([], 0.0, 0)                # N2: frame 1 starts with +inf tokens only
        assert run(g, ll_rows({}, row, {}))[:3] == ([], 0.0, 0)
        assert run(g, ll_rows({}, row))[:3] == ([], 0.0, 1)                # after the last frame: ok, no words
    # a -inf cell that leaves one finite token decodes on
    assert run(g, ll_rows({2: -INF}, {1: -1.0}))[:3] == ([7], 1.5, 1)


def test_infinite_beam_keeps_every_state():
    g = fst([INF, 0.0, 0.0], [[(1, 1, 1, 0.0), (2, 1, 2, 100.0)], [(1, 1, 0, 0.0)], [(2, 1, 0, 0.0)]])
    r = M.viterbi32(g, ll_rows({}, {}, {}), PDF)
    assert (r["words"], r["weight"], r["active_bound"]) == ([1], 0.0, 2)
    assert M.decode(g, ll_rows({}, {}, {}), PDF, beam=16.0)["active_bound"] == 1


# ---------------------------------------------------------------- the reference's decoder, finite inputs

@pytest.mark.skipif(not os.path.exists(DECLIB), reason="oracle/_ref/libpkref_decoder.so not built")
def test_model_agrees_with_the_reference_on_finite_random_inputs(tmp_path):
    """Non-negative epsilon weights (where the two keep the same tokens), Gaussian log-likelihoods (no ties), final
    weights within the beam, max-active 30000 (the reference's own).  Inputs on which the model empties the beam are
    not given to the reference (it dereferences a null token there)."""
    L = pk.lib()
    ref = C.CDLL(DECLIB)
    ref.pkref_decode.argtypes = [C.c_char_p, C.POINTER(pk.pk_decodable_t), C.POINTER(C.c_int), C.c_int,
                                 C.POINTER(C.c_float), C.POINTER(C.c_int)]
    am = L.pk_mi355_am_create()
    compared = 0
    try:
        for seed in range(10):
            g = SG.general(20 + 25 * seed, 7000 + seed, k=12, eps_k=12, neg_eps=False)
            g["final"] = np.where(np.isfinite(g["final"]), g["final"] / 4, np.inf).astype(np.float32)
            path = str(tmp_path / ("g%d.fst" % seed))
            SG.write_fst(path, 0, g["final"], g["arcs"])
            model_fst = fst(g["final"], g["arcs"])
            for u in range(4):
                rng = np.random.default_rng(100 * seed + u)
                ll = (rng.standard_normal((int(rng.integers(1, 16)), g["num_pdfs"])) * 1.5 - 1.0).astype(np.float32)
                want = M.decode(model_fst, ll, PDF)
                if not want["ok"]:
                    continue
                d = pk.pk_decodable_t()
                d.log_prob.ncol, d.log_prob.nrow = ll.shape
                d.log_prob.data = ll.ctypes.data_as(C.POINTER(C.c_float))
                d.am = am
                words = (C.c_int * 4096)()
                weight, ok = C.c_float(0), C.c_int(0)
                n = ref.pkref_decode(path.encode(), C.byref(d), words, 4096, C.byref(weight), C.byref(ok))
                assert n >= 0
                assert (list(words[:n]), np.float32(weight.value).tobytes(), ok.value) == \
                    (want["words"], np.float32(want["weight"]).tobytes(), want["ok"]), (seed, u)
                compared += 1
    finally:
        L.pk_mi355_am_destroy(am)
    assert compared >= 30
