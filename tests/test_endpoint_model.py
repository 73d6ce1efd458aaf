"""tests/endpoint_model.py against tests/decoder_model.py, and what the GPU endpointing tests assume of the shared
streams (tests/endpoint_cases.py): every frame determined, rules that fire.  No GPU."""
import numpy as np
import pytest

from pocketkaldi_amd import synth_graph as SG

import decoder_model as M
import endpoint_cases as EC
import endpoint_model as EM
from commit_cases import PDF, with_ids

f32, f64 = np.float32, np.float64


def small(seed):
    g = SG.general(60, seed=200 + seed)
    return g, SG.dyadic(40, g["num_pdfs"], seed=7 * seed)


@pytest.mark.parametrize("seed", range(10))
@pytest.mark.parametrize("beam", [3.0, 16.0])
def test_end_state_is_decoder_models(seed, beam):
    g, ll = small(seed)
    fst = with_ids(g)
    want = M.decode(fst, ll, PDF, beam=beam)
    got = EM.decode(fst, ll, PDF, beam=beam)
    assert got["words"] == want["words"] and got["ok"] == want["ok"] and got["active_bound"] == want["active_bound"]
    assert f32(got["weight"]).tobytes() == f32(want["weight"]).tobytes()
    assert got["determined"] == want["determined"]
    if want["determined"]:
        assert got["path"] == want["path"]


def test_end_state_with_max_active_binding():
    g = SG.word_loop(20, 10, seed=5)
    g["num_pdfs"] = g["num_tids"]
    ll = SG.flat(25, g["num_pdfs"], seed=1)
    fst = with_ids(g)
    want, got = M.decode(fst, ll, PDF, max_active=30), EM.decode(fst, ll, PDF, max_active=30)
    assert (got["words"], got["ok"], got["active_bound"]) == (want["words"], want["ok"], want["active_bound"])
    assert f32(got["weight"]).tobytes() == f32(want["weight"]).tobytes()


@pytest.mark.parametrize("seed", range(8))
def test_relative_cost_with_all_final_weights_zero(seed):
    g, ll = small(seed)
    g = dict(g, final=np.zeros_like(g["final"]))
    seen = 0
    for step in EM.frames(with_ids(g), ll, PDF, beam=6.0):
        e = step["endpoint"]
        if e is None:
            continue
        costs = [f64(c) for c, _, _ in step["tokens"]]
        finite = [c for c in costs if c != np.inf]
        assert e["num_final"] == len(finite)
        if finite:
            assert e["relative_cost"].tobytes() == f32(min(c - min(costs) for c in finite)).tobytes() == f32(0.0).tobytes()
            assert e["final_cost"].tobytes() == e["best_cost"].tobytes()
            seen += 1
    assert seen > 10


def test_trailing_silence_on_a_hand_made_path():
    # state 0 -1-> 1 -2-> 2 -eps-> 3 -2-> 4 -eps-> 5: pdf 2 is silence; one path, so the best path is it
    arcs = [[(1, 1, 7, 0.0)], [(2, 2, 0, 0.0)], [(3, 0, 0, 0.0)], [(4, 2, 0, 0.0)], [(5, 0, 8, 0.0)], []]
    g = dict(start=0, final=np.array([np.inf] * 5 + [0.5], np.float32), arcs=arcs, num_pdfs=4)
    ll = np.zeros((3, 4), np.float32)
    steps = list(EM.frames(with_ids(g), ll, PDF, silence={2}))
    assert [s["endpoint"]["trailing_silence_frames"] for s in steps] == [0, 0, 1, 2]
    assert [s["endpoint"]["frames"] for s in steps] == [0, 1, 2, 3]
    assert [s["endpoint"]["num_final"] for s in steps] == [0, 0, 0, 1]
    assert steps[3]["endpoint"]["relative_cost"] == f32(0.5) and steps[2]["endpoint"]["relative_cost"] == f32(np.inf)
    all_silent = list(EM.frames(with_ids(g), ll, PDF, silence={1, 2}))
    assert [s["endpoint"]["trailing_silence_frames"] for s in all_silent] == [0, 1, 2, 3]
    assert EM.finish(steps[3], g["final"])["words"] == [7, 8]
    assert EM.finish(steps[2], g["final"])["words"] == [] and EM.finish(steps[2], g["final"])["ok"] == 1


@pytest.mark.parametrize("seed", EC.SEEDS)
def test_the_shared_streams_are_determined_and_their_rules_fire(seed):
    steps = EC.model_steps(seed)
    T = EC.stream(seed)[0].shape[0]
    assert len(steps) == T + 1 and abs(T - EC.FRAMES) < 100
    assert all(s["determined"] and s["ok"] and s["endpoint"] for s in steps)
    fired = [EC.rule_of(steps[e]) for e in EC.chunk_ends(T)]
    first_length = fired.index(5)
    assert any(r in (2, 3) for r in fired[:first_length])          # a silence rule, before the length rule
    assert sum(1 for r in fired if r) >= 2
    assert any(s["endpoint"]["num_final"] == 0 for s in steps) and any(s["endpoint"]["num_final"] > 1 for s in steps)


def test_utterances_cut_where_the_rule_fires():
    seed = EC.SEEDS[0]
    g, (ll, _, _) = EC.graph(seed), EC.stream(seed)
    counts = [b - a for a, b in zip([0] + EC.chunk_ends(ll.shape[0])[:-1], EC.chunk_ends(ll.shape[0]))]
    pieces = EM.utterances(with_ids(g), ll, PDF, lambda f, t, c: EC.eval_frames(EC.RULES_FRAMES, f, t, c), counts,
                           silence=SG.silence_pdfs(g))
    assert len(pieces) >= 3 and pieces[-1][2] == 0 and all(r for _, _, r in pieces[:-1])
    assert sum(n for _, n, _ in pieces) == ll.shape[0]
    assert [f for f, _, _ in pieces] == list(np.cumsum([0] + [n for _, n, _ in pieces[:-1]]))
