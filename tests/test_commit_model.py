"""The commit rule of the online decoder (pk_mi355_online_decoder_set_commit) on the CPU: the per-frame host model
(tests/commit_model.py) ends where decoder_model.decode ends; hand-worked cases of the rule; and the ordering claim
the commit (CompactTrace<., true>) rests on -- in an arena whose indices are in creation order, the reachable records
below the first branching index are the shared trunk, in path order -- on a model of the arena that grows, branches,
prunes, compacts and commits."""
import numpy as np
import pytest

import decoder_model as M
import commit_model as CM
import commit_cases as CC

INF = np.inf


@pytest.mark.parametrize("seed", CC.SEEDS)
def test_model_ends_where_the_decoder_model_ends(seed):
    for beam in CC.BEAMS:
        want = M.decode(CC.with_ids(CC.graph(seed)), CC.loglik(seed), CC.PDF, beam=beam)
        got = CC.model_run(seed, beam)
        for key in ("words", "ok", "active_bound", "determined"):
            assert got[key] == want[key], (seed, beam, key)
        assert np.float32(got["weight"]).tobytes() == np.float32(want["weight"]).tobytes()
        assert got["path"] == (want["path"] or [])
        frames = got["frames"]
        assert len(frames) == CC.FRAMES + 1 if got["ok"] else len(frames) <= CC.FRAMES + 1
        # the shared prefix only grows, and every frame's prefix is a prefix of the next frame's (until the beam empties)
        for a, b in zip(frames, frames[1:]):
            if not b["tokens"]:
                assert not got["ok"] and b is frames[-1]
                break
            pa = next(iter(a["tokens"].values()))[1][:a["lcp"]]
            assert all(p[:a["lcp"]] == pa for _, p in b["tokens"].values()), (seed, beam)
            assert b["lcp"] >= a["lcp"]
        if got["ok"] and got["path"]:
            last = frames[-1]
            assert got["path"][:last["lcp"]] == next(iter(last["tokens"].values()))[1][:last["lcp"]]


def test_prefixes_are_shared_on_these_graphs():
    """What the mode is for: at beam 16 the shared prefix reaches well into the utterance, at beam 2 it trails the
    newest frame by a few arcs, and most runs are determined."""
    runs = {(s, b): CC.model_run(s, b) for s in CC.SEEDS for b in CC.BEAMS}
    assert sum(not r["determined"] for r in runs.values()) * 3 <= len(runs)
    for (s, b), r in runs.items():
        assert any(f["lcp"] >= 2 for f in r["frames"][:45]), (s, b)          # something commits before frame 45
    for s in CC.SEEDS:
        assert runs[s, 16.0]["frames"][-1]["lcp"] >= 19
        last = [f for f in runs[s, 2.0]["frames"] if f["tokens"]][-1]
        assert min(len(p) for _, p in last["tokens"].values()) - last["lcp"] <= 8


def chain(n, first_state=0, first_id=0, pdf=1):
    """States first_state .. first_state + n joined by emitting arcs."""
    return [[(first_state + i + 1, pdf, 0, 0.0, first_id + i)] for i in range(n)]


def run(arcs, T, num_pdfs=4):
    final = np.zeros(len(arcs), np.float32)
    return CM.decode((0, final, arcs), np.zeros((T, num_pdfs), np.float32), CC.PDF, beam=INF, max_active=1 << 30)


def test_one_chain():
    r = run(chain(6) + [[]], 5)
    assert [f["lcp"] for f in r["frames"]] == [0, 1, 2, 3, 4, 5]
    assert [CM.committed_after(f["lcp"]) for f in r["frames"]] == [0, 0, 1, 2, 3, 4]


def test_two_chains_that_never_meet():
    # 0 -> 1 -> 2 -> 3 and 0 -> 4 -> 5 -> 6: the paths differ in their first arc, nothing ever commits
    arcs = [[(1, 1, 0, 0.0, 0), (4, 2, 0, 0.0, 1)], [(2, 1, 0, 0.0, 2)], [(3, 1, 0, 0.0, 3)], [],
            [(5, 2, 0, 0.0, 4)], [(6, 2, 0, 0.0, 5)], []]
    r = run(arcs, 3)
    assert all(len(f["tokens"]) == 2 for f in r["frames"][1:])
    assert [f["lcp"] for f in r["frames"]] == [0, 0, 0, 0]


def test_y_commits_the_trunk_but_its_last_arc():
    # 0 -> 1 -> 2, then 2 -> 3 -> 4 and 2 -> 5 -> 6
    arcs = [[(1, 1, 0, 0.0, 0)], [(2, 1, 0, 0.0, 1)], [(3, 1, 0, 0.0, 2), (5, 2, 0, 0.0, 3)], [(4, 1, 0, 0.0, 4)], [],
            [(6, 2, 0, 0.0, 5)], []]
    r = run(arcs, 4)
    assert [f["lcp"] for f in r["frames"]] == [0, 1, 2, 2, 2]
    assert [CM.committed_after(f["lcp"]) for f in r["frames"]] == [0, 0, 1, 1, 1]


def test_a_path_that_is_a_prefix_of_another_counts_whole():
    # 0 -e-> 1 -e-> 2 -eps-> 3: after frame 1 the token at 2 has path [0, 1], the token at 3 has [0, 1, 2]
    arcs = [[(1, 1, 0, 0.0, 0)], [(2, 1, 0, 0.0, 1)], [(3, 0, 0, 0.0, 2)], []]
    r = run(arcs, 2)
    last = r["frames"][-1]
    assert sorted(p for _, p in last["tokens"].values()) == [[0, 1], [0, 1, 2]]
    assert last["lcp"] == 2 and CM.committed_after(last["lcp"]) == 1
    assert CM.common_prefix([[0, 1], [0, 1, 2]]) == 2 and CM.common_prefix([[], [0]]) == 0 and CM.common_prefix([]) == 0
    # the count rule sees it the same way: the token's own record bounds b
    rec = [(-1, 0), (0, 1), (1, 2)]
    assert CC.count_rule(rec, [1, 2]) == (1, [0])
    assert CC.count_rule(rec, [2]) == (2, [0, 1])
    assert CC.count_rule(rec, [-1, 2]) == (0, [])                          # a token still at the start
    assert CC.count_rule([(-1, 0), (-1, 1)], [0, 1]) == (0, [])            # two roots


@pytest.mark.parametrize("seed", range(8))
def test_reachable_records_below_the_first_branch_are_the_trunk_in_path_order(seed):
    """An arena in creation order: every step each token gets 0 .. 3 successor records, appended in a shuffled order;
    a token may also stay where it is (a path that is a prefix of another); at most `keep` tokens survive; now and
    then the reachable records are compacted in order, and whatever the rule commits leaves the arena with the last
    shared record as root.  A record's arc is its index in `full`, which is never compacted: the oracle for paths."""
    rng = np.random.default_rng(seed)
    keep = int(rng.integers(2, 9))
    full, rec, tokens, committed = [], [], [-1], []
    grew = 0
    for step in range(120):
        born = []
        for x in tokens:
            born += [x] * int(rng.integers(0, 4))
        rng.shuffle(born)
        new = []
        for x in born:
            full.append((rec[x][1] if x >= 0 else -1, len(full)))
            rec.append((x, len(full) - 1))
            new.append(len(rec) - 1)
        stay = [x for x in tokens if x >= 0 and rng.random() < 0.2]
        new = sorted(set(new + stay)) or tokens
        tokens = [int(x) for x in rng.choice(new, min(len(new), keep), replace=False)]
        if rng.random() < 0.3:                                            # CompactTrace: order kept
            alive = set()
            for x in tokens:
                while x >= 0 and x not in alive:
                    alive.add(x)
                    x = rec[x][0]
            remap = {x: i for i, x in enumerate(sorted(alive))}
            rec = [(remap.get(rec[x][0], -1), rec[x][1]) for x in sorted(alive)]
            tokens = [remap[x] if x >= 0 else -1 for x in tokens]
        paths = [CC.path_of(full, rec[x][1]) if x >= 0 else [] for x in tokens]
        lcp = CM.common_prefix(paths)
        b, arcs = CC.count_rule(rec, tokens)
        want = paths[0][:CM.committed_after(lcp)]
        assert committed + arcs == want, (seed, step)
        for x in tokens:                                                  # committed ++ tail is every token's path
            if x >= 0:
                assert committed + CC.path_of(rec, x) == CC.path_of(full, rec[x][1])
        if arcs and rng.random() < 0.7:                                   # the commit: the trunk leaves, b is the root
            alive = set()
            for x in tokens:
                while x >= b and x not in alive:
                    alive.add(x)
                    x = rec[x][0]
            remap = {x: i for i, x in enumerate(sorted(alive))}
            assert remap[b] == 0
            rec = [(remap.get(rec[x][0], -1) if x != b else -1, rec[x][1]) for x in sorted(alive)]
            tokens = [remap[x] for x in tokens]
            committed += arcs
            grew += 1
    assert grew >= 3 and len(committed) >= 10, (seed, grew, len(committed))


@pytest.mark.parametrize("n", CC.EDGES)
def test_two_chains_hold_exactly_n_records_at_the_first_compaction(n):
    """The record counts tests/test_gpu_compact_edges.py rests on, from the host model's token sets: every token of a
    frame is one new record behind its predecessor's; before a frame the arena is compacted, order kept, when more than
    half of cap is in use.  The first compaction finds exactly n records and keeps n - DEAD_FROM; there is no second."""
    D = CC.DEAD_FROM
    g, ll, cap = CC.two_chains(n)
    r = CM.decode(CC.with_ids(g), ll, CC.PDF, beam=CC.WIDE, max_active=1 << 30)
    assert r["ok"] == 1 and len(r["path"]) == ll.shape[0] == n - D + 4
    assert [len(f["tokens"]) for f in r["frames"][1:]] == [2] * D + [1] * (n - D + 4 - D)
    rec, at, seen = [], {(): -1}, []                           # records (prev, arc); a path's record; (top, survivors)
    for t in range(ll.shape[0]):
        if len(rec) > cap // 2:
            alive = set()
            for p in (p for _, p in r["frames"][t]["tokens"].values()):
                x = at[tuple(p)]
                while x >= 0 and x not in alive:
                    alive.add(x)
                    x = rec[x][0]
            remap = {x: i for i, x in enumerate(sorted(alive))}
            seen.append((len(rec), len(alive), t))
            rec = [(remap.get(rec[x][0], -1), rec[x][1]) for x in sorted(alive)]
            at = {p: remap[x] for p, x in at.items() if x in remap}
        for _, p in sorted(r["frames"][t + 1]["tokens"].values(), key=lambda v: v[1][-1]):
            rec.append((at[tuple(p[:-1])] if len(p) > 1 else -1, p[-1]))
            at[tuple(p)] = len(rec) - 1
    assert seen == [(n, n - D, n - D)]                         # top == n exactly, before frame n - D
    assert len(rec) == n - D + 4 and max(len(rec), seen[0][0]) == n
    # (the dead chain's records lay between the live ones: what moved down is still the best path, in order)
    assert CC.path_of(rec, len(rec) - 1) == r["path"]
