"""The online decoder's commit mode (pk_mi355_online_decoder_set_commit / _committed / _trace_stats,
pk_mi355_online_recognizer_stable: csrc/capi_online_decoder.hip; CompactTrace<., true> and OnlineDecodeKernel<., true> in
csrc/decode.hip).  The mode changes no result at any step; the committed prefix only grows, is a prefix of every later
path and is exactly the host model's max(|P| - 1, 0) arcs (tests/commit_model.py); a stream longer than its arena
decodes with the mode on and ends with PK_MI355_E_CAPACITY with it off; the scan's chunk edges; the edges of the rule;
the recognizer's stable text; the command-line flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth_graph as SG

import commit_cases as CC
import commit_model as CM
from test_gpu_align import bits, got_segments
from test_gpu_decode_edges import flat_list, graph, outcome
from test_gpu_online_align import batch, feed, full
from test_gpu_online_decode import ident_model, write_graph

pytestmark = pytest.mark.gpu
E_STATE, E_CAPACITY = -4, -6
INF = np.inf
HOWS = [1, "random", "whole"]


def make(fst, am, n, commit, align=True, beam=16.0, max_active=30000, cap=0):
    dec = pk.OnlineDecoder(fst, am, n, trace_capacity=cap)
    dec.set_beam(beam, max_active)
    if align:
        dec.set_alignment(True)
    if commit:
        dec.set_commit(True)
    return dec


def live(dec, slot):
    """What a live slot shows after an advance, as comparable values."""
    words, cost = dec.partial(slot)
    return words, bits(cost), dec.best_path_arcs(slot), got_segments(dec, slot)


def committed_arcs(dec, slot, arcs):
    """The committed prefix as arc ids (the first num_arcs of the slot's path), checked against the entry's own words
    and frame count."""
    words, n, frames = dec.committed(slot)
    path = dec.best_path_arcs(slot)
    assert n <= len(path), (n, len(path))
    head = path[:n]
    assert [arcs[a][2] for a in head if arcs[a][2]] == words
    assert sum(1 for a in head if arcs[a][1]) == frames
    return head


# ---------------------------------------------------------------- 1, 2: no result changes; prefix and exactness

_runs = {}


def general_runs(tmp_path, seed):
    """Graph `seed` at the three beams, with alignment off and on: slot u of one decoder is fed under chunking
    HOWS[u], once with the mode off and once with it on; what every advance showed is kept.  Computed once per seed."""
    if seed in _runs:
        return _runs[seed]
    g, ll = CC.graph(seed), CC.loglik(seed)
    fst, am, arcs = pk.Fst(write_graph(tmp_path, "g.fst", g)), ident_model(g["num_pdfs"]), flat_list(g)
    out = {}
    for beam in CC.BEAMS:
        want = batch(fst, am, [ll], beam=beam)
        for align in (False, True):
            seen = {}
            for commit in (False, True):
                dec = make(fst, am, 3, commit, align, beam)
                steps = {u: [] for u in range(3)}

                def after(slot, u, fed):
                    steps[u].append((fed, live(dec, slot), committed_arcs(dec, slot, arcs), dec.trace_stats(slot)))
                feed(dec, [ll] * 3, HOWS, seed=seed, after=after)
                seen[commit] = dec, steps
            out[beam, align] = want, seen
    _runs[seed] = g, ll, arcs, out
    return _runs[seed]


@pytest.mark.parametrize("seed", CC.SEEDS)
def test_no_result_changes(tmp_path, seed):
    g, ll, arcs, out = general_runs(tmp_path, seed)
    for (beam, align), (want, seen) in out.items():
        (off, off_steps), (on, on_steps) = seen[False], seen[True]
        for u in range(3):
            assert [(fed, shown) for fed, shown, _, _ in on_steps[u]] == [(fed, shown) for fed, shown, _, _ in off_steps[u]], (beam, u)
            assert len(on_steps[u]) >= (1 if HOWS[u] == "whole" else 9)
            assert all(head == [] for _, _, head, _ in off_steps[u])               # mode off: 0 / 0 / 0
            for dec in (off, on):
                assert outcome(dec, u) == outcome(want, 0), (beam, align, u, dec is on)
                if align:
                    assert full(dec, u) == full(want, 0), (beam, u)
                else:                                          # (no cost was kept: acoustic_cost is NaN)
                    assert [s[:4] for s in got_segments(dec, u)] == [s[:4] for s in got_segments(want, 0)]


@pytest.mark.parametrize("seed", CC.SEEDS)
def test_committed_is_a_growing_prefix_and_exactly_the_models(tmp_path, seed):
    g, ll, arcs, out = general_runs(tmp_path, seed)
    early = exact = 0
    for (beam, align), (want, seen) in out.items():
        model = CC.model_run(seed, beam)
        frames = model["frames"]
        on, steps = seen[True]
        for u in range(3):
            before = []
            for fed, (words, cost, path, segs), head, (in_use, peak, cap) in steps[u]:
                alive = fed < len(frames) and len(frames[fed]["tokens"]) > 0
                if not alive:                                  # the beam emptied: no path at all, whatever was committed
                    assert head == [] and path == [] and words == []
                    continue
                assert head[:len(before)] == before, (beam, u, fed)        # (head is path[:num_arcs]: see committed_arcs)
                before = head
                assert 0 <= in_use <= peak <= cap
                if frames[fed]["determined"]:
                    assert len(head) == CM.committed_after(frames[fed]["lcp"]), (beam, u, fed)
                    assert head == next(iter(frames[fed]["tokens"].values()))[1][:len(head)]
                    exact += 1
                early += fed < 45 and len(head) > 0
            final = on.best_path_arcs(u)
            if want.result(0)[2] and final:
                assert final[:len(before)] == before, (beam, u)
                assert committed_arcs(on, u, arcs) == before               # the finishing launch commits nothing
    assert early > 0 and exact > 0


def test_most_runs_are_determined():
    runs = [CC.model_run(s, b) for s in CC.SEEDS for b in CC.BEAMS]
    assert sum(not r["determined"] for r in runs) * 3 <= len(runs)


# ---------------------------------------------------------------- 3: a stream longer than its arena

def two_word_loop():
    """A loop state 0 (final) and two words of two and three emitting arcs over pdfs 1 .. 3, self-loops included."""
    return graph([0.0, INF, INF, INF],
                 [[(1, 1, 7, 0.5), (2, 3, 8, 0.75)],
                  [(1, 1, 0, 0.25), (0, 2, 0, 0.5)],
                  [(2, 3, 0, 0.25), (3, 2, 0, 0.5)],
                  [(3, 2, 0, 0.125), (0, 1, 0, 0.25)]], num_pdfs=4)


def longer_than_the_arena(fst, am, ll, cap, beam=16.0):
    """With the mode off the slot ends with PK_MI355_E_CAPACITY; with it on it ends as the batch decoder does."""
    assert ll.shape[0] > cap                                   # the best path alone cannot fit the arena
    want = batch(fst, am, [ll], beam=beam, trace=1 << 22)
    assert want.result(0)[2] == 1 and len(want.best_path_arcs(0)) >= ll.shape[0]
    off = make(fst, am, 1, False, cap=cap, beam=beam)
    codes = feed(off, [ll], ["random"], seed=5, tolerate=(E_CAPACITY,))
    assert codes and set(codes) == {E_CAPACITY} and off.result(0)[2] == 0 and off.best_path_arcs(0) == []
    on = make(fst, am, 1, True, cap=cap, beam=beam)
    peaks = []
    assert feed(on, [ll], ["random"], seed=5, after=lambda slot, u, fed: peaks.append(on.trace_stats(slot))) == []
    assert full(on, 0) == full(want, 0)
    in_use, peak, capacity = on.trace_stats(0)
    print("arena: in use %d, peak %d of %d records; %d arcs committed of %d" %
          (in_use, peak, capacity, on.committed(0)[1], len(on.best_path_arcs(0))))
    assert capacity == cap and 0 < peak <= capacity and all(i <= p <= cap for i, p, _ in peaks)
    assert on.committed(0)[1] > ll.shape[0] - cap              # what no longer fits was handed over
    return peak


def test_tiny_loop_stream_longer_than_its_arena(tmp_path):
    g = two_word_loop()
    fst, am = pk.Fst(write_graph(tmp_path, "loop.fst", g)), ident_model(4)
    ll = (np.random.default_rng(3).standard_normal((2000, 4)) * 2).astype(np.float32)
    longer_than_the_arena(fst, am, ll, 256)


def test_word_loop_stream_longer_than_its_arena(tmp_path):
    """Capacity = 4 x the BATCH decoder's active_bound on this utterance.  Why 4 suffices: a frame writes at most one
    record per touched state in its emitting pass and one per improvement of the closure, which in this word loop only
    ever reaches the two loop states, so a frame writes fewer than 2 x active_bound records; the arena is compacted
    before a frame once it is more than half full (2 x active_bound), so a frame always finds its room if what survives
    a compaction is below that half -- and with the planted path 30 ahead of everything else under a beam of 16, what
    survives is the few tokens of the newest frames and the short tail they do not share."""
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    fst, am = pk.Fst(write_graph(tmp_path, "w.fst", g)), ident_model(g["num_tids"])
    ll = SG.planted(g, 1700, seed=11, bonus=30.0, noise=0.5)[0]
    want = batch(fst, am, [ll], trace=1 << 22)
    assert want.active_bound(0) > 100
    longer_than_the_arena(fst, am, ll, 4 * want.active_bound(0))


# ---------------------------------------------------------------- 4: scan edges

def chain_arcs(first, n, pdf, into=None):
    """States first .. first + n - 1, each with one emitting arc to the next (the last one to `into`, or none)."""
    return [[(first + i + 1, pdf, first + i, 0.0)] if i + 1 < n or into is not None else [] for i in range(n)]


@pytest.mark.parametrize("N", [511, 512, 513, 1024, 1025])
def test_one_launch_commits_exactly_n_records(tmp_path, N):
    """Two chains from the start that never merge: two first arcs are alive, nothing can be committed, until the second
    chain's pdf is -inf at frame N + 1.  That launch ends with the first chain's N + 1 records reachable (every other
    index: the dead chain's lie between them) and commits N of them.  The beam is 1e30, not inf: no finite cost is
    ever pruned, as with inf, but a candidate of cost +inf falls outside it -- under a beam of inf it does not
    (inf > inf is false), and the second chain would live on with an infinite cost."""
    WIDE = 1e30
    T = N + 4
    a, b = 1, 1 + T + 2
    arcs = [[(a, 1, 0, 0.0), (b, 2, 0, 0.0)]] + chain_arcs(a, T + 2, 1) + chain_arcs(b, T + 2, 2)
    for s in range(len(arcs)):                                 # olabels: the source state, so words tell arcs apart
        arcs[s] = [(n, il, s + 1, w) for n, il, _, w in arcs[s]]
    g = graph([0.0] * len(arcs), arcs, num_pdfs=4)
    fst, am = pk.Fst(write_graph(tmp_path, "two.fst", g)), ident_model(4)
    ll = np.zeros((T, 4), np.float32)
    ll[:, 1] = -0.25 * (1 + np.arange(T) % 3)                  # costs that tell frames apart
    ll[N:, 2] = -np.inf
    for align in (False, True):
        want = batch(fst, am, [ll], beam=WIDE, max_active=1 << 30)
        assert want.result(0)[2] == 1 and len(want.best_path_arcs(0)) == T
        dec = make(fst, am, 1, True, align, beam=WIDE, max_active=1 << 30, cap=4096)
        dec.open(0)
        dec.advance_host({0: (ll[:N], False)})
        assert dec.committed(0) == ([], 0, 0) and dec.trace_stats(0)[0] == 2 * N
        dec.advance_host({0: (ll[N:N + 1], False)})
        words, n, frames = dec.committed(0)
        assert (n, frames) == (N, N) and words == want.result(0)[0][:N]
        assert dec.trace_stats(0)[0] == 1 and dec.best_path_arcs(0) == want.best_path_arcs(0)[:N + 1]
        dec.advance_host({0: (ll[N + 1:], True)})
        assert dec.committed(0)[1] == N
        if align:
            assert full(dec, 0) == full(want, 0)
        else:
            assert outcome(dec, 0) == outcome(want, 0)


@pytest.mark.parametrize("b", [511, 512, 513])
def test_the_branching_record_at_a_chunk_edge(tmp_path, b):
    """A Y fed whole: a trunk of b + 1 arcs, then two branches that stay alive.  The last trunk record has index b."""
    K, tail = b + 1, 5
    arcs = chain_arcs(0, K, 1, into=K)                         # states 0 .. K - 1, the last into state K
    left, right = K + 1, K + 1 + tail
    arcs += [[(left, 1, 0, 0.0), (right, 2, 0, 0.5)]] + chain_arcs(left, tail, 1) + chain_arcs(right, tail, 2)
    for s in range(len(arcs)):
        arcs[s] = [(n, il, s + 1, w) for n, il, _, w in arcs[s]]
    g = graph([0.0] * len(arcs), arcs, num_pdfs=4)
    fst, am = pk.Fst(write_graph(tmp_path, "y.fst", g)), ident_model(4)
    T = K + 3
    ll = np.zeros((T, 4), np.float32)
    ll[:, 1] = -0.25 * (1 + np.arange(T) % 3)
    ll[:, 2] = -0.125
    for align in (False, True):
        want = batch(fst, am, [ll], beam=INF, max_active=1 << 30)
        dec = make(fst, am, 1, True, align, beam=INF, max_active=1 << 30, cap=2048)
        dec.open(0)
        dec.advance_host({0: (ll, False)})
        words, n, frames = dec.committed(0)
        assert (n, frames) == (b, b) and words == list(range(1, b + 1))
        assert dec.trace_stats(0)[0] == 1 + 2 * 3              # the root and the two branches' three records each
        dec.advance_host({0: (ll[:0], True)})
        if align:
            assert full(dec, 0) == full(want, 0)
        else:
            assert outcome(dec, 0) == outcome(want, 0)


# ---------------------------------------------------------------- 5: edges of the rule

def test_edges_of_the_rule(tmp_path):
    g = two_word_loop()
    fst, am = pk.Fst(write_graph(tmp_path, "loop.fst", g)), ident_model(4)
    rng = np.random.default_rng(9)
    ll = (rng.standard_normal((300, 4)) * 2).astype(np.float32)
    dec = make(fst, am, 3, True, cap=512)
    # a closed, fresh slot
    assert dec.committed(1) == ([], 0, 0)
    with pytest.raises(pk.PkCodeError) as e:
        dec.trace_stats(1)
    assert e.value.code == E_STATE
    # T = 0 and T = 1, and a launch of no frames that is not final
    for T in (0, 1):
        want = batch(fst, am, [ll[:T]])
        dec.open(0)
        with pytest.raises(pk.PkCodeError) as e:
            dec.trace_stats(0)
        assert e.value.code == E_STATE
        dec.advance_host({0: (ll[:0], False)})
        assert dec.committed(0) == ([], 0, 0) and dec.best_path_arcs(0) == [] and dec.trace_stats(0)[0] >= 0
        with pytest.raises(pk.PkCodeError) as e:                       # the mode is the object's
            dec.set_commit(False)
        assert e.value.code == E_STATE
        dec.advance_host({0: (ll[:T], False)})
        dec.advance_host({0: (ll[:0], False)})
        assert dec.committed(0) == ([], 0, 0)
        dec.advance_host({0: (ll[:0], True)})
        assert full(dec, 0) == full(want, 0), T
    # a mid-launch compaction and a commit in the same launch: 200 frames fed whole write more than half the arena
    want = batch(fst, am, [ll])
    dec.open(0)
    dec.advance_host({0: (ll[:200], False)})
    in_use, peak, cap = dec.trace_stats(0)
    assert cap == 512 and peak > cap // 2 and in_use < 64 and dec.committed(0)[1] > 150
    # ... beside a poisoned neighbour, and a neighbour that N2 ends after it has committed
    poison = np.full((100, 4), np.nan, np.float32)
    dead = ll[:100].copy()
    dead[60] = -np.inf
    want_dead = batch(fst, am, [dead])
    assert want_dead.result(0)[2] == 0
    dec.open(1)
    dec.open(2)
    had = 0
    for t in range(100):
        dec.advance_host({0: (ll[200 + t:201 + t], False), 1: (poison[t:t + 1], False), 2: (dead[t:t + 1], False)})
        if t < 60:
            had = dec.committed(2)[1]
        else:                                                           # no words, no path, nothing committed
            assert dec.committed(2) == ([], 0, 0) and dec.partial(2)[0] == [] and dec.best_path_arcs(2) == []
        assert dec.committed(1) == ([], 0, 0)
    assert had > 30
    dec.advance_host({0: (ll[:0], True), 1: (poison[:0], True), 2: (dead[:0], True)})
    assert full(dec, 0) == full(want, 0)
    assert outcome(dec, 2) == outcome(want_dead, 0) and dec.result(1)[2] == 0
    kept = dec.committed(0)
    assert kept[1] > 250
    # the mode toggled between utterances: a finished slot keeps what it was opened with; a reopened slot starts empty
    dec.set_commit(False)
    assert dec.committed(0) == kept and full(dec, 0) == full(want, 0)
    dec.open(1)
    feed_one = lambda slot, x: [dec.advance_host({slot: (x[t:t + 7], False)}) for t in range(0, x.shape[0], 7)]
    feed_one(1, ll[:90])
    assert dec.committed(1) == ([], 0, 0)
    dec.advance_host({1: (ll[:0], True)})
    short = batch(fst, am, [ll[:90]])
    assert full(dec, 1) == full(short, 0) and dec.committed(0) == kept
    dec.set_commit(True)
    dec.open(0)                                                          # reopened after a long stream: lists cleared
    assert dec.committed(0) == ([], 0, 0) and dec.best_path_arcs(0) == []
    feed_one(0, ll[:90])
    assert 0 < dec.committed(0)[1] < 90 + 10
    dec.advance_host({0: (ll[:0], True)})
    assert full(dec, 0) == full(short, 0)


def test_advances_that_are_never_synchronized_lose_nothing(tmp_path):
    """What a launch commits lives only in the slot's path slice until the host has taken it: advances in a row without
    a synchronize, and calls whose slots differ from the call before, must still end with the batch decoder's result."""
    g = two_word_loop()
    fst, am = pk.Fst(write_graph(tmp_path, "loop.fst", g)), ident_model(4)
    rng = np.random.default_rng(17)
    lls = [(rng.standard_normal((T, 4)) * 2).astype(np.float32) for T in (400, 333)]
    want = batch(fst, am, lls)
    for align in (False, True):
        dec = make(fst, am, 2, True, align, cap=512)
        dec.open(0)
        dec.open(1)
        pos, turn = [0, 0], 0
        while min(pos[u] - lls[u].shape[0] for u in range(2)) < 0:
            # both slots, slot 0 alone, slot 1 alone, in turn; no synchronize and no getter in between
            chunks = {}
            for u in ((0, 1), (0,), (1,))[turn % 3]:
                if pos[u] < lls[u].shape[0]:
                    n = int(rng.integers(0, 12))
                    chunks[u] = (lls[u][pos[u]:pos[u] + n], False)
                    pos[u] += n
            dec.advance_host(chunks, sync=False)
            turn += 1
        dec.advance_host({0: (lls[0][:0], True)}, sync=False)
        dec.advance_host({1: (lls[1][:0], True)}, sync=False)
        dec.synchronize()
        for u in range(2):
            assert dec.committed(u)[1] > lls[u].shape[0] - 100
            if align:
                assert full(dec, u) == full(want, u), u
            else:
                assert outcome(dec, u) == outcome(want, u), u


# ---------------------------------------------------------------- 6: the recognizer and the command-line tool

def test_recognizer_stable_text_and_cli():
    from refmodel_text import DIR
    from test_gpu_decoder import G
    from test_gpu_online_recognizer import comparable
    conf = os.path.join(DIR, "recognizer.conf")
    files = [os.path.join(G, w) for w in ("en-us-hello.wav", "en-us-cat.wav")]
    waves = [pk.read_wav(f) for f in files]
    rec = pk.Recognizer(conf, max_utts=2, max_total_samples=sum(len(w) for w in waves))
    want = rec.process(waves)
    rec.close()
    online = pk.OnlineRecognizer(conf, max_streams=2, max_step_samples=2 * 1600)
    try:
        assert online.stable(0) == ""
        online.decoder.set_commit(True)
        for u in range(2):
            online.open(u)
        pos, before, live_slots, grew = [0, 0], ["", ""], {0, 1}, 0
        while live_slots:
            closing = []
            for u in sorted(live_slots):
                online.push(u, waves[u][pos[u]:pos[u] + 1600])
                pos[u] += 1600
                if pos[u] >= len(waves[u]):
                    online.close(u)
                    closing.append(u)
            online.step()
            for u in sorted(live_slots):
                stable, partial = online.stable(u), online.partial(u)
                assert partial.startswith(stable) and stable.startswith(before[u]), (u, before[u], stable, partial)
                assert stable == "" or partial == stable or partial[len(stable)] == " "
                grew += stable != before[u]
                before[u] = stable
            for u in closing:
                assert comparable(online.result(u)) == comparable(want[u]), u
                live_slots.discard(u)
        assert grew >= 1
    finally:
        online.destroy()
    # --online --commit: stdout as without it; every --partials line gains the stable text as a fourth field
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))) + os.pathsep +
               os.environ.get("PYTHONPATH", ""))
    tool = [sys.executable, "-m", "pocketkaldi_amd.recognize", conf, files[0], "--online", "--partials"]
    off = subprocess.run(tool, capture_output=True, text=True, env=env)
    on = subprocess.run(tool + ["--commit"], capture_output=True, text=True, env=env)
    assert off.returncode == 0 and on.returncode == 0, off.stderr + on.stderr
    assert on.stdout == off.stdout and on.stdout.split("\t")[1] == want[0].text
    shown_off = [l.split("\t") for l in off.stderr.splitlines() if l.startswith(files[0] + "\t")]
    shown_on = [l.split("\t") for l in on.stderr.splitlines() if l.startswith(files[0] + "\t")]
    assert shown_off and all(len(l) == 3 for l in shown_off) and all(len(l) == 4 for l in shown_on)
    assert all(l[2].startswith(l[3]) for l in shown_on) and shown_on[-1][2] == want[0].text
    assert [l[:3] for l in shown_on if l[:3] in shown_off] == shown_off      # every partial of the mode off is there
