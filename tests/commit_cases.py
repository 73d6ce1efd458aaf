"""The runs the commit mode's tests share (tests/test_commit_model.py on the CPU, tests/test_gpu_online_commit.py on
the GPU): SG.general(300, seed=40..45) with SG.dyadic(90, ...) at beams 2, 6 and 16, each decoded once by the host
model with per-frame output (tests/commit_model.py); and a host model of the kernel's count rule over an arena whose
indices are in creation order."""
import functools

import numpy as np

from pocketkaldi_amd import synth_graph as SG

import commit_model as CM

SEEDS = range(6)
BEAMS = (2.0, 6.0, 16.0)
FRAMES = 90
PDF = lambda t: t          # noqa: E731  (identity tid2pdf)


def with_ids(g):
    """The model's graph: arcs carry their file arc id."""
    by_state, k = [], 0
    for st in g["arcs"]:
        by_state.append([tuple(a) + (k + i,) for i, a in enumerate(st)])
        k += len(st)
    return g["start"], np.asarray(g["final"], np.float32), by_state


@functools.lru_cache(maxsize=None)
def graph(seed):
    return SG.general(300, seed=40 + seed)


@functools.lru_cache(maxsize=None)
def loglik(seed):
    return SG.dyadic(FRAMES, graph(seed)["num_pdfs"], seed=100 * seed)


@functools.lru_cache(maxsize=None)
def model_run(seed, beam):
    """commit_model.decode of the run: computed once, shared, never changed."""
    return CM.decode(with_ids(graph(seed)), loglik(seed), PDF, beam=beam)


def count_rule(rec, tokens):
    """The commit's rule (CompactTrace<., true>) on the host.  rec: [(prev, arc)] in creation order (prev < own index, or
    -1); tokens: the record index of every token (-1: a token at the start).
    -> (b, the arcs the launch commits, in order)."""
    count, roots, flag = [0] * len(rec), 0, False
    for x in tokens:
        if x < 0:
            flag = True
            continue
        while True:
            count[x] += 1
            if count[x] > 1:
                break
            if rec[x][0] < 0:
                roots += 1
                break
            x = rec[x][0]
    if roots != 1 or flag:
        return 0, []
    b = min([i for i, c in enumerate(count) if c >= 2] + [x for x in tokens])
    return b, [rec[i][1] for i in range(b) if count[i] > 0]


def path_of(rec, x):
    out = []
    while x >= 0:
        out.append(rec[x][1])
        x = rec[x][0]
    return out[::-1]


# ---------------------------------------------------------------- the plain compaction at the scan's chunk edges
# tests/test_commit_model.py (the record counts, no GPU) and tests/test_gpu_compact_edges.py

EDGES = (511, 512, 513, 1024, 1025)     # records at the first compaction: kDecThreads, twice that, +- 1
DEAD_FROM = 200                         # the first frame at which the second chain's pdf is -inf
WIDE = 1e30                             # a beam that prunes no finite cost and every infinite one


def two_chains(n, dead_from=DEAD_FROM):
    """test_one_launch_commits_exactly_n_records' graph (tests/test_gpu_online_commit.py): two chains from the start that
    never merge, olabel = source state + 1 so that words tell arcs apart.  The second chain dies at frame dead_from, and
    an arena of cap = 2 (n - 1) records holds exactly n when it is first more than half full.
    -> (graph, ll of T = n - dead_from + 4 frames, cap)"""
    T = n - dead_from + 4
    a, b = 1, 1 + T + 2

    def chain(first, pdf):
        return [[(first + i + 1, pdf, first + i + 1, 0.0)] if i + 1 < T + 2 else [] for i in range(T + 2)]
    arcs = [[(a, 1, 1, 0.0), (b, 2, 1, 0.0)]] + chain(a, 1) + chain(b, 2)
    g = dict(start=0, final=np.zeros(len(arcs), np.float32), arcs=arcs, num_pdfs=4)
    ll = np.zeros((T, 4), np.float32)
    ll[:, 1] = -0.25 * (1 + np.arange(T) % 3)                  # costs that tell frames apart
    ll[dead_from:, 2] = -np.inf
    return g, ll, 2 * (n - 1)
