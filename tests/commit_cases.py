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
    """CommitTrace's rule on the host.  rec: [(prev, arc)] in creation order (prev < own index, or -1); tokens: the
    record index of every token (-1: a token at the start).  -> (b, the arcs the launch commits, in order)."""
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
