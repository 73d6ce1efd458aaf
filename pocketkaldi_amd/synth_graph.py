"""Seeded HCLG-like decoding graphs in the reference's pk::fst_0 format (fst.cc:29-92), with planted
log-likelihoods -- test and benchmark input for the GPU decoder (tests/test_gpu_decode.py,
tools/decode_bench.py).  synth.py (models and waves) is separate and unchanged.

The graph is a word loop:
  * state 0 is the loop state (start, final); state 1 a back-off state (final);
  * each of V words is a chain of phones, each phone a 3-state HMM: every HMM state has a
    self-loop and a forward arc, both emitting (ilabel = a transition id, identity-mapped to a pdf);
  * the loop state enters a word through an emitting arc that carries the word (olabel) and a
    random LM weight; the word's last state returns to the loop state through an epsilon arc, and
    to the back-off state through another, which goes on to the loop state (epsilon, weight >= 0);
  * optionally a silence word (id V + 1, one phone) on the same loop;
  * weights are random floats (no ties); final weights span less than the beam.
Transition ids are 1 + 2 * (3 * phone + hmm_state) + (0 forward | 1 self-loop), all < num_pdfs.

general() makes small graphs of no particular shape for the decoder's edge tests (tests/test_gpu_decode_edges.py),
with dyadic weights and log-likelihoods (dyadic()) so that every float sum of a decode is exact.
"""
import struct

import numpy as np

SECTION = b"pk::fst_0"


def write_fst(path, start, final, arcs_by_state):
    """arcs_by_state[s] = [(next, ilabel, olabel, weight), ...]; states without arcs get first = -1."""
    ns = len(arcs_by_state)
    first = np.full(ns, -1, np.int32)
    flat = []
    for s, arcs in enumerate(arcs_by_state):
        if arcs:
            first[s] = len(flat)
            flat.extend(arcs)
    arr = np.zeros(len(flat), dtype=[("next", "<i4"), ("il", "<i4"), ("ol", "<i4"), ("w", "<f4")])
    if flat:
        arr["next"], arr["il"], arr["ol"], arr["w"] = zip(*flat)
    body = struct.pack("<iii", ns, len(flat), start) + np.asarray(final, "<f4").tobytes() + first.tobytes() + arr.tobytes()
    with open(path, "wb") as f:
        f.write(SECTION.ljust(32, b"\0") + struct.pack("<i", len(body)) + body)


def tid(phone, k, self_loop):
    return 1 + 2 * (3 * phone + k) + (1 if self_loop else 0)


def word_loop(num_words, num_phones, seed, silence=True, phones_per_word=(2, 4), lm=None):
    """-> dict(start, final, arcs (by state), words {word id: [phones]}, num_tids).  lm: the range of the word-entry
    (LM) weights; by default it widens with the vocabulary, as unigram costs do (2 .. 2 + 2 V^(1/3)), which keeps
    the active token count of large graphs well below max-active."""
    lm = lm or (2.0, 2.0 + 2.0 * num_words ** (1.0 / 3.0))
    rng = np.random.default_rng(seed)
    arcs = [[], []]
    final = [float(rng.uniform(0.0, 2.0)), float(rng.uniform(0.0, 2.0))]
    words = {}
    ids = list(range(1, num_words + 1)) + ([num_words + 1] if silence else [])
    for w in ids:
        if silence and w == num_words + 1:
            pron = [0]
        else:
            pron = [int(p) for p in rng.integers(1 if silence else 0, num_phones,
                                                 int(rng.integers(phones_per_word[0], phones_per_word[1] + 1)))]
        words[w] = pron
        hmm = [(p, k) for p in pron for k in range(3)]
        base = len(arcs)
        for _ in hmm:
            arcs.append([])
            final.append(float("inf"))
        p0, k0 = hmm[0]
        arcs[0].append((base, tid(p0, k0, False), w, float(rng.uniform(lm[0], lm[1]))))
        for i, (p, k) in enumerate(hmm):
            s = base + i
            arcs[s].append((s, tid(p, k, True), 0, float(rng.uniform(0.05, 1.5))))
            if i + 1 < len(hmm):
                pn, kn = hmm[i + 1]
                arcs[s].append((s + 1, tid(pn, kn, False), 0, float(rng.uniform(0.05, 1.5))))
        last = base + len(hmm) - 1
        arcs[last].append((0, 0, 0, float(rng.uniform(0.0, 1.0))))
        arcs[last].append((1, 0, 0, float(rng.uniform(0.5, 2.0))))
    arcs[1].append((0, 0, 0, float(rng.uniform(0.0, 0.5))))
    return dict(start=0, final=np.array(final, np.float32), arcs=arcs, words=words, num_tids=1 + 2 * 3 * num_phones)


def size_for_states(num_states, num_phones=400, seed=0, silence=True):
    """A word loop of about num_states states (about 9 HMM states per word)."""
    return word_loop(max(1, num_states // 9), num_phones, seed, silence)


def planted(graph, num_frames, seed, bonus=8.0, noise=3.0, num_pdfs=None):
    """Log-likelihoods [T][num_pdfs] with a planted word sequence: seeded noise, plus `bonus` on the pdf
    of the planted HMM state in every frame.  The sequence returns to the loop state (a final state)
    at its last frame.  T is about num_frames (whole words).  -> (loglik float32, words)."""
    rng = np.random.default_rng(seed)
    n = int(num_pdfs or graph["num_tids"])
    ids = sorted(graph["words"])
    seq, frames = [], []
    while len(frames) < num_frames or not seq:
        w = int(rng.choice(ids))
        seq.append(w)
        for p in graph["words"][w]:
            for k in range(3):
                d = int(rng.integers(1, 4))
                frames.append(tid(p, k, False))             # the frame that enters the state
                frames.extend([tid(p, k, True)] * (d - 1))  # its self-loops
    T = len(frames)
    ll = (-2.0 - noise * np.abs(rng.standard_normal((T, n)))).astype(np.float32)
    for t, pdf in enumerate(frames):
        ll[t, pdf] += np.float32(bonus)
    return ll, seq


def silence_pdfs(graph):
    """The pdfs of word_loop(silence=True)'s silence word (phone 0): the transition ids of its three HMM states."""
    return sorted(tid(0, k, loop) for k in range(3) for loop in (False, True))


def planted_pauses(graph, num_frames, seed, pause_frames, words_between=2, lead=0, bonus=8.0, noise=3.0, num_pdfs=None):
    """planted() for endpointing, on a word_loop(silence=True) graph: `lead` frames of the silence word, then runs of
    `words_between` planted words (never the silence word), each run followed by a stretch of the silence word of
    pause_frames[i % len(pause_frames)] frames (>= 3: one per HMM state, the rest self-loops spread over the three),
    until there are num_frames frames or more.  The last stretch returns to the loop state.
    -> (loglik float32, words, pauses [(first frame, frames)])."""
    rng = np.random.default_rng(seed)
    n = int(num_pdfs or graph["num_tids"])
    sil = max(graph["words"])
    assert graph["words"][sil] == [0], "the graph has no silence word"
    ids = [w for w in sorted(graph["words"]) if w != sil]
    seq, frames, pauses = [], [], []

    def stretch(total):
        assert total >= 3
        d = [1 + (total - 3) // 3 + (1 if k < (total - 3) % 3 else 0) for k in range(3)]
        pauses.append((len(frames), total))
        seq.append(sil)
        for k in range(3):
            frames.append(tid(0, k, False))
            frames.extend([tid(0, k, True)] * (d[k] - 1))

    if lead:
        stretch(lead)
    i = 0
    while len(frames) < num_frames or not seq:
        for _ in range(words_between):
            w = int(rng.choice(ids))
            seq.append(w)
            for p in graph["words"][w]:
                for k in range(3):
                    d = int(rng.integers(1, 4))
                    frames.append(tid(p, k, False))
                    frames.extend([tid(p, k, True)] * (d - 1))
        stretch(int(pause_frames[i % len(pause_frames)]))
        i += 1
    T = len(frames)
    ll = (-2.0 - noise * np.abs(rng.standard_normal((T, n)))).astype(np.float32)
    for t, pdf in enumerate(frames):
        ll[t, pdf] += np.float32(bonus)
    return ll, seq, pauses


def flat(num_frames, num_pdfs, seed, spread=0.05):
    """Nearly flat log-likelihoods: everything stays inside the beam (max-active binds)."""
    rng = np.random.default_rng(seed)
    return (-1.0 - spread * rng.random((num_frames, num_pdfs))).astype(np.float32)


def general(num_states, seed, k=2, eps_k=12, num_pdfs=12, max_arcs=4, eps_frac=0.3, hubs=1, hub_arcs=40,
            final_frac=0.3, empty_frac=0.08, neg_eps=True):
    """A seeded graph of no particular shape -> dict(start=0, final, arcs (by state), num_pdfs).  Ilabels are pdfs
    1 .. num_pdfs - 1 (identity map).  It has several final states (the rest +inf), states without arcs, parallel
    arcs, emitting and epsilon self-loops, epsilon arcs of zero or negative weight and `hubs` states of `hub_arcs`
    arcs.  Emitting weights are multiples of 2^-k in [-0.5, 3], epsilon weights multiples of 2^-eps_k: with the
    log-likelihoods of dyadic(), every float32 sum of a decode of a few hundred frames is exact.  An epsilon arc
    s -> t weighs phi(t) - phi(s) + r with a potential phi in [0, 2] (0 without neg_eps) and r >= 0 (0 in 10 %):
    every epsilon cycle weighs the sum of its r >= 0, so there is no negative cycle, and zero-weight ones occur."""
    rng = np.random.default_rng(seed)
    q, qe = 2.0 ** -k, 2.0 ** -eps_k

    def grid(lo, hi, step):
        return float(rng.integers(round(lo / step), round(hi / step) + 1)) * step

    phi = [grid(0.0, 2.0, qe) if neg_eps else 0.0 for _ in range(num_states)]
    hub_set = set(int(x) for x in rng.choice(num_states, min(hubs, num_states), replace=False)) if hubs else set()
    arcs = [[] for _ in range(num_states)]
    for s in range(num_states):
        if s != 0 and s not in hub_set and rng.random() < empty_frac:
            continue
        for i in range(hub_arcs if s in hub_set else int(rng.integers(1, max_arcs + 1))):
            nxt = s if rng.random() < 0.1 else int(rng.integers(num_states))
            ol = int(rng.integers(1, 50)) if rng.random() < 0.3 else 0
            if i and rng.random() < eps_frac:                        # the first arc of a state emits
                r = 0.0 if rng.random() < 0.1 else grid(0.0, 1.0, qe)
                arcs[s].append((nxt, 0, ol, phi[nxt] - phi[s] + r))
            else:
                arcs[s].append((nxt, int(rng.integers(1, num_pdfs)), ol, grid(-0.5, 3.0, q)))
            if arcs[s][-1][1] and rng.random() < 0.1:                # a parallel emitting arc: same ends, maybe a twin
                a = arcs[s][-1]
                arcs[s].append(a if rng.random() < 0.5 else (a[0], a[1], int(rng.integers(0, 50)), a[3]))
    final = np.array([grid(0.0, 3.0, q) if rng.random() < final_frac else np.inf for _ in range(num_states)], np.float32)
    final[int(rng.integers(num_states))] = grid(0.0, 3.0, q)
    return dict(start=0, final=final, arcs=arcs, num_pdfs=num_pdfs)


def dyadic(num_frames, num_pdfs, seed, k=2, lo=-4.0, hi=2.0):
    """Log-likelihoods [T][num_pdfs], multiples of 2^-k in [lo, hi] (float32, exact)."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -k
    return (rng.integers(round(lo / q), round(hi / q) + 1, (num_frames, num_pdfs)) * q).astype(np.float32)
