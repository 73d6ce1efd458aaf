"""A small host model of the GPU decoder's semantics (DESIGN.md "Decoder"), float32 arithmetic where the
reference computes in float and float64 where it computes in double (decoder.cc:132-339).  Slow; for
small graphs only.  Order-independent by construction: candidates keyed (cost, candidate id), the
epsilon closure run to its fixed point, the exact max_active-th cost as the max-active cutoff.  Non-finite
log-likelihoods: N1, a NaN decodes as -inf; N2, a frame that starts without a token of finite cost ends the
utterance with ok = 0."""
import numpy as np

f32, f64 = np.float32, np.float64
EPS_ID = 1 << 31


def split(arcs_by_state):
    """The decoder's emitting / epsilon CSR lists: candidate ids in arc order, state by state."""
    emit, eps = [], []
    for s, arcs in enumerate(arcs_by_state):
        e, n = [], []
        for a in arcs:
            (n if a[1] == 0 else e).append(a)
        emit.append(e)
        eps.append(n)
    ids_e, ids_n, ie, inn = [], [], 0, 0
    for s in range(len(arcs_by_state)):
        ids_e.append(list(range(ie, ie + len(emit[s]))))
        ids_n.append(list(range(inn, inn + len(eps[s]))))
        ie += len(emit[s])
        inn += len(eps[s])
    return emit, eps, ids_e, ids_n


def decode(fst, ll, pdf_of, beam=16.0, max_active=30000, arc_ids=None):
    """fst = (start, final, arcs_by_state) with arcs (next, ilabel, olabel, weight[, arc id]).
    -> dict(words, weight, ok, active_bound, path, determined).

    `determined` is False when the best path (words, arcs) may legitimately depend on the order of the epsilon
    closure: at some closure's fixed point a state won by an epsilon arc has a second epsilon candidate of its
    final cost.  A source that improves at equal cost (a lower candidate id only) does not re-resolve the
    successors it already reached, so the GPU's frontier order and this model's stack order can then keep
    different, equally cheap paths.  Weight, ok and active_bound never depend on the order."""
    start, final, arcs = fst
    emit, eps, ids_e, ids_n = split(arcs)
    beam = f32(beam)
    ll = np.where(np.isnan(ll), f32(-np.inf), ll).astype(f32)          # N1
    determined = True

    def closure(tok, F):
        work = [s for s, v in tok.items() if not v[0] > F]
        while work:
            s = work.pop()
            c, _, path = tok[s]
            for i, a in enumerate(eps[s]):
                cc = f32(c + f32(a[3]))
                if cc > F:
                    continue
                k = (cc, EPS_ID + ids_n[s][i])
                if a[0] not in tok or k < tok[a[0]][:2]:
                    tok[a[0]] = (cc, k[1], path + [a])
                    work.append(a[0])
        nonlocal determined
        ties = {}
        for s, (c, _, _) in tok.items():
            if c > F:
                continue
            for a in eps[s]:
                cc = f32(c + f32(a[3]))
                if cc > F:
                    continue
                v = tok[a[0]]
                if v[1] >= EPS_ID and cc == v[0]:
                    ties[a[0]] = ties.get(a[0], 0) + 1
        if any(n > 1 for n in ties.values()):
            determined = False
        return tok

    tok = closure({start: (f32(0.0), -1, [])}, f32(np.inf))
    F = f32(np.inf)
    active = len(tok)
    ok = 1
    for t in range(ll.shape[0]):
        L = sorted((v[0], s, v[2]) for s, v in tok.items() if not v[0] > F)
        if not L or not L[0][0] < np.inf:                             # N2 (and the empty beam)
            ok = 0
            break
        best, best_state = L[0][0], L[0][1]
        beam_cutoff = f64(best) + f64(beam)
        ab, wc = beam, f32(beam_cutoff)
        if len(L) > max_active:
            kth = sorted(c for c, _, _ in L)[max_active - 1]
            if f64(kth) < beam_cutoff:
                ab = f32(f64(kth) - f64(best) + f64(0.5))
                wc = kth
        r0 = np.inf
        for a in emit[best_state]:
            c = f32(f32(best + f32(a[3])) + f32(-ll[t, pdf_of(a[1])]))
            r0 = min(r0, f64(c) + f64(ab))
        new, cmin = {}, np.inf
        for c, s, path in L:
            if c > wc:
                continue
            for i, a in enumerate(emit[s]):
                cc = f32(f32(c + f32(a[3])) + f32(-ll[t, pdf_of(a[1])]))
                cmin = min(cmin, f64(cc))
                if f64(cc) > r0:
                    continue
                k = (cc, ids_e[s][i])
                if a[0] not in new or k < new[a[0]][:2]:
                    new[a[0]] = (cc, k[1], path + [a])
        F = f32(f64(cmin) + f64(ab))
        tok = closure(new, F)
        active = max(active, len(tok))
    L = [(v[0], s, v[2]) for s, v in tok.items() if not v[0] > F] if ok else []
    if not L:
        return dict(words=[], weight=0.0, ok=0, active_bound=active, path=[], determined=determined)
    bc, bs, bp = np.inf, -1, None
    for c, s, path in sorted(L, key=lambda x: x[1]):
        v = f64(c) + f64(final[s])
        if v != np.inf and v < bc:
            bc, bs, bp = v, s, path
    if bs < 0:
        return dict(words=[], weight=0.0, ok=1, active_bound=active, path=[], determined=determined)
    w = f32(bc)
    w = f32(w + f32(final[bs]))
    return dict(words=[a[2] for a in bp if a[2] != 0], weight=float(w), ok=1, active_bound=active,
                path=[a[4] for a in bp] if bp and len(bp[0]) > 4 else None, determined=determined)



def viterbi32(fst, ll, pdf_of):
    """Exhaustive Viterbi (no beam, no max-active) in the decoder's float arithmetic: the model above with an
    infinite beam -- every cutoff is then +inf and nothing is pruned."""
    return decode(fst, ll, pdf_of, beam=np.inf, max_active=1 << 30)
