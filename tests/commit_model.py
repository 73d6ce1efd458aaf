"""decoder_model.decode's frame loop restated with per-frame output, for the online decoder's commit mode
(pk_mi355_online_decoder_set_commit): after InitDecoding and after every frame, the token set with every token's
backtrace path, |P| -- the length of the longest prefix that ALL those paths share -- and whether the run is still
`determined` (decoder_model.decode's flag, as of that frame).  The commit rule: a launch that ends after that frame has
committed max(|P| - 1, 0) arcs in all.  Slow; for small graphs only."""
import numpy as np

from decoder_model import EPS_ID, f32, f64, split


def common_prefix(paths):
    """|P| of a list of paths (lists of comparable items): 0 for none, or when any path is empty.  A path that is a
    prefix of another counts with its full length, so |P| is at most the shortest path."""
    paths = list(paths)
    if not paths:
        return 0
    n = min(len(p) for p in paths)
    first = paths[0]
    for i in range(n):
        if any(p[i] != first[i] for p in paths):
            return i
    return n


def committed_after(lcp):
    return max(lcp - 1, 0)


def decode(fst, ll, pdf_of, beam=16.0, max_active=30000):
    """fst as decoder_model.decode takes it, arcs with their arc id: (next, ilabel, olabel, weight, arc id).
    -> dict(words, weight, ok, active_bound, path, determined, frames) where frames[0] is the state after InitDecoding
    and frames[t + 1] the state after frame t: dict(tokens={state: (cost, [arc ids])}, lcp=|P|, determined).  A run that
    N2 ends has no entry for the frame that ended it."""
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

    frames = []

    def record(tok, F):
        live = {s: (v[0], [a[4] for a in v[2]]) for s, v in tok.items() if not v[0] > F}
        frames.append(dict(tokens=live, lcp=common_prefix(p for _, p in live.values()), determined=determined))

    tok = closure({start: (f32(0.0), -1, [])}, f32(np.inf))
    F = f32(np.inf)
    active = len(tok)
    ok = 1
    record(tok, F)
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
        record(tok, F)
    out = dict(words=[], weight=0.0, ok=ok, active_bound=active, path=[], determined=determined, frames=frames)
    L = [(v[0], s, v[2]) for s, v in tok.items() if not v[0] > F] if ok else []
    if not L:
        out["ok"] = 0
        return out
    bc, bs, bp = np.inf, -1, None
    for c, s, path in sorted(L, key=lambda x: x[1]):
        v = f64(c) + f64(final[s])
        if v != np.inf and v < bc:
            bc, bs, bp = v, s, path
    if bs < 0:
        return out
    w = f32(bc)
    w = f32(w + f32(final[bs]))
    out.update(words=[a[2] for a in bp if a[2] != 0], weight=float(w), path=[a[4] for a in bp])
    return out
