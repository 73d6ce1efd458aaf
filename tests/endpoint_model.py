"""The host decoder model of tests/decoder_model.py as a generator (its frame step, copied), for the online decoder's
endpointing (pk_mi355_online_decoder_set_endpointing): after InitDecoding and after every frame it yields the token
list, the best partial path and what EndpointKernel and the host make of them.

    for step in frames(fst, ll, pdf_of, silence={...}):
        step["frames"], step["tokens"], step["best"], step["determined"], step["endpoint"]

tokens: [(cost, state, path)] sorted by (cost, state) -- what the next frame starts from (cost <= the frame's
non-emitting cutoff); path: the arcs from the start, as the graph's tuples.  best: the lowest cost, the lowest state on a
tie (None when no token has a finite cost).  endpoint: dict(frames, trailing_silence_frames, num_final, best_cost,
final_cost, relative_cost), the costs as numpy float32, or None where the device reports valid = 0 (no token).
determined: as decoder_model.decode's, up to this frame.  A frame that starts without a token of finite cost (N2) ends
the generator with a last step of ok = 0 and no tokens.  finish(step, final) is BestPath on a step: decode()'s result."""
import numpy as np

from decoder_model import EPS_ID, split

f32, f64 = np.float32, np.float64


def endpoint_of(tokens, final, pdf_of, silence, frames):
    """Section "Endpointing" of DESIGN.md on a token list: the relative cost in double, the silence that ends the
    best token's path."""
    if not tokens:
        return None
    m_best = min(f64(c) for c, _, _ in tokens)
    fins = [f64(c) + f64(final[s]) for c, s, _ in tokens]
    fins = [v for v in fins if v != np.inf]
    if fins:
        m_fin = min(fins)
        final_cost, relative = f32(m_fin), f32(m_fin - m_best)
    else:
        final_cost = relative = f32(np.inf)
    path = tokens[0][2] if tokens[0][0] < np.inf else []
    trailing = 0
    for a in path:
        if a[1] == 0:
            continue
        trailing = trailing + 1 if pdf_of(a[1]) in silence else 0
    return dict(frames=frames, trailing_silence_frames=trailing, num_final=len(fins), best_cost=f32(m_best),
                final_cost=final_cost, relative_cost=relative)


def frames(fst, ll, pdf_of, beam=16.0, max_active=30000, silence=()):
    start, final, arcs = fst
    emit, eps, ids_e, ids_n = split(arcs)
    beam = f32(beam)
    silence = set(int(p) for p in silence)
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

    def step(tok, F, active, t, ok=1):
        L = sorted((v[0], s, v[2]) for s, v in tok.items() if not v[0] > F) if ok else []
        best = L[0] if L and L[0][0] < np.inf else None
        return dict(frames=t, tokens=L, best=best, determined=determined, ok=ok, active_bound=active,
                    endpoint=endpoint_of(L, final, pdf_of, silence, t))

    tok = closure({start: (f32(0.0), -1, [])}, f32(np.inf))
    F = f32(np.inf)
    active = len(tok)
    yield step(tok, F, active, 0)
    for t in range(ll.shape[0]):
        L = sorted((v[0], s, v[2]) for s, v in tok.items() if not v[0] > F)
        if not L or not L[0][0] < np.inf:                             # N2 (and the empty beam)
            yield step(tok, F, active, t, ok=0)
            return
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
        yield step(tok, F, active, t + 1)


def finish(step, final):
    """BestPath (decoder.cc:304-339) on a step: what decoder_model.decode returns for the rows up to it."""
    L, active, determined = step["tokens"], step["active_bound"], step["determined"]
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


def decode(fst, ll, pdf_of, beam=16.0, max_active=30000):
    last = None
    for last in frames(fst, ll, pdf_of, beam, max_active):
        pass
    return finish(last, fst[1])


def utterances(fst, ll, pdf_of, rules_eval, counts, beam=16.0, max_active=30000, silence=()):
    """The stream ll cut as the online recognizer cuts it: the decoder sees counts[i] new rows at step i, and after a step
    whose endpoint fires (rules_eval(frames, trailing, relative_cost) != 0) the utterance ends there and the next row
    starts a new one.  The last step is the one that closes the stream: nothing is cut there.
    -> [(first_frame, num_frames, rule)], the last piece with rule 0."""
    out, first, pos = [], 0, 0
    gen, seen, step = None, 0, None
    for n in counts[:-1]:
        pos += n
        if gen is None:
            gen = frames(fst, ll[first:], pdf_of, beam, max_active, silence)
            step, seen = next(gen), 0
        while seen < pos - first:
            step = next(gen)
            seen += 1
        e = step["endpoint"]
        rule = rules_eval(e["frames"], e["trailing_silence_frames"], e["relative_cost"]) if e and step["ok"] else 0
        if rule:
            out.append((first, pos - first, rule))
            first, gen = pos, None
    out.append((first, ll.shape[0] - first, 0))
    return out
