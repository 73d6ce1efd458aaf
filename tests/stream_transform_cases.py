"""Feature transforms on a live slot: the rule restated in numpy, and the driver the GPU tests share.

The rule.  Lt, Rt the spec's contexts, C = Lt + Rt, R the model's right context, M = order * window with deltas and 0
without.  Per slot: nin input frames of the transform final so far (the normalised base frames, or behind deltas the
nd' of stream_delta_cases.advance), nx transform frames final so far, a rows scored so far.  One step makes transform
frames [nx, nx') final, nx' = closed ? nin : max(nx, nin - Rt); transform frame t reads the input frames
clamp(t + j, 0, nin - 1), j = -Lt .. Rt; the slot's own matrix, if it has one, is applied to the newly final frames with
L = R = 0, and a slot without one passes them on as bits; rows [a, b) are scored, b = closed ? nx' : max(a, nx' - R).
stream_transform carries what the kernel carries: a ring of the last C input frames, entry f mod C, in two buffers used
in turn.  Why C frames suffice: after every step of an open slot nx >= nin_old - Rt, and frame nx reads input frame
nx - Lt, so nothing below nin_old - C is read again.

Three wrong variants, as switches, for the test that shows the comparison tells them apart.  None of them can show at
C = 0: there is no ring, and with Rt = 0 nothing is held back."""
import numpy as np

import stream_delta_cases as SD
import transform_cases as TC

VARIANTS = ("short_ring", "clamp_open", "written_parity")
# (in_dim, Lt, Rt, rows, affine)
VARIANT_SPECS = ((13, 3, 3, 40, True), (40, 4, 4, 40, False))
CHUNKINGS = SD.CHUNKINGS
chunks_of = SD.chunks_of


def advance(nin, nx, a, Rt, R, closed):
    """-> (nx', b)."""
    nx1 = nin if closed else max(nx, nin - Rt)
    return nx1, (nx1 if closed else max(a, nx1 - R))


def lookahead(M, Rt, R):
    return M + Rt + R


def _apply(win, m, Dp):
    """One frame: win [W][Dp] the window's input frames, m [rows][K or K + 1] -> [rows], transform_cases' chain."""
    K = win.shape[0] * Dp
    flat = win.reshape(K)
    acc = np.zeros(m.shape[0], np.float32)
    with np.errstate(all="ignore"):
        for k in range(K):
            acc = acc + m[:, k] * flat[k]
        if m.shape[1] == K + 1:
            acc = acc + m[:, K]
    return acc.astype(np.float32)


def stream_transform(x, m, L, R, chunks, close_delay=0, variant=None):
    """x [T][Dp] pushed in `chunks` (sizes summing to T, zeros allowed), closed with the last push (close_delay 0) or that
    many empty steps later -> (the rows [T][rows], the number of rows every step made final).  m None: the rows pass as
    bits (L = R = 0).  Every row is computed from the step's fresh rows and a ring of exactly C frames in two buffers
    used in turn, with the batch rule's own chain.  variant: one of VARIANTS, the wrong rule."""
    x = np.ascontiguousarray(x, np.float32)
    T, Dp = x.shape
    C = L + R
    m = None if m is None else np.ascontiguousarray(m, np.float32)
    ring_len = C - 1 if variant == "short_ring" else C
    ring = [np.full((max(ring_len, 1), Dp), np.nan, np.float32) for _ in range(2)]
    par = 0
    nin = nx = pos = 0
    out, made = [], []
    steps = [(c, False) for c in chunks] or [(0, False)]
    steps = steps + [(0, False)] * close_delay
    steps[-1] = (steps[-1][0], True)
    for c, closed in steps:
        fresh = x[pos:pos + c]
        pos += c
        nin_old, nin = nin, nin + c
        nx1, _ = advance(nin, nx, 0, 0 if variant == "clamp_open" else R, 0, closed)
        old = ring[par]

        def frame(f, src=None):
            if variant is None:
                assert max(nin_old - C, 0) <= f < nin, (f, nin_old, nin)
            return fresh[f - nin_old] if f >= nin_old else (old if src is None else src)[f % ring_len]

        # the hand-over: frames [max(nin - C, 0), nin) to the other buffer, which nothing below reads
        if c > 0 and ring_len > 0:
            keep = {f % ring_len: frame(f).copy() for f in range(max(nin - ring_len, 0), nin)}
            for e, v in keep.items():
                ring[par ^ 1][e] = v
        read = ring[par ^ 1] if variant == "written_parity" else None
        for t in range(nx, nx1):
            if m is None:
                out.append(frame(t, read).copy())
            else:
                win = np.stack([frame(min(max(t + j, 0), nin - 1), read) for j in range(-L, R + 1)])
                out.append(_apply(win, m, Dp))
        made.append(nx1 - nx)
        if c > 0 and ring_len > 0:
            par ^= 1
        nx = nx1
    assert pos == T and nx == T
    width = Dp if m is None else m.shape[0]
    return (np.stack(out) if out else np.zeros((0, width), np.float32)), made


def batch_rows(x, m, L, R, slot_m=None):
    """transform_cases' batch rule on the whole input: the global stage (m None: none), then the slot's own matrix."""
    y = np.ascontiguousarray(x, np.float32) if m is None else TC.transform(x, m, L, R)
    return y if slot_m is None else TC.transform(y, slot_m, 0, 0)


def live_rows(x, m, L, R, chunks, close_delay=0, slot_m=None):
    """The live rule over a slot's life: the global stage step by step, the slot's own matrix over what every step made
    final."""
    y, made = stream_transform(x, m, L, R, chunks, close_delay)
    if slot_m is None:
        return y, made
    parts, at = [], 0
    for k in made:
        parts.append(TC.transform(y[at:at + k], slot_m, 0, 0))
        at += k
    return (np.concatenate(parts) if parts else np.zeros((0, slot_m.shape[0]), np.float32)), made


def lengths(M, Lt, Rt, R, G, extra=(70,)):
    """{0, 1, 2, Rt, Rt + 1, C, C + 1, Rt + R, Rt + R + 1, C + R + 1, G - 1, G, G + 1, 2G + 1} and the extras -- with deltas
    in front the values around M + Rt + R too -- ascending, each once."""
    C = Lt + Rt
    base = {0, 1, 2, Rt, Rt + 1, C, C + 1, Rt + R, Rt + R + 1, C + R + 1, G - 1, G, G + 1, 2 * G + 1, *extra}
    if M:
        base |= {M, M + Rt, M + Rt + R, M + Rt + R + 1, 2 * M + C + R + 1}
    return sorted(base)


def run_jobs(sc, jobs, prob_scale=0.1):
    """stream_delta_cases.run_jobs with one key more: `mat`, the slot's own matrix, handed over right after the open."""
    n = len(jobs)
    rows, nxt, state, k, pos, due, busy = [[] for _ in range(n)], [0] * n, ["pending"] * n, [0] * n, [0] * n, [None] * n, {}
    stats = [None] * n
    N = sc._am.num_pdfs()
    step = 0
    while any(s != "done" for s in state):
        for i, j in enumerate(jobs):
            if state[i] == "pending" and j["slot"] not in busy and step >= j.get("start", 0):
                if j["kind"] == "audio":
                    sc.open(j["slot"], j.get("rate", 16000), speaker_stats=j.get("spk"))
                else:
                    sc.open_features(j["slot"], j["kind"], speaker_stats=j.get("spk"))
                if j.get("mat") is not None:
                    sc.set_slot_transform(j["slot"], j["mat"])
                busy[j["slot"]] = i
                state[i] = "open"
            if state[i] == "open":
                if k[i] < len(j["chunks"]):
                    c = j["chunks"][k[i]]
                    (sc.push if j["kind"] == "audio" else sc.push_features)(j["slot"], j["data"][pos[i]:pos[i] + c])
                    pos[i] += c
                    k[i] += 1
                if k[i] == len(j["chunks"]):
                    if due[i] is None:
                        due[i] = step + j.get("close_delay", 0)
                    if step >= due[i]:
                        sc.close(j["slot"])
                        state[i] = "closed"
        if busy:
            sc.step(prob_scale)
        for i, j in enumerate(jobs):
            if state[i] not in ("open", "closed"):
                continue
            first, r = sc.fetch(j["slot"])
            if r.shape[0]:
                assert first == nxt[i], "job %d: rows start at %d, the last ended at %d" % (i, first, nxt[i])
                rows[i].append(r)
                nxt[i] += r.shape[0]
            if state[i] == "closed":
                state[i] = "done"
                if j.get("stats"):
                    stats[i] = sc.norm_stats(j["slot"])
                del busy[j["slot"]]
        step += 1
    return [(np.concatenate(r) if r else np.zeros((0, N), np.float32), st) for r, st in zip(rows, stats)]
