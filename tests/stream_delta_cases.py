"""Delta features on a live slot: the rule restated in numpy, and the driver the GPU tests share.

The rule.  M = order * window, R the model's right context.  Per slot: n normalised base frames so far, nd delta frames
final so far, a rows scored so far.  One step makes delta frames [nd, nd') final, nd' = closed ? n : max(nd, n - M);
delta frame t reads the base frames clamp(t + j, 0, n - 1); rows [a, b) are scored, b = closed ? nd' : max(a, nd' - R).
stream_add_deltas carries what the kernel carries: a ring of the last 2 M base frames, entry f mod 2 M."""
import numpy as np

import delta_cases as DC


def advance(n, nd, a, M, R, closed):
    """-> (nd', b)."""
    nd1 = n if closed else max(nd, n - M)
    return nd1, (nd1 if closed else max(a, nd1 - R))


def lookahead(order, window, R):
    return order * window + R


def stream_add_deltas(x, order, window, chunks, close_delay=0):
    """x [T][Db] pushed in `chunks` (sizes summing to T, zeros allowed), closed with the last push (close_delay 0) or that
    many empty steps later -> (the rows [T][(order + 1) Db], the number of rows every step made final).  Every row is
    computed from the step's fresh rows and a ring of exactly 2 M frames, with the batch rule's own chain."""
    x = np.asarray(x, np.float32)
    T, Db = x.shape
    M = order * window
    s = DC.scales(order, window)
    ring = np.full((2 * M, Db), np.nan, np.float32)
    n = nd = pos = 0
    out, made = [], []
    steps = [(c, False) for c in chunks] or [(0, False)]
    steps = steps + [(0, False)] * close_delay
    steps[-1] = (steps[-1][0], True)
    for c, closed in steps:
        fresh = x[pos:pos + c]
        pos += c
        n_old, n = n, n + c
        nd1, _ = advance(n, nd, 0, M, 0, closed)

        def frame(f):
            assert max(n_old - 2 * M, 0) <= f < n, (f, n_old, n)
            return fresh[f - n_old] if f >= n_old else ring[f % (2 * M)]

        for t in range(nd, nd1):
            row = np.zeros((order + 1) * Db, np.float32)
            for i in range(order + 1):
                acc = np.zeros(Db, np.float32)
                for j in range(-i * window, i * window + 1):
                    sc = s[i][j + i * window]
                    if sc != 0.0:
                        acc = (acc + (sc * frame(min(max(t + j, 0), n - 1))).astype(np.float32)).astype(np.float32)
                row[i * Db:(i + 1) * Db] = acc
            out.append(row)
        made.append(nd1 - nd)
        if c > 0:
            keep = {f % (2 * M): frame(f).copy() for f in range(max(n - 2 * M, 0), n)}
            for e, v in keep.items():
                ring[e] = v
        nd = nd1
    assert pos == T and nd == T
    return (np.stack(out) if out else np.zeros((0, (order + 1) * Db), np.float32)), made


def lengths(order, window, R, G, extra=(130,)):
    """{0, 1, 2, M, M + 1, 2M, 2M + 1, M + R, M + R + 1, 2M + R + 1, G - 1, G, G + 1} and the extras, ascending, each once."""
    M = order * window
    return sorted({0, 1, 2, M, M + 1, 2 * M, 2 * M + 1, M + R, M + R + 1, 2 * M + R + 1, G - 1, G, G + 1, *extra})


def chunks_of(n, how, rng):
    """Chunk sizes summing to n: "whole", an int (that many a push), or "random" (1 to 40, empty pushes in between)."""
    if how == "whole":
        return [n] if n else []
    if isinstance(how, int):
        return [how] * (n // how) + ([n % how] if n % how else [])
    out, left = [], n
    while left > 0:
        if rng.random() < 0.3:
            out.append(0)
        c = int(min(left, rng.integers(1, 41)))
        out.append(c)
        left -= c
    return out


CHUNKINGS = ("whole", 1, 7, "random")


def run_jobs(sc, jobs, prob_scale=0.1):
    """jobs: dicts {slot, kind ("audio" | "raw" | "normalized"), data, chunks (frames, or samples for audio), start,
    close_delay, rate, spk, stats}.  A job opens its slot at step `start` or later (once the slot's earlier job has been
    flushed), pushes one chunk a step, and closes with its last chunk (close_delay 0) or that many steps later (steps
    that bring the slot nothing); a job without chunks closes close_delay steps after it opened.  -> per job (rows, the
    slot's norm_stats after its flush when the job asks for `stats`, else None).  Each step's rows must continue where
    the slot's last ones ended."""
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
                busy[j["slot"]] = i
                state[i] = "open"
            if state[i] == "open":
                if k[i] < len(j["chunks"]):
                    c = j["chunks"][k[i]]
                    (sc.push if j["kind"] == "audio" else sc.push_features)(j["slot"], j["data"][pos[i]:pos[i] + c])
                    pos[i] += c
                    k[i] += 1
                if k[i] == len(j["chunks"]):
                    if due[i] is None:                  # the last chunk went in (or there is none): the delay counts from here
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
