"""Online scorer benchmark: S live streams x `seconds` of audio, model S, every stream pushing one chunk of C ms per
step (pk_mi355_stream_*).  Prints ONE JSON line and writes it to profiles/stream_bench.json:

  step_ms            wall time of one step (push of every stream's chunk + step + synchronize): median, p90, max
                     (an upper bound on the GPU time of a step: the host's planning and launches are inside it)
  frames_per_s       frames scored / total wall time of the timed steps
  rtf                median step wall time / chunk duration (all S streams served by one GPU: < 1 keeps up)
  algorithmic_delay_ms  how long after its last sample a frame can be scored at the earliest: the rest of its
                     400-sample window (15 ms after the frame shift) and R frames of look-ahead (10 ms each), plus up to
                     one chunk of waiting for the push that carries them; the step's compute time comes on top
  check              the first stream's rows equal BatchScorer on its whole wave, bit for bit

    python tools/stream_bench.py [--streams 256] [--seconds 10] [--chunk-ms 100] [--out profiles/stream_bench.json]

--decode adds the online decoder to every step (a word loop of about 20000 states, beam 16, max-active 2000): the
step is then push + score + pk_mi355_online_decoder_advance + every live stream's partial(), and the record gains

  window_ms          the median step time over the streams' first 10 s and over their last 10 s: a step whose cost
                     grows with the time since open shows here.  `step` is the whole step, `advance` the same
                     without the partial() calls (push + score + advance, the library alone), `partial` the
                     partial() calls of all streams alone (the Python getter builds a list of every word)
  trace              the largest arena peak and the records in use at the end, over the streams (trace_stats); the
                     most and the fewest arcs a stream committed, and the longest tail (final path - committed)

--commit (implies --decode) turns the decoder's commit mode on.  The long-stream leg is
    python tools/stream_bench.py --streams 32 --seconds 120 --decode [--commit] --out <file>
run with the mode off, on, off, on, each in a process of its own (profiles/stream_commit.json holds the four records).

--endpoint (implies --decode) turns endpointing on, the word loop's silence pdfs and the usual five rules: after every
advance every stream's endpoint() is read, and the streams whose rule fired are finished in one call and opened again.
window_ms gains `endpoint`, the time of those reads and cuts, and the record `endpoint.cuts`.  What the mode costs is
`advance` (the second kernel and the copy of its records are inside the synchronous advance) plus `endpoint`, against a
run without the flag: profiles/stream_endpoint.json.

--features normalized|raw feeds the same streams as features instead of audio: every stream pushes
the frames of one chunk per step (10 frames for 100 ms) into a features-only scorer (pk.OnlineFeatureScorer; with the
statistics for raw).  The features are the batch scorer's on the same waves -- its fbank for raw, its CMVN'd features for
normalized -- so the check against BatchScorer stays bit for bit.  profiles/stream_features_bench.json holds the audio
leg and both feature legs of one session.

--feat-dim D (with --features) replaces the waves by synthetic [T][D] features and model S by the tiny model at that
dimension: raw features then take StreamCmvnChainKernel in front of the layout launch, and the
normalized leg of the same dimension is the step without it.  profiles/cmvn_any_bench.json holds both legs at D = 80.

--frontend key=value,... (pk.parse_frontend, the syntax of recognize.py's flag) feeds the same audio to an online scorer
with that front-end and model S at the spec's dimension; the statistics are the means of the first
stream's features at the spec, count 2500, and the check is against BatchScorer(frontend=spec).
profiles/frontend_stream_bench.json holds those legs beside the plain audio leg.

--cmvn SPEC (pk.parse_norm's text: mode=none, mode=speaker,norm_vars=true, mode=online,norm_vars=true, ...) sets that
normalisation on the scorer, with stream 0's own statistics as the global record and as every
slot's speaker record; the check is against the batch scorer under the same spec.  profiles/stream_bench_cmvn_*.json
hold the default leg and one leg per mode.

--deltas order,window puts delta features in front of the splice (pk.DeltaSpec), with
--features raw --feat-dim Db (synthetic [T][Db] rows through the tiny model at (order + 1) Db, Db = 40 too) or with audio
and --frontend (model S at (order + 1) x the spec's dimension); the check is against the batch deltas scorer.  The leg to
hold it against is --features normalized --feat-dim (order + 1) Db on the same tree: the difference is StreamDeltaKernel
and the normaliser.  profiles/stream_deltas_bench.json holds those legs.

--transform left,right,out_dim puts a feature transform in front of the splice (pk.TransformSpec): a
seeded affine matrix from (left + right + 1) x the width in front of it -- Db, or (order + 1) Db behind --deltas -- to
out_dim, with --features raw --feat-dim Db (the tiny model at out_dim) or with audio and --frontend (model S at out_dim).
--slot-transforms hands every slot a matrix of its own (out_dim x (out_dim + 1)) when it is opened.  The check is against
the batch transform scorer under the same matrices; the leg to hold it against is --features normalized --feat-dim
out_dim on the same tree.  profiles/stream_transform_bench.json holds those legs.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402  (one HIP runtime in the process: the one torch loads, as bench.py)
import numpy as np  # noqa: E402

import pocketkaldi_amd as pk  # noqa: E402
from pocketkaldi_amd import synth  # noqa: E402


def bs_rows(bs):
    """The front-end's rows of the check's one utterance (a score in the scorer's current mode computes them)."""
    bs.score(0.1)
    return bs.fetch_fbank(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chunk-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stream_bench.json"))
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--commit", action="store_true")
    ap.add_argument("--endpoint", action="store_true")
    ap.add_argument("--trace-capacity", type=int, default=0)
    ap.add_argument("--features", choices=["normalized", "raw"], default=None)
    ap.add_argument("--feat-dim", type=int, default=40,
                    help="with --features: synthetic features of this dimension (5 N(0, 1) + 3; raw: statistics of count 2500, "
                         "StreamCmvnChainKernel's path, DESIGN.md section 15) through a small model; checked against FeatureScorer")
    ap.add_argument("--frontend", default=None, help="a front-end spec, key=value,... (audio streams; model S at its dimension)")
    ap.add_argument("--cmvn", default=None, help="a normalisation spec for the scorer, pk.parse_norm's text (mode=none | speaker | online,...; "
                    "DESIGN.md section 20); the global and the speakers' records are stream 0's own statistics")
    ap.add_argument("--deltas", default=None, help="order,window: delta features in front of the splice (DESIGN.md section 24), with "
                    "--features raw --feat-dim Db or with audio and --frontend")
    ap.add_argument("--transform", default=None, help="left,right,out_dim: a feature transform in front of the splice (DESIGN.md section 26), "
                    "with --features raw --feat-dim Db or with audio and --frontend; behind --deltas when both are given")
    ap.add_argument("--tiny", action="store_true", help="with --features at 40 dimensions: synthetic features through the tiny model, as at "
                    "every other --feat-dim (the leg to hold a transform to 40 dimensions against)")
    ap.add_argument("--slot-transforms", action="store_true", help="with --transform: every slot gets a matrix of its own at its open")
    a = ap.parse_args()
    xf = None
    if a.transform is not None:
        try:
            xf = tuple(int(v) for v in a.transform.split(","))
            assert len(xf) == 3 and min(xf[:2]) >= 0 and xf[2] >= 1
        except (ValueError, AssertionError):
            ap.error("--transform left,right,out_dim")
        if a.decode or a.commit or a.endpoint or not ((a.features == "raw") != (a.frontend is not None)):
            ap.error("--transform takes --features raw --feat-dim Db, or audio with --frontend, and no decoder")
    if a.slot_transforms and xf is None:
        ap.error("--slot-transforms goes with --transform")
    dspec = None
    if a.deltas is not None:
        try:
            dspec = pk.DeltaSpec(*[int(v) for v in a.deltas.split(",")])
            dspec.check()
        except (ValueError, TypeError, pk.PkError) as e:
            ap.error("--deltas order,window: %s" % e)
        if a.decode or a.commit or a.endpoint or not ((a.features == "raw") != (a.frontend is not None)):
            ap.error("--deltas takes --features raw --feat-dim Db, or audio with --frontend, and no decoder")
    if a.tiny and a.features is None:
        ap.error("--tiny goes with --features")
    synthetic = a.feat_dim != 40 or a.tiny or ((dspec is not None or xf is not None) and a.features is not None)

    def transform_of(width):
        """(the spec, the slots' four matrices or None) for rows `width` wide in front of the transform."""
        Lt, Rt, out = xf
        K = (Lt + Rt + 1) * width
        m = (np.random.default_rng(5).standard_normal((out, K + 1)) / np.sqrt(K)).astype(np.float32)
        own = [(np.eye(out, out + 1) + 0.1 * np.random.default_rng(60 + u).standard_normal((out, out + 1))).astype(np.float32) for u in range(4)]
        return pk.TransformSpec(m, Lt, Rt, in_dim=width), own if a.slot_transforms else None

    xspec = slot_mats = None
    if a.cmvn is not None and a.features == "normalized":
        ap.error("--cmvn takes audio or raw features")
    spec = None
    if a.frontend is not None:
        if a.features or a.feat_dim != 40:
            ap.error("--frontend takes audio streams")
        try:
            spec = pk.parse_frontend(a.frontend)
        except ValueError as e:
            ap.error(str(e))
    if a.feat_dim != 40 and dspec is None and xf is None and (a.features is None or a.decode or a.commit or a.endpoint):
        ap.error("--feat-dim takes --features and no decoder")
    a.decode = a.decode or a.commit or a.endpoint

    pk.set_device(0)
    layers, prior, L, R = synth.model("S")
    am = pk.AcousticModel(layers, prior, L, R)
    g = synth.global_cmvn_stats()
    waves = [synth.utterance(u, a.seconds) for u in range(a.streams)]
    chunk = int(round(a.chunk_ms * synth.SAMPLE_RATE / 1000.0))
    nsteps = (len(waves[0]) + chunk - 1) // chunk
    feats = None
    model_name = "S (440 -> 4 x 1024 -> 3000, L = R = 5), f32, stable softmax"
    if spec is not None:
        D = spec.dim
        Dm = D if dspec is None else dspec.dim(D)
        if xf is not None:
            xspec, slot_mats = transform_of(Dm)
            Dm = xf[2]
        layers, prior, L, R = synth.model("S", feat_dim=Dm)
        am = pk.AcousticModel(layers, prior, L, R)
        model_name = "S at feat_dim %d (%d -> 4 x 1024 -> 3000, L = R = 5), f32, stable softmax; front-end %r%s" % (
            Dm, 11 * Dm, spec, ("" if dspec is None else "; %r" % dspec) + ("" if xspec is None else "; %r" % xspec))
        fb = pk.Frontend(spec).compute(waves[0])
        g = np.concatenate([fb.astype(np.float64).mean(axis=0) * 2500.0, [2500.0]]).astype(np.float32)
        if xspec is not None:
            sc = pk.OnlineScorer.with_transform(am, g, a.streams, a.streams * chunk, xspec, frontend=spec, deltas=dspec)
        else:
            sc = pk.OnlineScorer(am, g, a.streams, a.streams * chunk, frontend=spec, deltas=dspec)
    elif synthetic:
        D = a.feat_dim
        Dm = D if dspec is None else dspec.dim(D)
        if xf is not None:
            xspec, slot_mats = transform_of(Dm)
            Dm = xf[2]
        layers, prior, L, R = synth.model("tiny", feat_dim=Dm)
        am = pk.AcousticModel(layers, prior, L, R)
        model_name = "tiny at feat_dim %d (L = R = 5), f32, stable softmax%s" % (
            Dm, ("" if dspec is None else "; %r in front, base %d" % (dspec, D)) + ("" if xspec is None else "; %r in front" % xspec))
        g = np.concatenate([np.full(D, 3.0 * 2500.0), [2500.0]]).astype(np.float32)
        T = pk.num_frames(len(waves[0]))
        base = [(5.0 * np.random.default_rng(u).standard_normal((T, D)) + 3.0).astype(np.float32) for u in range(4)]
        feats = [base[u % 4] for u in range(a.streams)]
        chunk = int(round(a.chunk_ms / 10.0))                  # frames per step
        nsteps = (T + chunk - 1) // chunk
        if xspec is not None:
            sc = pk.OnlineFeatureScorer.with_transform(am, a.streams, a.streams * chunk, xspec, global_stats=g, deltas=dspec)
        else:
            sc = pk.OnlineFeatureScorer(am, a.streams, a.streams * chunk, global_stats=g if a.features == "raw" else None, deltas=dspec)
    elif a.features:
        bs = pk.BatchScorer(am, g, a.streams, sum(len(w) for w in waves))
        bs.set_waves(waves)
        bs.score(0.1)
        feats = [(bs.fetch_fbank if a.features == "raw" else bs.fetch_cmvn)(u) for u in range(a.streams)]
        bs.close()
        chunk = int(round(a.chunk_ms / 10.0))                  # frames per step
        nsteps = (feats[0].shape[0] + chunk - 1) // chunk
        sc = pk.OnlineFeatureScorer(am, a.streams, a.streams * chunk, global_stats=g if a.features == "raw" else None)
    else:
        sc = pk.OnlineScorer(am, g, a.streams, a.streams * chunk)
    norm = record0 = None
    if a.cmvn is not None:
        norm = pk.parse_norm(a.cmvn)
        if feats:
            rows0 = feats[0]
        else:
            bs = pk.BatchScorer(am, g, 1, len(waves[0]), frontend=spec, deltas=dspec)
            bs.set_waves(waves[:1])
            bs.score(0.1)
            rows0 = bs.fetch_fbank(0)
            bs.close()
        record0 = pk.cmvn_normalize(rows0, pk.NormSpec("utterance", True, True))[1]
        online_cmvn = isinstance(norm, pk.OnlineCmvnSpec)
        sc.set_norm(norm, record0) if online_cmvn else sc.set_norm(norm)
        if not online_cmvn and norm.mode != pk.NORM_MODES["speaker"]:
            record0 = None                                     # (no records in mode none)
    dec = None
    if a.decode:
        import tempfile
        from pocketkaldi_amd import synth_graph
        graph = synth_graph.size_for_states(20000, seed=1)
        with tempfile.TemporaryDirectory() as tmp:
            synth_graph.write_fst(os.path.join(tmp, "loop.fst"), graph["start"], graph["final"], graph["arcs"])
            fst = pk.Fst(os.path.join(tmp, "loop.fst"))
        dec = pk.OnlineDecoder(fst, am, a.streams, trace_capacity=a.trace_capacity)
        dec.set_beam(16.0, 2000)
        dec.set_commit(a.commit)
        if a.endpoint:
            dec.set_endpointing(synth_graph.silence_pdfs(graph))

    cores = []                               # --decode: a step's time up to the end of advance
    ends = []                                # ... and up to the end of the endpoint reads and cuts
    cuts = [0]

    def run(record, nsteps=nsteps):
        for s in range(a.streams):
            sc.open_features(s, a.features, speaker_stats=record0) if feats else sc.open(s, speaker_stats=record0)
            if slot_mats:
                sc.set_slot_transform(s, slot_mats[s % 4])
            if dec:
                dec.open(s)
        walls, frames, rows0 = [], 0, []
        del cores[:]
        del ends[:]
        cuts[0] = 0
        for k in range(nsteps + 1):
            t0 = time.perf_counter()
            for s in range(a.streams):
                if k < nsteps and feats:
                    sc.push_features(s, feats[s][k * chunk:(k + 1) * chunk])
                elif k < nsteps:
                    sc.push(s, waves[s][k * chunk:(k + 1) * chunk])
                else:
                    sc.close(s)
            sc.step(0.1, sync=dec is None)
            if dec:
                dec.advance(sc)
                cores.append(time.perf_counter() - t0)
                if a.endpoint and k < nsteps:
                    fired = [s for s in range(a.streams) if dec.endpoint(s).rule]
                    if fired:
                        dec.finish(fired)
                        for s in fired:
                            dec.open(s)
                        cuts[0] += len(fired)
                ends.append(time.perf_counter() - t0)
                if k < nsteps:
                    for s in range(a.streams):
                        dec.partial(s)
            wall = time.perf_counter() - t0
            n = 0
            for s in range(a.streams):
                _, _, c = sc.loglik_device(s)
                n += c
            if record:
                first, r = sc.fetch(0)
                if r.shape[0]:
                    rows0.append(r)
            walls.append(wall)
            frames += n
        return walls, frames, rows0

    run(False, min(nsteps, 100))             # warm-up: a pass of at most 100 steps
    walls, frames, rows0 = run(True)
    walls_ms = np.array(walls) * 1e3
    if synthetic:
        bs = pk.FeatureScorer(am, 1, feats[0].shape[0], global_stats=g, deltas=dspec, transform=xspec)
        bs.set_features(feats[:1], a.features)
    else:
        bs = pk.BatchScorer(am, g, 1, len(waves[0]), frontend=spec, deltas=dspec, transform=xspec)
        bs.set_waves(waves[:1])
    if norm is not None:
        bs.set_norm(norm, pk.cmvn_normalize(feats[0] if feats else bs_rows(bs), pk.NormSpec("utterance", True, True))[1]) \
            if isinstance(norm, pk.OnlineCmvnSpec) else bs.set_norm(norm)
        if record0 is not None:
            bs.set_speaker_stats([record0])
    if slot_mats:                            # (consumed by the score call that follows)
        bs.set_utt_transforms(slot_mats[:1])
    bs.score(0.1)
    ok = np.concatenate(rows0).tobytes() == bs.fetch(0).log_prob().tobytes()
    rec = {
        "streams": a.streams, "seconds": a.seconds, "chunk_ms": a.chunk_ms, "steps": len(walls),
        "input": "features, %s, %d frames a push" % (a.features, chunk) if feats else "audio",
        "model": model_name, "cmvn": a.cmvn, "deltas": a.deltas, "transform": a.transform, "slot_transforms": bool(a.slot_transforms),
        "device": torch.cuda.get_device_name(0),
        "step_ms": {"median": float(np.median(walls_ms)), "p90": float(np.percentile(walls_ms, 90)),
                    "max": float(walls_ms.max())},
        "frames": int(frames),
        "frames_per_s": float(frames / (walls_ms.sum() / 1e3)),
        "rtf": float(np.median(walls_ms) / a.chunk_ms),
        "algorithmic_delay_ms": {"window_and_lookahead": 15.0 + 10.0 * (R + (dspec.order * dspec.window if dspec else 0) + (xf[1] if xf else 0)),
                                 "plus_chunk_at_most": a.chunk_ms},
        "check_stream0_equals_batch": bool(ok),
    }
    if dec:
        per_window = int(round(10000.0 / a.chunk_ms))
        stats = [dec.trace_stats(s) for s in range(a.streams)]
        rec["decoder"] = {"graph": "word loop, about 20000 states", "beam": 16.0, "max_active": 2000, "commit": bool(a.commit),
                          "trace_capacity": int(stats[0][2])}
        cores_ms = np.array(cores) * 1e3
        window = lambda x: {"first_10s": float(np.median(x[:per_window])), "last_10s": float(np.median(x[-1 - per_window:-1]))}
        ends_ms = np.array(ends) * 1e3
        rec["window_ms"] = {"step": window(walls_ms), "advance": window(cores_ms), "partial": window(walls_ms - ends_ms)}
        if a.endpoint:
            rec["window_ms"]["endpoint"] = window(ends_ms - cores_ms)
            rec["endpoint"] = {"silence_pdfs": synth_graph.silence_pdfs(graph), "rules": "the usual five", "cuts": cuts[0]}
        rec["trace"] = {"peak_max": int(max(p for _, p, _ in stats)), "in_use_end_max": int(max(i for i, _, _ in stats)),
                        "committed_arcs_max": int(max(dec.committed(s)[1] for s in range(a.streams))),
                        "committed_arcs_min": int(min(dec.committed(s)[1] for s in range(a.streams))),
                        "tail_arcs_max": int(max(len(dec.best_path_arcs(s)) - dec.committed(s)[1] for s in range(a.streams)))}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
