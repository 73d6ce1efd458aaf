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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chunk-ms", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stream_bench.json"))
    a = ap.parse_args()

    pk.set_device(0)
    layers, prior, L, R = synth.model("S")
    am = pk.AcousticModel(layers, prior, L, R)
    g = synth.global_cmvn_stats()
    waves = [synth.utterance(u, a.seconds) for u in range(a.streams)]
    chunk = int(round(a.chunk_ms * synth.SAMPLE_RATE / 1000.0))
    nsteps = (len(waves[0]) + chunk - 1) // chunk
    sc = pk.OnlineScorer(am, g, a.streams, a.streams * chunk)

    def run(record):
        for s in range(a.streams):
            sc.open(s)
        walls, frames, rows0 = [], 0, []
        for k in range(nsteps + 1):
            t0 = time.perf_counter()
            for s in range(a.streams):
                if k < nsteps:
                    sc.push(s, waves[s][k * chunk:(k + 1) * chunk])
                else:
                    sc.close(s)
            sc.step(0.1, sync=True)
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

    run(False)                               # warm-up: one whole pass
    walls, frames, rows0 = run(True)
    walls_ms = np.array(walls) * 1e3
    bs = pk.BatchScorer(am, g, 1, len(waves[0]))
    bs.set_waves(waves[:1])
    bs.score(0.1)
    ok = np.concatenate(rows0).tobytes() == bs.fetch(0).log_prob().tobytes()
    rec = {
        "streams": a.streams, "seconds": a.seconds, "chunk_ms": a.chunk_ms, "steps": len(walls),
        "model": "S (440 -> 4 x 1024 -> 3000, L = R = 5), f32, stable softmax",
        "device": torch.cuda.get_device_name(0),
        "step_ms": {"median": float(np.median(walls_ms)), "p90": float(np.percentile(walls_ms, 90)),
                    "max": float(walls_ms.max())},
        "frames": int(frames),
        "frames_per_s": float(frames / (walls_ms.sum() / 1e3)),
        "rtf": float(np.median(walls_ms) / a.chunk_ms),
        "algorithmic_delay_ms": {"window_and_lookahead": 15.0 + 10.0 * R, "plus_chunk_at_most": a.chunk_ms},
        "check_stream0_equals_batch": bool(ok),
    }
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
