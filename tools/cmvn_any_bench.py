"""CMVN at any feature dimension: what CmvnChainKernel costs in the batch scorer.  Prints ONE
JSON line and writes it to profiles/cmvn_any_bench.json (key "batch"; the online legs of tools/stream_bench.py
--feat-dim, when the caller passes their output lines with --stream-lines, go under "online").

256 utterances x 998 frames at D = 80 through the tiny model: score() of the batch fed as RAW features beside score() of
the same utterances fed as NORMALIZED features (the RAW call's fetch_cmvn) to the same scorer, hipEvents on the batch's
stream, alternating, medians of five, per-stage timing on.  The cmvn slot of the RAW leg holds CmvnChainKernel and
FeatureLayoutKernel, that of the NORMALIZED leg FeatureLayoutKernel alone; their difference is the chain.  The chain's
floor is not bandwidth: a wave runs T dependent widen / f64 add / f64 add / narrow steps.

    python tools/cmvn_any_bench.py [--utts 256] [--frames 998] [--dim 80] [--steps 5] [--stream-lines FILE]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402  (one HIP runtime in the process: the one torch loads, as bench.py)
import numpy as np  # noqa: E402

import pocketkaldi_amd as pk  # noqa: E402
from pocketkaldi_amd import build as pkbuild, synth  # noqa: E402


def batch_leg(utts, frames, D, steps):
    layers, prior, L, R = synth.model("tiny", feat_dim=D)
    am = pk.AcousticModel(layers, prior, L, R)
    g = np.concatenate([np.full(D, 3.0 * 2500.0), [2500.0]]).astype(np.float32)
    base = [(5.0 * np.random.default_rng(u).standard_normal((frames, D)) + 3.0).astype(np.float32) for u in range(4)]
    raw = [base[u % 4] for u in range(utts)]
    fs = pk.FeatureScorer(am, utts, utts * frames, global_stats=g)
    fs.set_features(raw, "raw")
    fs.score(0.1)
    norm4 = [fs.fetch_cmvn(u) for u in range(4)]
    norm = [norm4[u % 4] for u in range(utts)]
    feeds = {"raw": lambda: fs.set_features(raw, "raw"), "normalized": lambda: fs.set_features(norm, "normalized")}
    stream = torch.cuda.ExternalStream(fs.stream())
    fs.enable_timing(True)
    ms = {k: [] for k in feeds}
    cmvn = {k: [] for k in feeds}
    stages, rows = {}, {}
    for step in range(steps + 1):                               # the first pass warms up; the legs alternate
        for name, feed in feeds.items():
            feed()
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record(stream)
            fs.score(0.1, sync=False)
            e1.record(stream)
            fs.synchronize()
            t = fs.timing()
            if step:
                ms[name].append(e0.elapsed_time(e1))
                cmvn[name].append(t["cmvn"][0])
            stages[name] = {k: [round(v[0], 4), v[1]] for k, v in t.items()}
            rows[name] = fs.fetch(utts - 1).log_prob()
    med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    slot = {k: round(float(np.median(v)), 4) for k, v in cmvn.items()}
    chain_ms = round(slot["raw"] - slot["normalized"], 4)
    total = int(fs.total_frames())
    fs.close()
    waves = utts * ((D + 63) // 64)
    return dict(utts=utts, frames_per_utt=frames, frames=total, dim=D, model="tiny at feat_dim %d, L = R = %d" % (D, L), steps=steps,
                score_ms=med, score_ms_all={k: [round(x, 4) for x in v] for k, v in ms.items()},
                cmvn_slot_ms=slot, cmvn_slot_ms_all={k: [round(x, 4) for x in v] for k, v in cmvn.items()},
                chain_ms=chain_ms, chain_waves=waves, chain_ns_per_frame_of_a_wave=round(chain_ms * 1e6 / frames, 2),
                chain_bytes=3 * 4 * total * D, chain_gb_per_s=round(3 * 4 * total * D / max(chain_ms, 1e-6) / 1e6, 1),
                stage_ms_and_launches=stages, same_rows=bool(rows["raw"].tobytes() == rows["normalized"].tobytes()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=998)
    ap.add_argument("--dim", type=int, default=80)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--stream-lines", default=None, help="lines '<leg> <stream_bench.py JSON line>' to record under 'online'")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cmvn_any_bench.json"))
    a = ap.parse_args()
    if pk.lib().pk_mi355_device_count() < 1:
        print("cmvn_any_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    res = dict(kind="cmvn_any", batch=batch_leg(a.utts, a.frames, a.dim, a.steps), device=torch.cuda.get_device_name(0),
               library_build_hash=pkbuild.source_hash()[:16], gemm_source_hash=pkbuild.gemm_source_hash())
    if a.stream_lines:
        res["online"] = {}
        with open(a.stream_lines) as f:
            for line in f:
                tag, _, text = line.partition(" ")
                if text.strip().startswith("{"):
                    res["online"][tag] = json.loads(text)
    print(json.dumps(res))
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["batch"]["same_rows"] else 1


if __name__ == "__main__":
    sys.exit(main())
