"""The time-splice layer: what the separate splice passes cost in the batch scorer.
Prints ONE JSON line and writes it to profiles/time_splice_bench.json.

256 utterances x 998 frames of 40-dim features, left = right = 5 (input 440), three models:
  * tdnn:            440 -> 1024, then 3 x (splice {-3, 0, 3} -> 3072 -> 1024 + ReLU), -> 3000 + softmax
  * framewise_k3072: the same 3072 -> 1024 matrices fed frame-wise, their K = 3072 input made by tiling: the Linear in
                     front of each is widened to N = 3072 with its weight rows and bias repeated three times (440 -> 3072,
                     2 x (3072 -> 3072 + ReLU), 3072 -> 1024 + ReLU, -> 3000 + softmax).  Every inner layer reads K = 3072 as
                     the tdnn's do; the tiling itself costs GEMM work (N = 3072 where the tdnn has 1024), which the "gemm"
                     slots of the two legs show.
  * framewise:       440 -> 1024, then 3 x (1024 -> 1024 + ReLU), -> 3000 + softmax: the same depth without time context.
What the splice passes themselves cost is the tdnn model's "other" slot (device events around its TimeSpliceKernel
launches; its ReLUs are fused into the GEMMs) and the kernel trace below.  256 x (998 + 10 + 18) rows are more than one
pass of 262 144: the tdnn's walk has two passes and takes the separate tail launch.
The step time is a host clock around score(sync=True), all models in one process, alternating, medians; then one more
pass per model with the per-stage device-event timing on.  Nothing is asserted.

Per-kernel durations come from a run of their own:
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/time_splice_bench.py --trace-only
    python tools/time_splice_bench.py --kernel-stats DIR     (adds them, and the kernel's achieved bytes/s, to the profile)
Bytes per frame, from the shapes: 4 in_dim read and 4 n in_dim written by every splice.

    python tools/time_splice_bench.py [--utts 256] [--frames 998] [--steps 5]
"""
import argparse
import csv
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402  (one HIP runtime in the process: the one torch loads, as bench.py)
import numpy as np  # noqa: E402

import pocketkaldi_amd as pk  # noqa: E402
from pocketkaldi_amd import build as pkbuild  # noqa: E402

D, L, R, HIDDEN, PDFS = 40, 5, 5, 1024, 3000
OFFSETS = [-3, 0, 3]
HBM_PEAK_SPEC = 8.0e12                                   # bytes/s
TRACE_STEPS = 3                                          # scored passes under --trace-only (the first included)
SPLICE_BYTES_PER_FRAME = 3 * 4 * HIDDEN * (1 + len(OFFSETS))


def linear(rng, n_in, n_out):
    return ("linear", (rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(np.float32), (0.1 * rng.standard_normal(n_out)).astype(np.float32))


def models():
    rng = np.random.default_rng(29)
    n_in = D * (L + R + 1)
    tdnn = [linear(rng, n_in, HIDDEN)]
    for _ in range(3):
        tdnn += [("splice", OFFSETS), linear(rng, len(OFFSETS) * HIDDEN, HIDDEN), ("relu",)]
    tdnn += [linear(rng, HIDDEN, PDFS), ("softmax",)]
    flat = [linear(rng, n_in, HIDDEN)]
    for _ in range(3):
        flat += [linear(rng, HIDDEN, HIDDEN), ("relu",)]
    flat += [linear(rng, HIDDEN, PDFS), ("softmax",)]

    def tiled(l):                                         # the layer whose output is its own, three times side by side
        return ("linear", np.tile(l[1], (len(OFFSETS), 1)), np.tile(l[2], len(OFFSETS)))
    lin = [l for l in tdnn if l[0] == "linear"]           # 440 -> 1024, 3 x (3072 -> 1024), 1024 -> 3000
    k3072 = [tiled(lin[0]), tiled(lin[1]), ("relu",), tiled(lin[2]), ("relu",), lin[3], ("relu",), lin[4], ("softmax",)]
    return {"tdnn": tdnn, "framewise_k3072": k3072, "framewise": flat}


def scorers(a, names):
    feats4 = [(np.random.default_rng(u).standard_normal((a.frames, D)) * 1.5).astype(np.float32) for u in range(4)]
    feats = [feats4[u % 4] for u in range(a.utts)]
    prior = np.full(PDFS, 1.0 / PDFS, np.float32)
    out = {}
    for name, layers in models().items():
        if name not in names:
            continue
        am = pk.AcousticModel(layers, prior, L, R)
        fs = pk.FeatureScorer(am, a.utts, a.utts * a.frames)
        fs.set_features(feats, "normalized")
        out[name] = (am, fs)
    return out


def kernel_stats(directory, frames):
    rows = []
    for root, _, files in os.walk(directory):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                with open(os.path.join(root, f)) as fh:
                    rows += list(csv.DictReader(fh))
    if not rows:
        raise SystemExit("no *kernel_stats.csv under %s" % directory)
    out = []
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if "TimeSpliceKernel" not in name:
            continue
        calls, total_ns = int(r["Calls"]), float(r["TotalDurationNs"])
        moved = SPLICE_BYTES_PER_FRAME * frames * TRACE_STEPS      # the three layers over the traced passes
        rate = moved / (total_ns * 1e-9)
        out.append(dict(kernel=name, calls=calls, total_ms=round(total_ns / 1e6, 4), average_us=round(total_ns / calls / 1e3, 2), bytes_moved=moved,
                        achieved_tb_per_s=round(rate / 1e12, 3), share_of_hbm_spec=round(rate / HBM_PEAK_SPEC, 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=998)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true", help="the tdnn model, %d passes, nothing written" % TRACE_STEPS)
    ap.add_argument("--kernel-stats", help="directory of a rocprofv3 --kernel-trace --stats run of --trace-only: merged into the profile")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "time_splice_bench.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            res = json.load(f)
        res["kernels"] = kernel_stats(a.kernel_stats, res["rows_per_pass"])
        res["kernels_note"] = ("rocprofv3 --kernel-trace --stats of a run of its own (--trace-only, %d passes); bytes from the shapes (4 in_dim read + "
                               "4 n in_dim written per row of the layer stack, the context pads' rows included), the three layers together; HBM peak "
                               "8.0 TB/s spec" % TRACE_STEPS)
        print(json.dumps(res))
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        return 0
    if pk.lib().pk_mi355_device_count() < 1:
        print("time_splice_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    sc = scorers(a, ("tdnn",) if a.trace_only else ("tdnn", "framewise_k3072", "framewise"))
    if a.trace_only:
        for _ in range(TRACE_STEPS):
            sc["tdnn"][1].score(0.1)
        return 0
    ms = {k: [] for k in sc}
    for step in range(a.steps + 1):                       # the first pass warms up
        for name, (_, fs) in sc.items():
            t0 = time.perf_counter()
            fs.score(0.1)                                 # (sync: returns after the last kernel)
            if step:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    slots = {}
    for name, (_, fs) in sc.items():
        fs.enable_timing(True)
        fs.score(0.1)
        fs.score(0.1)
        t = fs.timing()
        slots[name] = {k: dict(ms=round(t[k][0], 4), launches=t[k][1]) for k in ("gemm", "tail", "other")}
        fs.enable_timing(False)
    frames = int(sc["tdnn"][1].total_frames())
    lh, rh = sc["tdnn"][0].time_context()
    rows = a.utts * (a.frames + L + R + lh + rh)          # the rows of the layer stack: every utterance with its pads
    legs = {}
    for name, (am, fs) in sc.items():
        legs[name] = dict(step_ms=round(float(np.median(ms[name])), 4), step_ms_all=[round(x, 4) for x in ms[name]], slots=slots[name],
                          flops_per_frame=am.flops_per_frame())
        fs.close()
        am.close()
    other = legs["tdnn"]["slots"]["other"]["ms"]
    res = dict(kind="time_splice", utts=a.utts, frames_per_utt=a.frames, frames=frames, rows_per_pass=rows, steps=a.steps, feat_dim=D, left_context=L,
               right_context=R, offsets=OFFSETS, time_context=[lh, rh], legs=legs, splice_bytes_per_row=SPLICE_BYTES_PER_FRAME,
               splice_passes_ms=other, splice_passes_tb_per_s=round(SPLICE_BYTES_PER_FRAME * rows / (other * 1e-3) / 1e12, 3) if other > 0 else None,
               device=torch.cuda.get_device_name(0), library_build_hash=pkbuild.source_hash()[:16], gemm_source_hash=pkbuild.gemm_source_hash())
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
