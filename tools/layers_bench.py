"""Layer kinds beyond ReLU: what the separate sigmoid and p-norm passes cost in the batch scorer.
Prints ONE JSON line and writes it to profiles/layer_kinds_bench.json.

256 utterances x 998 frames of 40-dim features, left = right = 5 (input 440), four models:
  * sigmoid:      440 -> 4 x (1024 + sigmoid) -> 3000 + softmax
  * relu:         the same affine layers with ReLU (fused into the GEMM's epilogue): sigmoid's comparison
  * pnorm:        440 -> 4 x (3000 -> p-norm 300 + Normalize) -> 3000 + softmax
  * relu_norm:    440 -> 4 x (3000 + ReLU + Normalize) -> 3000 + softmax: the existing kinds at the p-norm model's hidden
                  width.  Its inner affine layers are 3000 x 3000, not 300 x 3000 -- no network of the existing kinds has the
                  p-norm model's affine shapes, because only p-norm narrows the width between two affine layers -- so the
                  two are set side by side, not subtracted.
The step time is a host clock around score(sync=True), all models in one process, alternating, medians; then one more
pass per model with the per-stage device-event timing on (gemm / tail / other slots: "other" holds the new passes, the
Normalize launches and, for the p-norm model, nothing else).  Nothing is asserted.

Per-kernel durations come from a run of their own:
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/layers_bench.py --trace-only
    python tools/layers_bench.py --kernel-stats DIR       (adds them, and each kernel's achieved bytes/s, to the profile)
Bytes per frame, from the shapes: 8 dim for an elementwise kind, 4 (G + 1) out_dim for p-norm.

    python tools/layers_bench.py [--utts 256] [--frames 998] [--steps 5]
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

D, L, R, PDFS = 40, 5, 5, 3000
HBM_PEAK_SPEC, HBM_PEAK_MEASURED = 8.0e12, 6.29e12      # bytes/s: the spec and a float4 copy
TRACE_STEPS = 3                                          # scored passes per model under --trace-only (the first included)


def linear(rng, n_in, n_out):
    return ("linear", (rng.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(np.float32), (0.1 * rng.standard_normal(n_out)).astype(np.float32))


def models():
    rng = np.random.default_rng(27)
    n_in = D * (L + R + 1)
    out = {}
    for name, act in (("sigmoid", [("sigmoid",)]), ("relu", [("relu",)])):
        layers, w = [], n_in
        for _ in range(4):
            layers += [linear(rng, w, 1024)] + act
            w = 1024
        out[name] = layers + [linear(rng, w, PDFS), ("softmax",)]
    layers, w = [], n_in
    for _ in range(4):
        layers += [linear(rng, w, 3000), ("pnorm", 300), ("normalize",)]
        w = 300
    out["pnorm"] = layers + [linear(rng, w, PDFS), ("softmax",)]
    layers, w = [], n_in
    for _ in range(4):
        layers += [linear(rng, w, 3000), ("relu",), ("normalize",)]
        w = 3000
    out["relu_norm"] = layers + [linear(rng, w, PDFS), ("softmax",)]
    return out


def new_pass_bytes_per_frame(layers):
    """{kernel family: bytes per frame} of the new passes of a model, from the shapes."""
    b, w = {}, 0
    for l in layers:
        if l[0] == "linear":
            w = l[1].shape[0]
        elif l[0] in ("sigmoid", "tanh", "add", "mul"):
            b["LayerElementwiseKernel"] = b.get("LayerElementwiseKernel", 0) + 8 * w
        elif l[0] == "pnorm":
            b["PnormPanelKernel"] = b.get("PnormPanelKernel", 0) + 4 * (w // l[1] + 1) * l[1]
            w = l[1]
    return b


def scorers(a):
    feats4 = [(np.random.default_rng(u).standard_normal((a.frames, D)) * 1.5).astype(np.float32) for u in range(4)]
    feats = [feats4[u % 4] for u in range(a.utts)]
    prior = np.full(PDFS, 1.0 / PDFS, np.float32)
    out = {}
    for name, layers in models().items():
        am = pk.AcousticModel(layers, prior, L, R)
        fs = pk.FeatureScorer(am, a.utts, a.utts * a.frames)
        fs.set_features(feats, "normalized")
        out[name] = (am, fs, layers)
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
    per_frame = {}
    for layers in models().values():
        for k, v in new_pass_bytes_per_frame(layers).items():
            per_frame[k] = v
    out = []
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        fam = next((k for k in per_frame if k in name), None)
        if fam is None:
            continue
        calls, total_ns = int(r["Calls"]), float(r["TotalDurationNs"])
        moved = per_frame[fam] * frames * TRACE_STEPS         # every call of the family over the traced passes
        rate = moved / (total_ns * 1e-9)
        out.append(dict(kernel=name, calls=calls, total_ms=round(total_ns / 1e6, 4), average_us=round(total_ns / calls / 1e3, 2),
                        bytes_moved=moved, achieved_tb_per_s=round(rate / 1e12, 3), share_of_hbm_spec=round(rate / HBM_PEAK_SPEC, 3),
                        share_of_hbm_measured_copy=round(rate / HBM_PEAK_MEASURED, 3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=998)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true", help="the sigmoid and p-norm models, %d passes each, nothing written" % TRACE_STEPS)
    ap.add_argument("--kernel-stats", help="directory of a rocprofv3 --kernel-trace --stats run of --trace-only: merged into the profile")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "layer_kinds_bench.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            res = json.load(f)
        res["kernels"] = kernel_stats(a.kernel_stats, res["frames"])
        res["kernels_note"] = ("rocprofv3 --kernel-trace --stats of a run of its own (--trace-only, %d passes per model); bytes from the shapes "
                               "(8 dim per frame for an elementwise kind, 4 (G + 1) out_dim for p-norm), all layers of the family together; "
                               "HBM peak 8.0 TB/s spec, 6.29 TB/s measured with a float4 copy" % TRACE_STEPS)
        print(json.dumps(res))
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        return 0
    if pk.lib().pk_mi355_device_count() < 1:
        print("layers_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    sc = scorers(a)
    if a.trace_only:
        for name in ("sigmoid", "pnorm"):
            for _ in range(TRACE_STEPS):
                sc[name][1].score(0.1)
        return 0
    ms = {k: [] for k in sc}
    for step in range(a.steps + 1):                       # the first pass warms up
        for name, (_, fs, _) in sc.items():
            t0 = time.perf_counter()
            fs.score(0.1)                                 # (sync: returns after the last kernel)
            if step:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    slots = {}
    for name, (_, fs, _) in sc.items():
        fs.enable_timing(True)
        fs.score(0.1)
        fs.score(0.1)
        t = fs.timing()
        slots[name] = {k: dict(ms=round(t[k][0], 4), launches=t[k][1]) for k in ("gemm", "tail", "other")}
        fs.enable_timing(False)
    frames = int(sc["sigmoid"][1].total_frames())
    legs = {}
    for name, (am, fs, layers) in sc.items():
        per_frame = new_pass_bytes_per_frame(layers)
        legs[name] = dict(step_ms=round(float(np.median(ms[name])), 4), step_ms_all=[round(x, 4) for x in ms[name]], slots=slots[name],
                          flops_per_frame=am.flops_per_frame(), new_pass_bytes_per_frame=per_frame,
                          new_pass_bytes=sum(per_frame.values()) * frames)
        fs.close()
        am.close()
    res = dict(kind="layer_kinds", utts=a.utts, frames_per_utt=a.frames, frames=frames, steps=a.steps, feat_dim=D, left_context=L, right_context=R,
               legs=legs, sigmoid_minus_relu_ms=round(legs["sigmoid"]["step_ms"] - legs["relu"]["step_ms"], 4),
               device=torch.cuda.get_device_name(0), library_build_hash=pkbuild.source_hash()[:16], gemm_source_hash=pkbuild.gemm_source_hash())
    print(json.dumps(res))
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
