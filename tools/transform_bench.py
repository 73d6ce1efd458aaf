"""Feature transforms: what TransformKernel costs in the batch scorer.  Prints ONE JSON line and
writes it to profiles/transform_bench.json.

256 utterances x 998 frames through the tiny model at feat_dim 40, three legs:
  * lda_13x7_to_40:  13 -> +-3 -> 40 affine (the global stage);
  * lda_40x9_to_40:  40 -> +-4 -> 40 linear (the global stage);
  * fmllr_40_to_40:  40 -> 40 affine with a matrix per utterance (the per-utterance stage alone, matrix=None).
Every leg takes the PK_MI355_K_CMVN slot of score() (per-stage timing on) for the transform scorer on RAW rows in mode none
and for THE SAME object fed the host result as NORMALIZED -- alternating, medians of five.  Both hold the layout at
feat_dim and mode none launches no norm kernel, so the kernel's time is the difference.  It is stated beside the bytes
the kernel must move (it reads 4 in_dim and writes 4 * 40 bytes per frame; the matrix stays in cache) and the arithmetic
it does (K products and K adds per output).  Nothing is asserted.

    python tools/transform_bench.py [--utts 256] [--frames 998] [--steps 5]
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

D = 40


def slots(feeds, steps):
    """feeds: {name: (scorer, feed)}.  The cmvn slot of score() for every feed, alternating; the first pass warms up.
    -> medians, all values, launches"""
    ms = {k: [] for k in feeds}
    launches = {}
    for step in range(steps + 1):
        for name, (fs, feed) in feeds.items():
            feed()
            fs.score(0.1)
            t = fs.timing()
            if step:
                ms[name].append(t["cmvn"][0])
            launches[name] = t["cmvn"][1]
    return ({k: round(float(np.median(v)), 4) for k, v in ms.items()}, {k: [round(x, 4) for x in v] for k, v in ms.items()}, launches)


def features(frames, dim, seed):
    return (5.0 * np.random.default_rng(seed).standard_normal((frames, dim)) + 3.0).astype(np.float32)


def matrix(rows, cols, seed):
    return (np.random.default_rng(seed).standard_normal((rows, cols)) / np.sqrt(cols)).astype(np.float32)


def leg(am, utts, frames, in_dim, left, right, affine, per_utt, steps):
    K = (left + right + 1) * in_dim
    base4 = [features(frames, in_dim, u) for u in range(4)]
    raw = [base4[u % 4] for u in range(utts)]
    if per_utt:
        spec = pk.TransformSpec(None, in_dim=in_dim)
        mats4 = [matrix(D, K + (1 if affine else 0), 100 + u) for u in range(4)]
        mats = [mats4[u % 4] for u in range(utts)]
        ready4 = [pk.transform_feats(x, pk.TransformSpec(m, in_dim=in_dim)) for x, m in zip(base4, mats4)]
    else:
        m = matrix(D, K + (1 if affine else 0), 99)
        spec = pk.TransformSpec(m, left, right, in_dim=in_dim)
        mats = None
        ready4 = [pk.transform_feats(x, spec) for x in base4]
    ready = [ready4[u % 4] for u in range(utts)]
    fs = pk.FeatureScorer(am, utts, utts * frames, transform=spec)
    fs.enable_timing(True)
    fs.set_norm(pk.NormSpec("none"))

    def feed_raw():
        fs.set_features(raw, "raw")
        if mats is not None:
            fs.set_utt_transforms(mats)

    feeds = {"transform": (fs, feed_raw), "normalized": (fs, lambda: fs.set_features(ready, "normalized"))}
    med, every, launches = slots(feeds, steps)
    total = int(fs.total_frames())
    feed_raw()                                           # the bits: the scorer's rows are the host rule's
    fs.score(0.1)
    same = fs.fetch_cmvn(utts - 1).tobytes() == ready[utts - 1].tobytes()
    fs.close()
    kernel = round(med["transform"] - med["normalized"], 4)
    moved = total * 4 * (in_dim + D)
    flops = 2 * total * D * K
    return dict(utts=utts, frames_per_utt=frames, frames=total, in_dim=in_dim, left_context=left, right_context=right, rows=D, affine=affine,
                per_utterance=per_utt, K=K, steps=steps, cmvn_slot_ms=med, cmvn_slot_ms_all=every, cmvn_slot_launches=launches,
                transform_kernel_ms=kernel, layout_at_feat_dim_ms=med["normalized"], bytes_moved=moved,
                transform_kernel_gb_per_s=round(moved / max(kernel, 1e-6) / 1e6, 1), products=flops // 2, adds=flops // 2,
                transform_kernel_gflop_per_s=round(flops / max(kernel, 1e-6) / 1e6, 1), live_lanes_of_64=D, same_rows=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=998)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "transform_bench.json"))
    a = ap.parse_args()
    if pk.lib().pk_mi355_device_count() < 1:
        print("transform_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    layers, prior, L, R = synth.model("tiny", feat_dim=D)
    am = pk.AcousticModel(layers, prior, L, R)
    legs = {"lda_13x7_to_40": leg(am, a.utts, a.frames, 13, 3, 3, True, False, a.steps),
            "lda_40x9_to_40": leg(am, a.utts, a.frames, 40, 4, 4, False, False, a.steps),
            "fmllr_40_to_40": leg(am, a.utts, a.frames, 40, 0, 0, True, True, a.steps)}
    am.close()
    res = dict(kind="transform", model="tiny at feat_dim %d, L = R = %d" % (D, L), legs=legs, device=torch.cuda.get_device_name(0),
               library_build_hash=pkbuild.source_hash()[:16], gemm_source_hash=pkbuild.gemm_source_hash())
    print(json.dumps(res))
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
