"""Delta features: what DeltaKernel costs in the batch scorer.  Prints ONE JSON line and writes it
to profiles/delta_bench.json.

256 utterances x 998 frames through the tiny model, for 13 -> 39 and 40 -> 120 (order 2, window 2): the PK_MI355_K_CMVN
slot of score() (per-stage timing on) for
  * a scorer with deltas, RAW rows at the base dimension, in mode none and in utterance mode with variance;
  * a scorer of a base-dimension model under the same two norms, without deltas;
  * the deltas scorer fed NORMALIZED features at feat_dim (the layout at feat_dim and nothing else)
-- alternating, medians of five.  DeltaKernel's time is the `deltas_none` slot minus the `normalized` one (both hold the
layout at feat_dim; mode none launches no norm kernel).  It is stated beside the bytes the kernel must move -- it reads
4 Db and writes 4 (order + 1) Db bytes per frame -- and beside the layout kernel's own time.

    python tools/delta_bench.py [--utts 256] [--frames 998] [--steps 5]
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


def features(frames, D, seed):
    return (5.0 * np.random.default_rng(seed).standard_normal((frames, D)) + 3.0).astype(np.float32)


def leg(utts, frames, Db, spec, steps):
    F = spec.dim(Db)
    layers, prior, L, R = synth.model("tiny", feat_dim=F)
    am = pk.AcousticModel(layers, prior, L, R)
    layers, prior, L, R = synth.model("tiny", feat_dim=Db)
    am_base = pk.AcousticModel(layers, prior, L, R)
    base4 = [features(frames, Db, u) for u in range(4)]
    raw = [base4[u % 4] for u in range(utts)]
    ready4 = [pk.add_deltas(x, spec) for x in base4]
    ready = [ready4[u % 4] for u in range(utts)]
    with_deltas = pk.FeatureScorer(am, utts, utts * frames, deltas=spec)
    without = pk.FeatureScorer(am_base, utts, utts * frames)
    for fs in (with_deltas, without):
        fs.enable_timing(True)
    none, utt = pk.NormSpec("none"), pk.NormSpec("utterance", True, True)

    def feed(fs, norm, feats, kind="raw"):
        def run():
            fs.set_norm(norm)
            fs.set_features(feats, kind)
        return fs, run

    feeds = {"deltas_none": feed(with_deltas, none, raw), "base_none": feed(without, none, raw),
             "deltas_utterance_vars": feed(with_deltas, utt, raw), "base_utterance_vars": feed(without, utt, raw),
             "normalized": feed(with_deltas, none, ready, "normalized")}
    med, every, launches = slots(feeds, steps)
    total = int(with_deltas.total_frames())
    # the bits: the deltas scorer's rows are the host rule's
    feeds["deltas_utterance_vars"][1]()
    with_deltas.score(0.1)
    want = pk.add_deltas(pk.cmvn_normalize(raw[utts - 1], utt)[0], spec)
    same = with_deltas.fetch_cmvn(utts - 1).tobytes() == want.tobytes()
    for o in (with_deltas, without, am, am_base):
        o.close()
    kernel = round(med["deltas_none"] - med["normalized"], 4)
    moved = total * 4 * (Db + F)
    return dict(utts=utts, frames_per_utt=frames, frames=total, base_dim=Db, feat_dim=F, order=spec.order, window=spec.window,
                model="tiny at feat_dim %d and %d, L = R = %d" % (F, Db, L), steps=steps, cmvn_slot_ms=med, cmvn_slot_ms_all=every,
                cmvn_slot_launches=launches, delta_kernel_ms=kernel, layout_at_feat_dim_ms=med["normalized"], layout_at_base_dim_ms=med["base_none"],
                delta_kernel_with_norm_ms=round(med["deltas_utterance_vars"] - med["base_utterance_vars"] - (med["normalized"] - med["base_none"]), 4),
                bytes_moved=moved, delta_kernel_gb_per_s=round(moved / max(kernel, 1e-6) / 1e6, 1), same_rows=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=998)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "delta_bench.json"))
    a = ap.parse_args()
    if pk.lib().pk_mi355_device_count() < 1:
        print("delta_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    spec = pk.DeltaSpec(2, 2)
    res = dict(kind="deltas", legs={"13_to_39": leg(a.utts, a.frames, 13, spec, a.steps), "40_to_120": leg(a.utts, a.frames, 40, spec, a.steps)},
               device=torch.cuda.get_device_name(0), library_build_hash=pkbuild.source_hash()[:16], gemm_source_hash=pkbuild.gemm_source_hash())
    print(json.dumps(res))
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    return 0 if all(v["same_rows"] for v in res["legs"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
