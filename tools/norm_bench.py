"""The normalisation spec: what NormKernel costs in the batch scorer, beside CmvnChainKernel.
Prints ONE JSON line and writes it to profiles/norm_bench.json.

256 utterances x 998 frames at D = 80 through the tiny model, fed as RAW features to one scorer: the PK_MI355_K_CMVN
slot of score() (per-stage timing on) for utterance mode with variance, speaker mode, online CMVN at its defaults with
and without variance, `none`, the sliding rule, and the
same utterances fed as NORMALIZED features -- alternating, medians of five.  Every slot holds FeatureLayoutKernel; the
NORMALIZED leg holds nothing else, so a leg's kernel is its slot minus that one.  The yardstick is the sliding leg's
CmvnChainKernel in the same session: serial in t like NormKernel, which reads the rows twice.
--long N adds one utterance of N frames (60000) in utterance mode: one wave per 64 features walks it, by the rule's own
summation order.

    python tools/norm_bench.py [--utts 256] [--frames 998] [--dim 80] [--steps 5] [--long 60000]
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


def slots(fs, feeds, steps):
    """The cmvn slot of score() for every feed, alternating; the first pass warms up.  -> medians, all values, launches"""
    fs.enable_timing(True)
    ms = {k: [] for k in feeds}
    launches = {}
    for step in range(steps + 1):
        for name, feed in feeds.items():
            feed()
            fs.score(0.1)
            t = fs.timing()
            if step:
                ms[name].append(t["cmvn"][0])
            launches[name] = t["cmvn"][1]
    return ({k: round(float(np.median(v)), 4) for k, v in ms.items()}, {k: [round(x, 4) for x in v] for k, v in ms.items()}, launches)


def features(frames, D, seed):
    return (5.0 * np.random.default_rng(seed).standard_normal((frames, D)) + 3.0).astype(np.float32)


def batch_leg(utts, frames, D, steps):
    layers, prior, L, R = synth.model("tiny", feat_dim=D)
    am = pk.AcousticModel(layers, prior, L, R)
    g = np.concatenate([np.full(D, 3.0 * 2500.0), [2500.0]]).astype(np.float32)
    base = [features(frames, D, u) for u in range(4)]
    raw = [base[u % 4] for u in range(utts)]
    rec4 = [pk.cmvn_normalize(x, pk.NormSpec("utterance", True, True))[1] for x in base]
    rec = [rec4[u % 4] for u in range(utts)]
    fs = pk.FeatureScorer(am, utts, utts * frames, global_stats=g)

    glob = sum(rec4)                                       # online CMVN's global record

    def feed(spec, kind="raw", stats=None):
        def run():
            fs.set_norm(spec, glob) if isinstance(spec, pk.OnlineCmvnSpec) else fs.set_norm(spec)
            if stats is not None:
                fs.set_speaker_stats(stats)
            fs.set_features(raw, kind)
        return run

    feeds = {"utterance_vars": feed(pk.NormSpec("utterance", True, True)), "speaker_vars": feed(pk.NormSpec("speaker", True, True), stats=rec),
             "online_cmvn": feed(pk.OnlineCmvnSpec(), stats=rec), "online_cmvn_vars": feed(pk.OnlineCmvnSpec(norm_vars=True), stats=rec),
             "none": feed(pk.NormSpec("none")), "sliding": feed(pk.NormSpec()), "normalized": feed(pk.NormSpec(), "normalized")}
    med, every, launches = slots(fs, feeds, steps)
    total = int(fs.total_frames())
    # the bits: utterance mode is the host rule, speaker mode on the same records is utterance mode
    feeds["utterance_vars"]()
    fs.score(0.1)
    got = fs.fetch_cmvn(utts - 1)
    same = got.tobytes() == pk.cmvn_normalize(raw[utts - 1], pk.NormSpec("utterance", True, True))[0].tobytes()
    feeds["speaker_vars"]()
    fs.score(0.1)
    same = same and got.tobytes() == fs.fetch_cmvn(utts - 1).tobytes()
    feeds["online_cmvn_vars"]()                            # online CMVN is its host rule
    fs.score(0.1)
    same = same and fs.fetch_cmvn(utts - 1).tobytes() == pk.cmvn_online(raw[utts - 1], pk.OnlineCmvnSpec(norm_vars=True), glob, rec[utts - 1]).tobytes()
    fs.close()
    am.close()
    layout = med["normalized"]
    kernel = {k: round(v - layout, 4) for k, v in med.items() if k != "normalized"}
    return dict(utts=utts, frames_per_utt=frames, frames=total, dim=D, model="tiny at feat_dim %d, L = R = %d" % (D, L), steps=steps,
                cmvn_slot_ms=med, cmvn_slot_ms_all=every, cmvn_slot_launches=launches, kernel_ms=kernel,
                waves=utts * ((D + 63) // 64), norm_over_chain=round(kernel["utterance_vars"] / max(kernel["sliding"], 1e-6), 3),
                speaker_over_chain=round(kernel["speaker_vars"] / max(kernel["sliding"], 1e-6), 3),
                online_cmvn_over_chain=round(kernel["online_cmvn_vars"] / max(kernel["sliding"], 1e-6), 3),
                norm_ns_per_frame_of_a_wave=round(kernel["utterance_vars"] * 1e6 / frames, 2), same_rows=bool(same))


def long_leg(frames, D, steps):
    layers, prior, L, R = synth.model("tiny", feat_dim=D)
    am = pk.AcousticModel(layers, prior, L, R)
    raw = [features(frames, D, 9)]
    fs = pk.FeatureScorer(am, 1, frames)
    feeds = {"utterance_vars": lambda: (fs.set_norm(pk.NormSpec("utterance", True, True)), fs.set_features(raw, "raw")),
             "none": lambda: (fs.set_norm(pk.NormSpec("none")), fs.set_features(raw, "raw"))}
    med, every, _ = slots(fs, feeds, steps)
    fs.close()
    am.close()
    ms = round(med["utterance_vars"] - med["none"], 4)
    return dict(frames=frames, dim=D, cmvn_slot_ms=med, cmvn_slot_ms_all=every, kernel_ms=ms, waves=(D + 63) // 64,
                ns_per_frame_of_a_wave=round(ms * 1e6 / frames, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=998)
    ap.add_argument("--dim", type=int, default=80)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--long", type=int, default=60000, help="frames of the single long utterance (0: skip)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "norm_bench.json"))
    a = ap.parse_args()
    if pk.lib().pk_mi355_device_count() < 1:
        print("norm_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    res = dict(kind="norm", batch=batch_leg(a.utts, a.frames, a.dim, a.steps), device=torch.cuda.get_device_name(0),
               library_build_hash=pkbuild.source_hash()[:16], gemm_source_hash=pkbuild.gemm_source_hash())
    if a.long > 0:
        res["long_utterance"] = long_leg(a.long, a.dim, a.steps)
    print(json.dumps(res))
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["batch"]["same_rows"] else 1


if __name__ == "__main__":
    sys.exit(main())
