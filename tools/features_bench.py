"""Features benchmark: what feeding the batch scorer features costs and saves.  Prints ONE JSON
line and writes it to profiles/features_layout.json.

  layout       tools/ubench/layout_probe (built here if it is missing and there is a hipcc): FeatureLayoutKernel's one
               launch for 256 utterances x 998 frames x 40 features, L = R = 5, hipEvents around the launch alone, median
               of 20 after warm-up; the traffic floor 2 x 4 x 40 bytes per frame at 8 TB/s; and whether Yt is the padded
               transpose.  (The comparison with the per-utterance PadTransposeKernel, since removed, is history: the
               figures recorded in the output file are carried over as layout.pad_transpose_recorded.)
  score        score() of a wave batch (256 x 10 s, model S) beside score() of the same utterances fed as RAW features
               (the wave call's fbank) and as NORMALIZED features (its CMVN) to the same scorer, hipEvents on the
               batch's stream, alternating, medians; the stage times of each (the layout launch is reported in the
               cmvn slot, fbank reports no launch); whether the three gave the same rows
  bench        (--bench-lines FILE) lines "new|old <bench.py JSON line>" collected by the caller from bench.py of this
               tree and of the parent's, alternating in one session: value and ms_per_step of each, medians

    python tools/features_bench.py [--utts 256] [--seconds 10] [--steps 5] [--bench-lines FILE]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402  (one HIP runtime in the process: the one torch loads, as bench.py)
import numpy as np  # noqa: E402

import pocketkaldi_amd as pk  # noqa: E402
from pocketkaldi_amd import build as pkbuild, synth  # noqa: E402

PROBE = os.path.join(REPO, "tools", "ubench", "layout_probe")


def build_probe():
    if os.path.exists(PROBE):
        return
    csrc = os.path.join(REPO, "pocketkaldi_amd", "csrc")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=" + pkbuild.ARCH, "-std=c++17", "-O3",
                           "-ffp-contract=off", "-w", "-I", csrc, "-I", os.path.join(REPO, "include"), PROBE + ".hip",
                           os.path.join(csrc, "features.hip"), "-o", PROBE])


def layout_leg(utts, frames):
    build_probe()
    out = subprocess.run([PROBE, str(utts), str(frames), "40", "5", "5", "20"], capture_output=True, text=True, timeout=120)
    if out.returncode != 0:
        raise RuntimeError("layout_probe failed (%d): %s%s" % (out.returncode, out.stdout, out.stderr))
    return json.loads(out.stdout.strip().splitlines()[-1])


def score_leg(utts, seconds, steps):
    layers, prior, L, R = synth.model("S")
    am = pk.AcousticModel(layers, prior, L, R)
    base = [synth.utterance(u, seconds) for u in range(4)]       # a few distinct utterances, repeated
    waves = [base[u % 4] for u in range(utts)]
    bs = pk.BatchScorer(am, synth.global_cmvn_stats(), utts, sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    fb4, cm4 = [bs.fetch_fbank(u) for u in range(4)], [bs.fetch_cmvn(u) for u in range(4)]
    feeds = {"waves": lambda: bs.set_waves(waves),
             "raw": lambda: bs.set_features([fb4[u % 4] for u in range(utts)], kind="raw"),
             "normalized": lambda: bs.set_features([cm4[u % 4] for u in range(utts)], kind="normalized")}
    stream = torch.cuda.ExternalStream(bs.stream())
    bs.enable_timing(True)
    ms = {k: [] for k in feeds}
    stages, rows = {}, {}
    for step in range(steps + 1):                               # the first pass warms up; the legs alternate
        for name, feed in feeds.items():
            feed()
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record(stream)
            bs.score(0.1, sync=False)
            e1.record(stream)
            bs.synchronize()
            if step:
                ms[name].append(e0.elapsed_time(e1))
            stages[name] = {k: [round(v[0], 4), v[1]] for k, v in bs.timing().items()}
            rows[name] = bs.fetch(utts - 1).log_prob()
    med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    total = bs.total_frames()
    bs.close()
    return dict(utts=utts, seconds=seconds, frames=int(total), model="S", steps=steps, score_ms=med,
                score_ms_all={k: [round(x, 4) for x in v] for k, v in ms.items()},
                saved_ms_raw=round(med["waves"] - med["raw"], 4), saved_ms_normalized=round(med["waves"] - med["normalized"], 4),
                stage_ms_and_launches=stages,
                same_rows=bool(rows["waves"].tobytes() == rows["raw"].tobytes() == rows["normalized"].tobytes()))


def bench_leg(path):
    legs = {"new": [], "old": []}
    with open(path) as f:
        for line in f:
            tag, _, text = line.partition(" ")
            if tag in legs and text.strip().startswith("{"):
                d = json.loads(text)
                legs[tag].append((d["value"], d["ms_per_step"], d["stage_ms_per_step"]))
    out = {}
    for tag, runs in legs.items():
        if runs:
            out[tag] = dict(runs=len(runs), frames_per_s=float(np.median([r[0] for r in runs])),
                            ms_per_step=float(np.median([r[1] for r in runs])), ms_per_step_all=[round(r[1], 4) for r in runs],
                            stage_ms_per_step=runs[-1][2])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "features_layout.json"))
    a = ap.parse_args()
    if pk.lib().pk_mi355_device_count() < 1:
        print("features_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    res = dict(kind="features", layout=layout_leg(a.utts, pk.num_frames(int(a.seconds * 16000))), score=score_leg(a.utts, a.seconds, a.steps),
               library_build_hash=pkbuild.source_hash()[:16], gemm_source_hash=pkbuild.gemm_source_hash())
    if a.bench_lines:
        res["bench"] = dict(what="bench.py --gpus 1 of this tree (new) and of the parent commit's tree (old), alternating in one session",
                            **bench_leg(a.bench_lines))
    try:                                                     # the recorded comparison with the removed kernel stays
        with open(a.out) as f:
            old = json.load(f)["layout"]
        res["layout"]["pad_transpose_recorded"] = old.get("pad_transpose_recorded") or {
            k: v for k, v in old.items() if k.startswith("pad_transpose") or k in ("launches_before", "feature_layout_us")}
    except (OSError, ValueError, KeyError):
        pass
    print(json.dumps(res))
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    lay = res["layout"]
    ok = lay["same_yt"] and res["score"]["same_rows"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
