"""The front-end at a specification: what FbankAnyKernel costs in the batch scorer.  Prints ONE
JSON line and writes it to profiles/frontend_any_bench.json.

256 utterances x 10 s of int16 PCM through the tiny model at the spec's dimension, per-stage timing on: the
PK_MI355_K_FBANK slot of score() -- the one launch of the front-end -- as the median of five steps with all five
listed, for
    reference   FbankKernel (pk_mi355_batch_create's object)
    default     FbankAnyKernel at the default spec, on the same waves in the same run (the two alternate)
    fbank80     80-bin Povey fbank
    mfcc13      13-of-23 MFCC
and, for fbank80, the front-end's share of the whole score step (hipEvents on the batch's stream).

    python tools/frontend_bench.py [--utts 256] [--seconds 10] [--steps 5]
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


def scorer(spec, utts, samples):
    D = 40 if spec is None else spec.dim
    layers, prior, L, R = synth.model("tiny", feat_dim=D)
    am = pk.AcousticModel(layers, prior, L, R)
    g = np.concatenate([np.full(D, 15.0 * 2500.0), [2500.0]]).astype(np.float32)
    bs = pk.BatchScorer(am, g, utts, utts * samples) if spec is None else pk.BatchScorer(am, g, utts, utts * samples, frontend=spec)
    bs.enable_timing(True)
    return am, bs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frontend_any_bench.json"))
    a = ap.parse_args()
    if pk.lib().pk_mi355_device_count() < 1:
        print("frontend_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    samples = int(16000 * a.seconds)
    base = [synth.utterance(100 + u, a.seconds) for u in range(4)]
    waves = [np.ascontiguousarray(base[u % 4][:samples], np.int16) for u in range(a.utts)]
    samples = min(w.size for w in waves)
    specs = {"reference": None, "default": pk.frontend_default(),
             "fbank80": pk.FrontendSpec("fbank", 80, None, "povey"), "mfcc13": pk.FrontendSpec("mfcc", 23, 13, "povey")}
    objs = {k: scorer(s, a.utts, samples) for k, s in specs.items()}
    for _, bs in objs.values():
        bs.set_waves_i16(waves)
    slot = {k: [] for k in objs}
    score_ms = {k: [] for k in objs}
    stages = {}
    for step in range(a.steps + 1):                             # the first pass warms up; the legs alternate
        for name, (_, bs) in objs.items():
            stream = torch.cuda.ExternalStream(bs.stream())
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record(stream)
            bs.score(0.1, sync=False)
            e1.record(stream)
            bs.synchronize()
            t = bs.timing()
            if step:
                slot[name].append(t["fbank"][0])
                score_ms[name].append(e0.elapsed_time(e1))
            stages[name] = {k: [round(v[0], 4), v[1]] for k, v in t.items()}
    same = bool(objs["reference"][1].fetch_fbank(0).tobytes() == objs["default"][1].fetch_fbank(0).tobytes())
    frames = int(objs["reference"][1].total_frames())
    med = {k: round(float(np.median(v)), 4) for k, v in slot.items()}
    med_score = {k: round(float(np.median(v)), 4) for k, v in score_ms.items()}
    res = dict(kind="frontend_any", utts=a.utts, samples_per_utt=samples, frames=frames, steps=a.steps,
               fbank_slot_ms=med, fbank_slot_ms_all={k: [round(x, 4) for x in v] for k, v in slot.items()},
               default_over_reference=round(med["default"] / max(med["reference"], 1e-9), 3),
               ns_per_frame={k: round(v * 1e6 / frames, 2) for k, v in med.items()},
               score_ms=med_score, score_ms_all={k: [round(x, 4) for x in v] for k, v in score_ms.items()},
               fbank80_share_of_score=round(med["fbank80"] / max(med_score["fbank80"], 1e-9), 4),
               stage_ms_and_launches=stages, default_rows_equal_reference=same,
               model="tiny at the spec's dimension", device=torch.cuda.get_device_name(0),
               library_build_hash=pkbuild.source_hash()[:16], gemm_source_hash=pkbuild.gemm_source_hash())
    print(json.dumps(res))
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    for am, bs in objs.values():
        bs.close()
        am.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
