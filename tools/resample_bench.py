"""Resampler benchmark: 256 x 10 s utterances at 48000 Hz and at 44100 Hz through BatchScorer.set_waves(rates=...) +
score, beside set_waves + score of the same audio already at 16 kHz (converted beforehand by pk.resample, the same
kernel).  Prints ONE JSON line and writes it to profiles/resample.json.

  native_ms / plain_ms   hipEvents on the batch's stream around [set_waves, score] -- the upload, the conversion and
                         the scoring of the whole batch -- the two legs alternating in one session, medians
  extra_ms               native_ms - plain_ms: what audio at this rate costs more than 16 kHz audio (its larger upload
                         and the conversion)
  score_ms               score alone (no upload), for scale
  same_rows              the log-likelihoods of the two legs are the same bits
  traffic_gb             what ResampleKernel must move: 4 B x (samples in + samples out)

The kernel's own time is not separable with events from outside the call; take it from
`rocprofv3 --kernel-trace --stats -- python tools/resample_bench.py` in a run of its own (ResampleKernel).

    python tools/resample_bench.py [--utts 256] [--seconds 10] [--steps 5] [--rates 48000,44100]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rates", default="48000,44100")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample.json"))
    a = ap.parse_args()
    rates = [int(r) for r in a.rates.split(",")]
    if pk.lib().pk_mi355_device_count() < 1:
        print("resample_bench: no GPU; nothing is measured without one", file=sys.stderr)
        return 1
    layers, prior, L, R = synth.model("S")
    am = pk.AcousticModel(layers, prior, L, R)
    legs = []
    for rate in rates:
        n_in = int(a.seconds * rate)
        rng = np.random.default_rng(rate)
        # a few distinct utterances, repeated: the kernel's work does not depend on the sample values
        base = [np.round(3000 * rng.standard_normal(n_in)).astype(np.float32) for _ in range(4)]
        native = [base[u % 4] for u in range(a.utts)]
        converted4 = [pk.resample(w, rate) for w in base]
        plain = [converted4[u % 4] for u in range(a.utts)]
        n_out = len(plain[0])
        bs = pk.BatchScorer(am, synth.global_cmvn_stats(), a.utts, a.utts * n_out)
        stream = torch.cuda.ExternalStream(bs.stream())

        def timed(set_waves):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record(stream)
            set_waves()
            bs.score(0.1, sync=False)
            e1.record(stream)
            bs.synchronize()
            return e0.elapsed_time(e1)

        def score_only():
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record(stream)
            bs.score(0.1, sync=False)
            e1.record(stream)
            bs.synchronize()
            return e0.elapsed_time(e1)

        native_ms, plain_ms, score_ms = [], [], []
        rows = {}
        for step in range(a.steps + 1):                    # the first pass warms up; the legs alternate
            t = timed(lambda: bs.set_waves(native, rates=[rate] * a.utts))
            rows["native"] = bs.fetch(a.utts - 1).log_prob()
            s = score_only()
            p = timed(lambda: bs.set_waves(plain))
            rows["plain"] = bs.fetch(a.utts - 1).log_prob()
            if step:
                native_ms.append(t)
                plain_ms.append(p)
                score_ms.append(s)
        same = rows["native"].tobytes() == rows["plain"].tobytes()
        med = lambda x: float(np.median(x))
        legs.append(dict(rate=rate, utts=a.utts, seconds=a.seconds, samples_in=a.utts * n_in, samples_out=a.utts * n_out,
                         traffic_gb=round(4.0 * a.utts * (n_in + n_out) / 1e9, 3),
                         native_ms=round(med(native_ms), 3), plain_ms=round(med(plain_ms), 3),
                         extra_ms=round(med(native_ms) - med(plain_ms), 3), score_ms=round(med(score_ms), 3),
                         native_ms_all=[round(x, 3) for x in native_ms], plain_ms_all=[round(x, 3) for x in plain_ms],
                         same_rows=bool(same)))
        bs.close()
    res = dict(kind="resample", what="set_waves(rates) + score beside set_waves + score of the same audio at 16 kHz, hipEvents "
               "on the batch's stream, alternating in one session; uploads from pageable host memory included",
               steps=a.steps, legs=legs, library_build_hash=pkbuild.source_hash()[:16])
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    return 0 if all(l["same_rows"] for l in legs) else 1


if __name__ == "__main__":
    sys.exit(main())
