"""GPU decoder benchmark: 256 x 10 s utterances, model S, a synthetic word-loop graph of about 200 k
states (pocketkaldi_amd/synth_graph.py).  Prints ONE JSON line and writes it to profiles/r06_decode.json
(profiles/r07_decode_gc.json when a trace-gc leg is asked for); exits non-zero if the reference-settings leg misses
a condition:

  score_ms / decode_ms      hipEvents on the batch's stream (score; decode_batch ordered after it)
  gpu_frames_per_s          frames / (score + GPU decode)
  max_active / max_active_bound   the max-active of the 256-utterance leg and the largest active_bound (model S's
                            synthetic outputs are near-flat: the default, 2000, binds; at 30000 the call writes more
                            backtrace records than record indices can number, which --reference-settings decodes
                            with trace gc)
  trace                     pk_mi355_decoder_trace_stats of that leg: the largest peak, the slice, all compactions
  same_work                 the first `cpu_utts` utterances decoded by BOTH decoders at max-active 30000 (the
                            reference's kBeamSize): GPU and CPU (reference decoder, oracle/_ref/libpkref_decoder.so,
                            16 host threads) times, the reference's per-call graph load, and how many results agree
  reference_settings        (--reference-settings) the WHOLE batch at max-active 30000 with trace gc on: decode_ms, the
                            largest active_bound, peak records against the slice, all compactions, and how many of
                            the first `cpu_utts` results equal the reference decoder's (words, weight bits, ok)
  mode_cost                 (--mode-cost) the first leg's call with trace gc off, on, off, on in one session
  alignment_cost            (--alignment) the first leg's call with alignment off, on, off, on on the one decoder in one
                            session (written to profiles/r08_decode_alignment.json): each on-run has an off-run beside
                            it as its yardstick; the frames aligned in the on-runs are counted

    python tools/decode_bench.py [--utts 256] [--seconds 10] [--states 200000] [--cpu-utts 16] [--steps 3]
                                 [--max-active 2000] [--trace-capacity 2^30] [--trace-gc] [--reference-settings]
                                 [--mode-cost] [--alignment]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402  (one HIP runtime in the process: the one torch loads, as bench.py)
import numpy as np  # noqa: E402

import pocketkaldi_amd as pk  # noqa: E402
from pocketkaldi_amd import build as pkbuild, synth, synth_graph as SG  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--states", type=int, default=200000)
    ap.add_argument("--cpu-utts", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    # model S's synthetic outputs are near-flat: without a tighter max-active every utterance keeps tens of
    # thousands of tokens per frame, and 256 x 1000 frames write more records than one shared arena can index
    # (2^31 - 1); with --trace-gc every utterance compacts a slice of its own and max-active 30000 decodes
    ap.add_argument("--max-active", type=int, default=2000)
    ap.add_argument("--trace-capacity", type=int, default=1 << 30)
    ap.add_argument("--trace-gc", action="store_true", help="the first leg with trace gc on (Decoder.set_trace_gc)")
    ap.add_argument("--reference-settings", action="store_true",
                    help="add the leg at the reference's settings: the whole batch at max-active 30000, trace gc on")
    ap.add_argument("--mode-cost", action="store_true", help="add the first leg's call with trace gc off / on / off / on")
    ap.add_argument("--alignment", action="store_true", help="add the first leg's call with alignment off / on / off / on")
    ap.add_argument("--out", default=None, help="profiles/r06_decode.json; profiles/r07_decode_gc.json with any of "
                    "--trace-gc, --reference-settings, --mode-cost")
    a = ap.parse_args()
    if a.out is None:
        gc_run = a.trace_gc or a.reference_settings or a.mode_cost
        a.out = os.path.join(REPO, "profiles", "r08_decode_alignment.json" if a.alignment else
                             "r07_decode_gc.json" if gc_run else "r06_decode.json")

    pk.set_device(0)
    layers, prior, L, R = synth.model("S")
    am = pk.AcousticModel(layers, prior, L, R)
    waves = [synth.utterance(u, a.seconds) for u in range(a.utts)]
    bs = pk.BatchScorer(am, synth.global_cmvn_stats(), a.utts, sum(len(w) for w in waves))
    bs.set_waves(waves)
    g = SG.size_for_states(a.states, seed=1)
    tmp = tempfile.mkdtemp()
    fst_path = os.path.join(tmp, "g.fst")
    SG.write_fst(fst_path, g["start"], g["final"], g["arcs"])
    fst = pk.Fst(fst_path)
    dec = pk.Decoder(fst, am, a.utts, trace_capacity=a.trace_capacity, trace_gc=a.trace_gc)
    stream = torch.cuda.ExternalStream(bs.stream())
    frames = bs.total_frames()

    def timed(max_active, steps):
        """score + decode_batch, `steps` times after a warm-up pass -> (median score ms, median decode ms)."""
        dec.set_beam(16.0, max_active)
        score_ms, decode_ms = [], []
        for step in range(steps + 1):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(stream)
            bs.score(0.1, sync=False)
            e1.record(stream)
            dec.decode_batch(bs, sync=False)
            e2.record(stream)
            dec.synchronize()
            if step:                                     # the first pass warms up
                score_ms.append(e0.elapsed_time(e1))
                decode_ms.append(e1.elapsed_time(e2))
        return float(np.median(score_ms)), float(np.median(decode_ms))

    def trace():
        st = [dec.trace_stats(u) for u in range(a.utts)]
        return dict(max_peak_records=max(p for p, _, _ in st), slice_records=st[0][1], compactions=sum(c for _, _, c in st))

    s_ms, d_ms = timed(a.max_active, a.steps)
    bound = max(dec.active_bound(u) for u in range(a.utts))
    res = dict(kind="decode", utts=a.utts, seconds=a.seconds, frames=int(frames), graph_states=fst.num_states(),
               graph_arcs=fst.num_arcs(), beam=16.0, max_active=a.max_active, trace_gc=bool(a.trace_gc),
               score_ms=round(s_ms, 3), decode_ms=round(d_ms, 3),
               gpu_frames_per_s=round(frames / ((s_ms + d_ms) / 1e3)), max_active_bound=int(bound),
               words_utt0=len(dec.result(0)[0]), trace=trace(), library_build_hash=pkbuild.source_hash()[:16])
    if a.mode_cost:
        legs = []
        for on in (False, True, False, True):
            dec.set_trace_gc(on)
            legs.append(dict(trace_gc=on, decode_ms=round(timed(a.max_active, a.steps)[1], 3), **trace()))
        dec.set_trace_gc(a.trace_gc)
        off_ms = np.mean([x["decode_ms"] for x in legs if not x["trace_gc"]])
        on_ms = np.mean([x["decode_ms"] for x in legs if x["trace_gc"]])
        res["mode_cost"] = dict(max_active=a.max_active, legs=legs, on_over_off=round(float(on_ms / off_ms), 4))
    if a.alignment:
        legs = []
        for on in (False, True, False, True):
            dec.set_alignment(on)
            ms = round(timed(a.max_active, a.steps)[1], 3)
            legs.append(dict(alignment=on, decode_ms=ms,
                             frames_aligned=sum(len(dec.alignment(u)[0]) for u in range(a.utts)) if on else 0))
        dec.set_alignment(False)
        off = [x["decode_ms"] for x in legs if not x["alignment"]]
        on_ms = [x["decode_ms"] for x in legs if x["alignment"]]
        res["alignment_cost"] = dict(max_active=a.max_active, trace_gc=bool(a.trace_gc), legs=legs,
                                     on_over_off=round(float(np.mean(on_ms) / np.mean(off)), 4),
                                     off_spread=round(float(max(off) / min(off)), 4))
    ref = None
    # Same work on both sides: the first cpu_utts utterances at the reference's own max-active (kBeamSize = 30000;
    # pkref_decode cannot take another), decoded by the GPU decoder from the same fetch_all views and by the
    # reference's decoder on 16 host threads.  pkref_decode reads the graph file on every call: that load is timed
    # on its own (a T = 0 decodable) and reported beside the raw figure.
    declib = os.path.join(REPO, "oracle", "_ref", "libpkref_decoder.so")
    if os.path.exists(declib) and a.cpu_utts > 0:
        L = C.CDLL(declib)
        L.pkref_decode.argtypes = [C.c_char_p, C.POINTER(pk.pk_decodable_t), C.POINTER(C.c_int), C.c_int,
                                   C.POINTER(C.c_float), C.POINTER(C.c_int)]
        n = min(a.cpu_utts, a.utts)
        t0 = time.perf_counter()
        views = bs.fetch_all()
        t1 = time.perf_counter()
        same = pk.Decoder(fst, am, n, trace_capacity=a.trace_capacity)
        same.set_beam(16.0, 30000)
        same.decode(views[:n])                               # warm-up (upload path, allocations)
        g0 = time.perf_counter()
        same.decode(views[:n])
        g1 = time.perf_counter()

        def run(u):
            words = (C.c_int * 8192)()
            w, ok = C.c_float(), C.c_int()
            d = views[u]._d
            k = L.pkref_decode(fst_path.encode(), C.byref(d), words, 8192, C.byref(w), C.byref(ok))
            return list(words[:max(k, 0)]), w.value, ok.value

        empty = pk.pk_decodable_t()
        empty.am = am.handle
        l0 = time.perf_counter()
        for _ in range(3):
            L.pkref_decode(fst_path.encode(), C.byref(empty), (C.c_int * 1)(), 1, C.byref(C.c_float()), C.byref(C.c_int()))
        load_ms = (time.perf_counter() - l0) / 3 * 1e3
        c0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            ref = list(ex.map(run, range(n)))
        c1 = time.perf_counter()
        agree = sum(1 for u in range(n) if (same.result(u)[0], np.float32(same.result(u)[1]).tobytes(), same.result(u)[2])
                    == (ref[u][0], np.float32(ref[u][1]).tobytes(), ref[u][2]))
        fr = sum(bs.num_frames(u) for u in range(n))
        cpu_ms = (c1 - c0) * 1e3
        cpu_ms_noload = max(cpu_ms - -(-n // 16) * load_ms, 1e-3)
        res["same_work"] = dict(
            utts=n, frames=int(fr), max_active=30000, note="both decoders at max-active 30000 on the same fetch_all views; "
            "gpu: pk_mi355_decoder_decode wall time (upload included, the n utterances use n CUs); cpu: the reference's "
            "decoder on 16 host threads, whose pkref_decode re-reads the graph file on every call",
            gpu_decode_ms=round((g1 - g0) * 1e3, 3), gpu_frames_per_s=round(fr / (g1 - g0)),
            gpu_max_active_bound=max(same.active_bound(u) for u in range(n)),
            cpu_decode_ms=round(cpu_ms, 3), cpu_frames_per_s=round(fr / (cpu_ms / 1e3)),
            cpu_graph_load_ms_per_call=round(load_ms, 3),
            cpu_decode_ms_without_graph_loads=round(cpu_ms_noload, 3),
            cpu_frames_per_s_without_graph_loads=round(fr / (cpu_ms_noload / 1e3)),
            identical_results=agree, fetch_all_ms=round((t1 - t0) * 1e3, 3))
        del same
    if a.reference_settings:
        # The reference's settings on the whole batch: beam 16, max-active 30000 (kBeamSize), which one shared arena
        # cannot decode; each utterance compacts its own slice instead.
        dec.set_trace_gc(True)
        s_ms, d_ms = timed(30000, a.steps)
        leg = dict(utts=a.utts, frames=int(frames), max_active=30000, trace_capacity=a.trace_capacity,
                   score_ms=round(s_ms, 3), decode_ms=round(d_ms, 3), gpu_frames_per_s=round(frames / ((s_ms + d_ms) / 1e3)),
                   max_active_bound=max(dec.active_bound(u) for u in range(a.utts)), **trace())
        if ref is not None:
            leg["compared_with_reference"] = len(ref)
            leg["identical_results"] = sum(
                1 for u in range(len(ref)) if (dec.result(u)[0], np.float32(dec.result(u)[1]).tobytes(), dec.result(u)[2])
                == (ref[u][0], np.float32(ref[u][1]).tobytes(), ref[u][2]))
        # what the leg has to show, not only record: the call succeeded (it got here), neither max-active bound, and
        # every compared utterance equals the reference's decoder; without the reference's decoder nothing was compared
        leg["conditions_met"] = bool(leg["max_active_bound"] < 30000 and ref is not None and len(ref) > 0
                                     and leg["identical_results"] == len(ref))
        res["reference_settings"] = leg
        dec.set_trace_gc(a.trace_gc)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if a.reference_settings and not res["reference_settings"]["conditions_met"]:
        sys.exit("decode_bench: the reference-settings leg did not meet its conditions (see reference_settings)")


if __name__ == "__main__":
    main()
