"""The stage plans in C++ ("The two plans"): tests/cpp/plan_test.cc -- csrc/pk_plan.cc in a process of its
own, plain and under ASan + UBSan -- prints the batch plan and the stream plan for every cell of their cross products.
The expected lines below are written out from the table of DESIGN.md, row by row, not by calling the library; the two
must be equal line for line.  Two properties are asserted of the printed plans on top: the fused Cmvn stage occurs for
SLIDING at Db = 40 without deltas only, and every plan for audio or raw rows ends in exactly one write of Yt."""
import os
import re
import subprocess

import pytest

import pocketkaldi_amd as pk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pocketkaldi_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
MODES = ["sliding", "none", "utterance", "speaker", "online"]
RAW, FEATS, DELTA = 1, 2, 4                                     # the bits of `buffers`

# The normalise stage at Db, from d_raw: mode -> (kernel or None, rows afterwards).  SLIDING is the chain here; the fused
# row of the table is told apart below.
NORMALISE = {"none": (None, "d_raw"), "online": ("OnlineCmvn", "d_feats"), "utterance": ("Norm", "d_feats"), "speaker": ("Norm", "d_feats"),
             "sliding": ("CmvnChain", "d_feats")}
BUFFER_BIT = {"d_raw": RAW, "d_feats": FEATS, "d_delta": DELTA}


def batch_line(source, spec, deltas, Db, stats, mode, spk):
    D = 3 * Db if deltas else Db
    steps = []                                                  # (text, rows read, rows written)
    speaker = writes_stats = 0
    if source == "normalized":                                  # the mode is ignored
        steps.append(("FeatureLayout(feats->Yt@%d)" % D, None, None))
    elif source != "nothing" and (stats or mode != "sliding"):
        if source == "waves":
            steps.append(("front:%s(-->d_raw@%d)" % ("FbankAny" if spec else "Fbank", Db), None, "d_raw"))
        if mode == "sliding" and Db == 40 and not deltas:       # the fused row ends the chain
            steps.append(("Cmvn(d_raw->Yt@40)", "d_raw", None))
        else:
            kernel, rows = NORMALISE[mode]
            if kernel:
                steps.append(("%s(d_raw->%s@%d)" % (kernel, rows, Db), "d_raw", rows))
            speaker = int(mode == "online" and spk)
            writes_stats = int(mode == "utterance")
            if deltas:
                steps.append(("Delta(%s->d_delta@%d)" % (rows, Db), rows, "d_delta"))
                rows = "d_delta"
            steps.append(("FeatureLayout(%s->Yt@%d)" % (rows, D), rows, None))
    buffers = 0
    for _, r, w in steps:
        buffers |= BUFFER_BIT.get(r, 0) | BUFFER_BIT.get(w, 0)
    return "batch %s spec=%d deltas=%d Db=%d D=%d stats=%d %s spk=%d:%s | speaker=%d stats=%d buffers=%d" % (
        source, spec, deltas, Db, D, stats, mode, spk, "".join(" " + s[0] for s in steps), speaker, writes_stats, buffers)


def expected_batch():
    lines = [batch_line(source, spec, deltas, Db, 1, mode, spk)
             for source in ("waves", "raw", "normalized") for spec in (1, 0) for deltas in (1, 0) for Db in (40, 13) for mode in MODES
             for spk in (1, 0)]
    lines += [batch_line(source, 0, 0, Db, 0, "sliding", 0) for source in ("waves", "raw", "normalized") for Db in (40, 13)]
    return lines + [batch_line("nothing", 0, 0, 40, 1, "none", 0)]


def stream_line(area, mode, n_front, n_back, max_m, raw_pushed, chain_pushed):
    normaliser = {"sliding": "StreamCmvnChain", "none": "-"}.get(mode, "StreamNorm")
    blocks = []
    if area:                    # one block: every record, all rows in the staging
        blocks.append("[first x%d d_upload %s StreamFeatureLayout]" % (n_front + n_back, normaliser if max_m > 0 or chain_pushed > 0 else "-"))
    else:
        if n_front > 0 and mode == "sliding":
            blocks.append("[first x%d d_rows%s - StreamCmvn]" % (n_front, " RawRows" if raw_pushed > 0 else ""))
        elif n_front > 0:
            blocks.append("[first x%d d_rows %s StreamFeatureLayout]" % (n_front, normaliser if max_m > 0 else "-"))
        if n_back > 0:
            blocks.append("[back x%d d_upload %s StreamFeatureLayout]" % (n_back, normaliser if chain_pushed > 0 else "-"))
    return "stream area=%d %s front=%d back=%d m=%d raw=%d chain=%d: front=%d%s" % (
        area, mode, n_front, n_back, max_m, raw_pushed, chain_pushed, int(n_front > 0), "".join(" " + b for b in blocks))


def expected_stream():
    return [stream_line(area, mode, nf, nb, m, raw, chain) for area in (0, 1) for mode in MODES for nf in (0, 2) for nb in (0, 2) for m in (0, 3)
            for raw in (0, 3) for chain in (0, 3)]


@pytest.mark.parametrize("flavour", [
    "plain",
    pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                       reason="a GPU is present: sanitizer builds run on CPU machines only")),
])
def test_plans_stand_alone(flavour):
    binary_path = os.path.join(REPO, "tests", "cpp", "plan_test_%s.bin" % flavour)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + (SANITIZE if flavour == "sanitized" else []) +
                          [os.path.join(REPO, "tests", "cpp", "plan_test.cc"), os.path.join(CSRC, "pk_plan.cc"), "-o", binary_path])
    run = subprocess.run([binary_path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-4000:]
    assert run.stderr == ""                                  # a sanitizer reports there
    out = run.stdout.splitlines()
    want = expected_batch() + expected_stream() + ["plan_test ok"]
    assert len(want) == 240 + 7 + 320 + 1
    for k, (got, exp) in enumerate(zip(out, want)):
        assert got == exp, "line %d" % k
    assert len(out) == len(want)
    for line in out:
        if not line.startswith("batch"):
            continue
        fused = " sliding " in line and " Db=40 " in line and " deltas=0 " in line and " stats=1 " in line.split(":")[0] and " normalized " not in line
        assert (len(re.findall(r"\bCmvn\(", line)) == 1) == (fused and " nothing " not in line), line
        if line.startswith(("batch waves", "batch raw")) and not (" stats=0 " in line.split(":")[0] and " sliding " in line):
            steps = line.split(":", 1)[1].split("|")[0].split()
            assert sum("->Yt@" in s for s in steps) == 1 and "->Yt@" in steps[-1], line
