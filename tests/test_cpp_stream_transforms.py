"""Feature transforms on a live slot in C++.
  * tests/cpp/stream_transform_test.cc: the frame accounting, the fresh-or-ring choice and the host streaming apply of
    csrc/pk_transform.h in a process of its own, plain and under ASan + UBSan; the streaming apply is held there to
    pk_mi355_transform_apply on the whole matrix at every chunking, with a ring of exactly C frames.
  * tests/cpp/stream_transform_plan_test.cc: the transform rows of the stream plan (csrc/pk_plan.cc), printed and compared
    with the lines written out here from the table of DESIGN.md.
  * The numpy restatement (tests/stream_transform_cases.py) against the library's batch rule.
  * tests/cpp/online_transforms_example.cc compiles and links against the header."""
import os
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import stream_transform_cases as ST
import transform_cases as TC
from test_cpp_stream import build
from test_cpp_stream_deltas import FLAVOURS, MODES, run_stand_alone

# (in_dim, Lt, Rt, rows) -> cases: 12 per length of {0, 1, 2, Rt, Rt + 1, C, C + 1, 2C, 2C + 1, 70}
STAND_ALONE = (((1, 0, 0, 1), 48), ((13, 3, 3, 40), 120), ((40, 0, 4, 40), 96), ((5, 5, 0, 7), 96), ((3, 8, 8, 65), 120), ((6, 0, 0, 0), 48))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_accounting_pick_and_streaming_apply_stand_alone(flavour):
    out = run_stand_alone("stream_transform_test", ["pk_transform.cc", "pk_files.cc"], flavour, ["-ffp-contract=off"])
    for (Dp, L, R, rows), cases in STAND_ALONE:
        assert len({0, 1, 2, R, R + 1, L + R, L + R + 1, 2 * (L + R), 2 * (L + R) + 1, 70}) * 12 == cases
    assert out == ["stream transform %d (%d,%d) -> %d: %d cases" % (s + (n,)) for s, n in STAND_ALONE] + ["stream_transform_test ok"]


def plan_line(deltas, glob, slots, area, mode, n_front, n_back, max_m, chain_pushed):
    """The transform rows of the table: one block per step, normaliser -> [StreamDelta] -> [StreamTransform] ->
    [SlotTransform] -> StreamFeatureLayout, never fused, the rows in the upload staging; SLIDING is the chain at every
    base dimension."""
    normaliser = {"sliding": "StreamCmvnChain", "none": "-"}.get(mode, "StreamNorm")
    stages = (" StreamDelta" if deltas else "") + (" StreamTransform" if glob else "") + (" SlotTransform" if slots else "")
    blocks = []
    if area:
        blocks.append("[first x%d d_upload %s%s StreamFeatureLayout]" % (n_front + n_back, normaliser if max_m > 0 or chain_pushed > 0 else "-", stages))
    elif n_back > 0:
        blocks.append("[back x%d d_upload %s%s StreamFeatureLayout]" % (n_back, normaliser if chain_pushed > 0 else "-", stages))
    return "stream transform deltas=%d global=%d slots=%d area=%d %s front=%d back=%d m=%d chain=%d: front=%d%s" % (
        deltas, glob, slots, area, mode, n_front, n_back, max_m, chain_pushed, int(n_front > 0), "".join(" " + b for b in blocks))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_transform_rows_of_the_stream_plan(flavour):
    out = run_stand_alone("stream_transform_plan_test", ["pk_plan.cc"], flavour)
    want = [plan_line(d, g, sl, area, mode, nf, nb, m, chain) for d in (0, 1) for g in (0, 1) for sl in (0, 1) for area in (0, 1) for mode in MODES
            for nf in ((0, 2) if area else (0,)) for nb in (0, 2) for m in ((0, 3) if nf else (0,)) for chain in (0, 3)]
    assert out == want + ["stream_transform_plan_test ok"]
    assert not any("StreamCmvn " in line or line.endswith("StreamCmvn]") for line in out)      # nothing is fused


def test_numpy_restatement_is_the_library_batch_rule_at_every_chunking():
    rng = np.random.default_rng(1)
    for Dp, L, R, rows, affine in ((13, 3, 3, 40, True), (3, 8, 8, 65, False), (5, 5, 0, 7, True)):
        m = TC.matrix(Dp, L, R, rows, affine)
        spec = pk.TransformSpec(m, L, R, in_dim=Dp)
        for T in (1, R + 1, L + R + 1, 2 * (L + R) + 1, 40):
            x = TC.wide(T, Dp, 5 + T)
            want = pk.transform_feats(x, spec)
            assert TC.bits_equal(want, TC.transform(x, m, L, R))
            for how in ST.CHUNKINGS:
                for delay in (0, 1, 2):
                    chunks = ST.chunks_of(T, how, rng)
                    y, made = ST.stream_transform(x, m, L, R, chunks, delay)
                    assert TC.bits_equal(y, want), (Dp, L, R, T, how, delay)
                    assert sum(made) == T and len(made) == max(len(chunks), 1) + delay


def test_online_transforms_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("online_transforms_example"), "--link-only"], text=True)
