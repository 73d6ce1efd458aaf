"""A scorer's creation in front of the device, in C++.
  * tests/cpp/create_request_test.cc: the request and its checks in front of the model's (csrc/pk_create.h,
    CheckRequestArgs) for a batch entry and for a live entry with either text for a missing model, and the argument checks
    of the recognizers' load entries (CheckLoadArgs), in a process of its own, plain and under ASan + UBSan.  The expected
    lines are written out here from the order of section 28, not by calling that code."""
import pytest

from test_cpp_stream_deltas import FLAVOURS, run_stand_alone

DELTAS = "-1 deltas spec: order 4 is outside [1, 3]"
XFORM = "-1 transform spec: left_context 17 is outside [0, 16]"
NONFINITE = "-1 transform spec: matrix entry at row 2, column 5 is not finite"
FRONTEND = "-1 front-end spec: num_mel_bins 129 is outside 3 .. 128"
NULL_ARG = "-1 null argument"


def request_lines(head, no_model, live):
    """The model, then null arguments, then the deltas, the transform and (a live entry: here; a batch entry: behind its
    model's dimensions) the front-end spec."""
    front = FRONTEND if live else "ok"
    rows = (("no model", no_model), ("no model, everything else bad too", no_model), ("null argument", NULL_ARG),
            ("null argument, bad specs", NULL_ARG), ("bad deltas", DELTAS), ("bad deltas, transform, front-end", DELTAS),
            ("bad transform", XFORM), ("bad transform, front-end", XFORM), ("transform not finite", NONFINITE), ("bad front-end", front),
            ("bad front-end alone", front), ("all three", "ok"), ("front-end alone", "ok"), ("no spec", "ok"))
    return ["%s %s: %s" % (head, name, verdict) for name, verdict in rows]


def load_lines(kind, needs, capacity):
    """The path and the specs the entry needs ("null path" where it needs none), the specs given in the order front-end,
    deltas, transform, then the capacities.  (The program hands an entry only the specs it takes, and a transform entry
    deltas too.)"""
    null = "-1 null argument" if needs else "-1 null path"
    takes = set(needs) | ({"deltas"} if "transform" in needs else set())
    first_bad = lambda kinds: next((text for k, text in (("frontend", FRONTEND), ("deltas", DELTAS), ("transform", XFORM)) if k in kinds and k in takes), None)
    rows = (("good", "ok"), ("null path", null), ("null path, all else bad", null),
            ("no front-end", null if "frontend" in needs else "ok"), ("no deltas", null if "deltas" in needs else "ok"),
            ("no transform", null if "transform" in needs else "ok"),
            ("bad specs, bad capacity", first_bad({"frontend", "deltas", "transform"}) or capacity),
            ("bad deltas, transform", first_bad({"deltas", "transform"}) or "ok"), ("bad transform", first_bad({"transform"}) or "ok"),
            ("no utterances", capacity), ("no samples", capacity), ("negative trace", capacity))
    return ["load %s %s: %s" % (kind, name, verdict) for name, verdict in rows]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_request_and_load_argument_checks_stand_alone(flavour):
    out = run_stand_alone("create_request_test", ["pk_delta.cc", "pk_transform.cc", "pk_tables.cc", "pk_files.cc"], flavour)
    batch, online = "-1 bad recognizer capacity", "-1 bad online recognizer capacity"
    want = (request_lines("batch", "-4 model not finalized", False) + request_lines("live", "-4 model not finalized", True) +
            request_lines("live (null model)", "-1 null model", True) +
            load_lines("plain", (), batch) + load_lines("frontend", ("frontend",), online) + load_lines("deltas", ("frontend", "deltas"), batch) +
            load_lines("transform", ("frontend", "transform"), online))
    assert out == want + ["create_request_test ok"]
