"""Host-only: the file readers of csrc/pk_files.cc in a process of their own (tests/cpp/files_test.cc: no HIP, no
library, no Python), built plain and with ASan + UBSan.  What the program reads from the reference-written fixtures
must hash to what independent Python parsers get -- the model from the TEXT it was converted from
(tests/refmodel_text.py), the graphs from the bytes of the fixture -- and its sweep over every header field and
section boundary must end in error codes only.  No GPU needed."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk
from refmodel_text import DIR, load_text_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
CSRC = os.path.join(REPO, "pocketkaldi_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "files_test.cc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TYPE_ID = {"linear": 0, "relu": 1, "normalize": 2, "softmax": 3}       # nnet.h


def fnv(data):
    h = 14695981039346656037
    for byte in bytes(data):
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def arr(values, dtype):
    return np.ascontiguousarray(values, dtype).tobytes()


def parse_fst(path):
    """-> (num_states, num_arcs, start, final bytes, first, arcs as int32 [na][4] with the weight's bits)"""
    raw = open(path, "rb").read()
    ns, na, start = struct.unpack("<iii", raw[36:48])
    first = np.frombuffer(raw, "<i4", ns, 48 + 4 * ns)
    arcs = np.frombuffer(raw, "<i4", 4 * na, 48 + 8 * ns).reshape(na, 4)
    return ns, na, start, raw[48:48 + 4 * ns], first, arcs


def arc_ranges(ns, na, first):
    """Fst::CountArcs as tests/test_fst_host.py::count_arcs states it: (first, count) per state."""
    out = []
    for s in range(ns):
        nxt = [first[t] for t in range(s + 1, ns) if first[t] > 0]
        out.append((0, 0) if first[s] < 0 else (int(first[s]), int(nxt[0] if nxt else na) - int(first[s])))
    return out


def expected_graph_lines(name, path, tid2pdf):
    ns, na, start, final, first, arcs = parse_fst(path)
    ranges = arc_ranges(ns, na, first)
    lines = ["fst %s states %d arcs %d start %d final %s first %s arc_first %s arc_count %s arcs %s" % (
        name, ns, na, start, fnv(final), fnv(arr(first, "<i4")), fnv(arr([r[0] for r in ranges], "<i4")),
        fnv(arr([r[1] for r in ranges], "<i4")), fnv(arcs.tobytes()))]
    off, src, arc = {"e": [0], "n": [0]}, {"e": [], "n": []}, {"e": [], "n": []}
    for s, (lo, count) in enumerate(ranges):
        for a in range(lo, lo + count):
            nxt, ilabel, _, wbits = (int(v) for v in arcs[a])
            k = "e" if ilabel else "n"
            arc[k].append((nxt, int(tid2pdf[ilabel]) if ilabel else 0, wbits, a))
            src[k].append(s)
        off["e"].append(len(arc["e"]))
        off["n"].append(len(arc["n"]))
    lines.append("split %s e %d n %d e_off %s n_off %s e_src %s n_src %s e_arc %s n_arc %s olabel %s" % (
        name, len(arc["e"]), len(arc["n"]), fnv(arr(off["e"], "<i4")), fnv(arr(off["n"], "<i4")), fnv(arr(src["e"], "<i4")),
        fnv(arr(src["n"], "<i4")), fnv(arr(arc["e"], "<i4")), fnv(arr(arc["n"], "<i4")), fnv(arr(arcs[:, 2], "<i4"))))
    return lines, 4 + ns + 3 * na           # header fields: size, states, arcs, start; first[]; next / ilabel / olabel per arc


def expectations():
    """-> (the program's positive lines, {file: (number of 4-byte header fields, number of MAT0 sections)})"""
    layers, prior, left, right, tid2pdf, cmvn41 = load_text_model()
    lines = ["nnet layers %d" % len(layers)]
    nnet_fields = 2                         # NNT0: section size, layer count
    for i, layer in enumerate(layers):
        nnet_fields += 2                    # LAY0: section size, type
        if layer[0] == "linear":
            W, b = layer[1], layer[2]
            lines.append("layer %d type 0 in %d out %d W %s b %s" % (i, W.shape[1], W.shape[0], fnv(arr(W, "<f4")), fnv(arr(b, "<f4"))))
            nnet_fields += 3 + 2 * (W.shape[0] + 1)     # MAT0: section size, rows, cols; a VEC0 (bytes, n) per row and the bias
        else:
            lines.append("layer %d type %d in 0 out 0 W %s b %s" % (i, TYPE_ID[layer[0]], fnv(b""), fnv(b"")))
    lines.append("prior n %d %s" % (len(prior), fnv(arr(prior, "<f4"))))
    lines.append("tid2pdf n %d %s" % (len(tid2pdf), fnv(arr(tid2pdf, "<i4"))))
    lines.append("cmvn n 41 %s" % fnv(arr(cmvn41, "<f4")))
    lines.append("conf left %d right %d num_pdfs %d stats %s nnet %s prior %s tid2pdf %s" % (
        left, right, len(prior), fnv(arr(cmvn41, "<f4")), os.path.join(DIR, "refmodel.nnet"), os.path.join(DIR, "refmodel.prior"),
        os.path.join(DIR, "refmodel_tid2pdf.bin")))
    wav = open(os.path.join(G, "en-us-hello.wav"), "rb").read()
    samples = np.frombuffer(wav, "<i2", offset=44).astype(np.float32)
    lines.append("wav n %d %s" % (len(samples), fnv(arr(samples, "<f4"))))
    fields = {"refmodel.nnet": (nnet_fields, sum(layer[0] == "linear" for layer in layers)),
              "mat0_40_bytes": (7, 1),      # the issue's 40-byte file: NNT0 (2), LAY0 (2), MAT0 (3) and no row
              "refmodel.prior": (2, 0), "refmodel_tid2pdf.bin": (2, 0), "refmodel_cmvn.bin": (2, 0),
              "refmodel.conf": (0, 0),      # text: truncations only
              "en-us-hello.wav": (7, 0)}    # chunk size, fmt size, format|channels, rate, byte rate, align|bits, data size
    for name, path in (("testinput.fst", os.path.join(G, "testinput.fst")), ("wordloop.fst", os.path.join(DIR, "wordloop.fst"))):
        graph_lines, graph_fields = expected_graph_lines(name, path, tid2pdf)
        fields[name] = (graph_fields, 0)
        lines += graph_lines
    return lines, fields


@pytest.mark.parametrize("flavour", [
    "plain",
    pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                       reason="a GPU is present: sanitizer builds run on CPU machines only")),
])
def test_file_readers_stand_alone(flavour, tmp_path):
    binary = os.path.join(REPO, "tests", "cpp", "files_test_%s.bin" % flavour)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1"] + (SANITIZE if flavour == "sanitized" else []) +
                          [SRC, os.path.join(CSRC, "pk_files.cc"), "-o", binary])
    run = subprocess.run([binary, G, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stderr == ""                               # a sanitizer reports there
    out = run.stdout.splitlines()
    assert out[-1] == "files_test ok"

    want, fields = expectations()
    assert out[:len(want)] == want

    swept = {}
    for line in out:
        m = re.fullmatch(r"sweep (\S+) fields (\d+) mats (\d+) cases (\d+) codes((?: -?\d+)+)", line)
        if m:
            swept[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)), {int(c) for c in m.group(5).split()})
    assert sorted(swept) == sorted(fields)
    for name, (nfields, nmats, cases, codes) in swept.items():
        assert (nfields, nmats) == fields[name], name
        assert cases > 8 * nfields + 64 * nmats, name      # every field x 8 values, rows x cols of every MAT0 x 8 x 8, and the truncations
        assert codes <= {0, -1, -3} and -3 in codes, name
    for regression in ("mat0 1073741824 x 1073741824", "mat0 1048576 x 1048576", "mat0 1073741824 x 2147483647",
                       "mat0 2147483647 x 1073741824", "vec0 n 1073741824", "directory"):
        assert "regression %s: -3" % regression in out
