"""The layer kinds 4 to 8 in C++.
  * tests/cpp/layers_test.cc: csrc/pk_layers.cc and csrc/pk_files.cc in a process of its own, plain and under ASan +
    UBSan -- the rules at the edge widths in exactly sized buffers, hashed and compared with the numpy restatement
    (tests/layer_cases.py); every refusal; the reader on a well-formed file of every new kind, on each of its proper
    prefixes and on malformed ones.  Given a file pocketkaldi_amd.write_nnet wrote, it prints what the reader made of it.
  * tests/cpp/layer_kinds_example.cc over include/pocketkaldi_amd.hpp compiles and links."""
import os
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

import layer_cases as LC
from test_cpp_ark_features import fnv
from test_cpp_transforms import FLAVOURS, REPO, h, run_stand_alone

SPECIAL = np.array([0x00000000, 0x80000000, 0x322bcc77, 0xb22bcc77, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00400000, 0x80400000,
                    0x3f800000, 0xbf800000, 0x41880000, 0xc1880000, 0x42b00000, 0xc2b00000, 0x42d00000, 0xc2d00000, 0x5f8ac723, 0xdf8ac723,
                    0x7f800000, 0xff800000, 0x7fc00000, 0x7f800000, 0xff800000], np.uint32)
KINDS = {"add": pk.ADD, "mul": pk.MUL, "sigmoid": pk.SIGMOID, "tanh": pk.TANH}
WIDTHS, ROWS, GROUPS = [1, 7, 16, 17, 129], [1, 67], [1, 2, 5, 10]


def cpp_input(n):
    i = np.arange(n)
    x = ((h(i + 99) >> np.uint64(12)).astype(np.float64) / 16384.0 - 32.0).astype(np.float32)
    at = i % 13 == 5
    x.view(np.uint32)[at] = SPECIAL[(i[at] // 13) % 25]
    return x


def cpp_vector(n):
    return ((h(np.arange(n) + 7) >> np.uint64(12)).astype(np.float64) / 262144.0 - 2.0).astype(np.float32)


def hash_rows(y):
    y = np.ascontiguousarray(y, np.float32).copy()
    y.view(np.uint32)[np.isnan(y)] = 0x7FC00000
    return fnv(y.tobytes())


def test_the_special_table_is_what_the_issue_lists():
    s = SPECIAL.view(np.float32)
    want = np.array([0.0, -0.0, 1e-8, -1e-8, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 5.877472e-39, -5.877472e-39, 1, -1, 17, -17, 88, -88,
                     104, -104, 2e19, -2e19, np.inf, -np.inf], np.float32)
    assert s[:22].tobytes() == want.tobytes() and np.isnan(s[22])


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_host_side_stand_alone(flavour):
    out = run_stand_alone("layers_test", flavour, ["pk_layers.cc", "pk_files.cc"])
    want = []
    for kind in ("add", "mul", "sigmoid", "tanh"):
        for D in WIDTHS:
            for T in ROWS:
                y = LC.apply(kind, cpp_input(T * D).reshape(T, D), cpp_vector(D) if kind in ("add", "mul") else None)
                want.append("rule %d %d %d %s" % (KINDS[kind], D, T, hash_rows(y)))
    for O in WIDTHS:
        for G in GROUPS:
            for T in ROWS:
                want.append("pnorm %d %d %d %s" % (O, G, T, hash_rows(LC.pnorm(cpp_input(T * O * G).reshape(T, O * G), O))))
    assert out[:len(want)] == want
    assert out[len(want):] == ["layers_test ok"]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_reader_takes_what_write_nnet_writes(flavour, tmp_path):
    """All nine kinds through pk.write_nnet and back through ReadNnet, in the stand-alone program: kind, dimensions and
    the bytes of every matrix and vector."""
    from test_layer_kinds_host import all_nine
    layers = all_nine(np.random.default_rng(11))
    path = tmp_path / "nine.nnet"
    pk.write_nnet(str(path), layers)
    binary = os.path.join(REPO, "tests", "cpp", "layers_test_%s.bin" % flavour)
    if not os.path.exists(binary):
        run_stand_alone("layers_test", flavour, ["pk_layers.cc", "pk_files.cc"])
    run = subprocess.run([binary, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-3000:]
    want, width = [], 0
    empty = fnv(b"")
    for l in layers:
        k = pk._LAYER_KIND[l[0]]
        if l[0] == "linear":
            want.append("layer 0 %d %d %s %s" % (l[1].shape[1], l[1].shape[0], fnv(l[1].tobytes()), fnv(l[2].tobytes())))
            width = l[1].shape[0]
        elif l[0] in ("add", "mul"):
            want.append("layer %d %d %d %s %s" % (k, width, width, empty, fnv(l[1].tobytes())))
        elif l[0] == "pnorm":
            want.append("layer %d %d %d %s %s" % (k, width, l[1], empty, empty))
            width = l[1]
        else:
            want.append("layer %d 0 0 %s %s" % (k, empty, empty))
    assert run.stdout.splitlines() == want + ["layers_test ok"]


def test_layer_kinds_example_compiles_and_links():
    """tests/cpp/layer_kinds_example.cc over include/pocketkaldi_amd.hpp; tests/test_gpu_layer_kinds.py runs it."""
    from test_cpp_stream import build
    assert "pk_mi355" in subprocess.check_output([build("layer_kinds_example"), "--link-only"], text=True)
