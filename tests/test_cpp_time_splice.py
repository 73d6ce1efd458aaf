"""The time-splice layer, kind 9, in C++.
  * tests/cpp/time_splice_test.cc: csrc/pk_layers.cc and csrc/pk_files.cc in a process of its own, plain and under ASan +
    UBSan -- the host rule at the edge widths in exactly sized buffers, hashed and compared with the numpy restatement
    (tests/time_splice_cases.py); every refusal; the reader on a well-formed file, on each of its proper prefixes and on
    malformed ones.
  * tests/cpp/time_splice_example.cc over include/pocketkaldi_amd.hpp compiles and links."""
import subprocess

import numpy as np
import pytest

import time_splice_cases as TC
from test_cpp_ark_features import fnv
from test_cpp_transforms import FLAVOURS, h, run_stand_alone

SPECIAL = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000000, 0x00000001, 0x7F800000, 0xFF800000], np.uint32)
WIDTHS = [1, 7, 16, 17, 129]
LISTS = [[0], [-1, 0, 1], [-3, 3], [0, 2], [-2, 1], [-7, 2], [-32, 32]]


def cpp_input(n):
    i = np.arange(n)
    w = h(i + 99).astype(np.uint32)
    at = i % 13 == 5
    w[at] = SPECIAL[(i[at] // 13) % 8]
    return w.view(np.float32)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_host_side_stand_alone(flavour):
    out = run_stand_alone("time_splice_test", flavour, ["pk_layers.cc", "pk_files.cc"])
    want = []
    for li, offsets in enumerate(LISTS):
        lo, hi = TC.lo_hi(offsets)
        for D in WIDTHS:
            for more in (1, 67):
                T = lo + hi + more
                y = TC.time_splice(cpp_input(T * D).reshape(T, D), offsets)
                assert y.shape == (more, len(offsets) * D)
                want.append("splice %d %d %d %s" % (li, D, T, fnv(y.tobytes())))
    assert out[:len(want)] == want
    assert out[len(want):] == ["time_splice_test ok"]


def test_time_splice_example_compiles_and_links():
    """tests/cpp/time_splice_example.cc over include/pocketkaldi_amd.hpp; tests/test_gpu_time_splice.py runs it."""
    from test_cpp_stream import build
    assert "pk_mi355" in subprocess.check_output([build("time_splice_example"), "--link-only"], text=True)
