"""Host-only: the path-to-frames rule of the online alignment (PathFrames, csrc/pk_files.cc) in a process of its own
(tests/cpp/online_align_test.cc: no HIP, no library, no Python), built plain and with ASan + UBSan as
tests/test_symtab_host.py builds symtab_test.cc; what it prints must be the hand-worked frames and, through
WordSegments, the hand-worked segments.  Through the library, without a device: null handles of every new entry are
refused, and pk_mi355_online_recognizer_load reports pk_load's keys in the reference's words and order.  No GPU needed."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

from test_symtab_host import ARCS, CSRC, FIXTURES, G, REPO, SANITIZE, f32_sum_bits

SRC = os.path.join(REPO, "tests", "cpp", "online_align_test.cc")
E_INVALID, E_IO, E_DEVICE = -1, -3, -2
P = None                                         # an epsilon arc's slot: never read

# case -> (path, a cost per arc of the path, the frames decoded, max_frames)
CASES = {
    "eps_between": ([0, 1, 2, 0, 3, 6, 5, 0], [P, 1.0, P, P, 2.5, P, 0.3, P], 3, 8),
    "emitting_ends": ([3, 2, 6, 5, 4], [1.0, P, P, 2.5, 0.3], 3, 3),
    "no_emitting": ([0, 2, 6], [P, P, P], 0, 4),
    "empty": ([], [], 0, 4),
    "mismatch_few": ([1, 2, 3], [1.0, P, 2.5], 3, 8),
    "mismatch_many": ([1, 2, 3], [1.0, P, 2.5], 1, 8),
    "max_smaller": ([1, 0, 3, 4, 5], [1.0, P, 2.5, 0.3, 0.7], 4, 2),
    "max_zero": ([1, 3], [1.0, 2.5], 2, 0),
    "outside_and_nonfinite": ([-1, 1, 7, 3, 5], [P, np.inf, P, np.nan, 0.5], 3, 8),
}
# hand-worked: case -> (return value, [(arc, transition-id, cost)] written)
FRAMES = {
    "eps_between": (3, [(1, 3, 1.0), (3, 4, 2.5), (5, 1, 0.3)]),
    "emitting_ends": (3, [(3, 4, 1.0), (5, 1, 2.5), (4, 2, 0.3)]),
    "no_emitting": (0, []),
    "empty": (0, []),
    "mismatch_few": (E_DEVICE, []),
    "mismatch_many": (E_DEVICE, []),
    "max_smaller": (4, [(1, 3, 1.0), (3, 4, 2.5)]),
    "max_zero": (2, []),
    "outside_and_nonfinite": (3, [(1, 3, np.inf), (3, 4, np.nan), (5, 1, 0.5)]),
}
# hand-worked: case -> [(word, start_frame, num_frames, the segment's arc weights, its frames' costs)]
SEGMENTS = {
    # 0 1 | 2 0 | 3 | 6 5 0: a leading segment over one frame, word 5 on an epsilon arc, word 6, word 8 on an epsilon arc
    "eps_between": [(0, 0, 1, [0.25, 0.5], [1.0]), (5, 1, 0, [0.125, 0.25], []), (6, 1, 1, [1.5], [2.5]),
                    (8, 2, 1, [0.3, 0.2, 0.25], [0.3])],
    "emitting_ends": [(6, 0, 1, [1.5], [1.0]), (5, 1, 0, [0.125], []), (8, 1, 1, [0.3, 0.2], [2.5]), (7, 2, 1, [0.1], [0.3])],
    "no_emitting": [(0, 0, 0, [0.25], []), (5, 0, 0, [0.125], []), (8, 0, 0, [0.3], [])],
    "empty": [],
    # arcs -1 and 7 are outside the graph: epsilon arcs of weight 0
    "outside_and_nonfinite": [(0, 0, 1, [0.5], [np.inf]), (6, 1, 2, [1.5, 0.2], [np.nan, 0.5])],
}


def f32_bits(x):
    return struct.unpack("<I", np.float32(x).tobytes())[0]


@pytest.mark.parametrize("flavour", [
    "plain",
    pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                       reason="a GPU is present: sanitizer builds run on CPU machines only")),
])
def test_path_frames_stand_alone(flavour):
    assert [a[0] for a in ARCS] == [0, 3, 0, 4, 2, 1, 0]       # the graph online_align_test.cc writes down
    binary = os.path.join(REPO, "tests", "cpp", "online_align_test_%s.bin" % flavour)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1"] + (SANITIZE if flavour == "sanitized" else []) +
                          [SRC, os.path.join(CSRC, "pk_files.cc"), "-o", binary])
    run = subprocess.run([binary], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stderr == ""                               # a sanitizer reports there
    out = run.stdout.splitlines()
    assert out[-1] == "online_align_test ok"
    frames, segments = {}, {}
    for line in out:
        head, *items = line.split(" | ")
        if line.startswith("frames "):
            _, name, rc, written = head.split()
            assert int(written) == len(items)
            frames[name] = (int(rc), [(int(a), int(t), int(c, 16)) for a, t, c in (i.split() for i in items)])
        elif line.startswith("segments "):
            _, name, n = head.split()
            assert int(n) == len(items)
            segments[name] = [tuple(int(x, 16) if i >= 3 else int(x) for i, x in enumerate(s.split())) for s in items]
    assert sorted(frames) == sorted(CASES) == sorted(FRAMES) and sorted(segments) == sorted(SEGMENTS)
    for name, (path, costs, decoded, max_frames) in CASES.items():
        # the rule itself, restated: the arcs of the path whose ilabel is not 0
        emitting = [(a, ARCS[a][0], c) for a, c in zip(path, costs) if 0 <= a < len(ARCS) and ARCS[a][0] != 0]
        rc, written = FRAMES[name]
        assert rc == (len(emitting) if len(emitting) == decoded else E_DEVICE), name
        assert [(a, t, f32_bits(c)) for a, t, c in written] == \
            [(a, t, f32_bits(c)) for a, t, c in ([] if rc < 0 else emitting[:max_frames])], name
        assert frames[name] == (rc, [(a, t, f32_bits(c)) for a, t, c in written]), name
    for name, want in SEGMENTS.items():
        assert len(segments[name]) == len(want), name
        for (word, start, count, graph, acoustic), seg in zip(want, segments[name]):
            assert seg[:4] == (word, start, count, f32_sum_bits(graph)), (name, seg)
            assert seg[4] == f32_sum_bits(acoustic), (name, seg)


def test_null_handles_and_missing_keys_are_refused_without_a_device(tmp_path):
    L = pk.lib()
    word = pk.pk_mi355_word_t()
    ints, floats = (C.c_int32 * 4)(), (C.c_float * 4)()
    assert L.pk_mi355_online_decoder_set_alignment(None, 1) == E_INVALID and b"null online decoder" in L.pk_mi355_last_error()
    assert L.pk_mi355_online_decoder_alignment(None, 0, ints, ints, floats, 4) == E_INVALID
    assert L.pk_mi355_online_decoder_num_frames(None, 0) == E_INVALID
    assert L.pk_mi355_online_decoder_word_segments(None, 0, C.byref(word), 1) == E_INVALID
    assert L.pk_mi355_online_recognizer_load(None, 1, 1600, 0) is None and L.pk_mi355_last_error_code() == E_INVALID
    for entry in ("am", "stream", "decoder", "symtab"):
        assert getattr(L, "pk_mi355_online_recognizer_" + entry)(None) is None
        assert L.pk_mi355_last_error_code() == E_INVALID and b"null online recognizer" in L.pk_mi355_last_error()
    for entry in ("open", "close", "finished"):
        assert getattr(L, "pk_mi355_online_recognizer_" + entry)(None, 0) == E_INVALID
    assert L.pk_mi355_online_recognizer_push(None, 0, floats, 4) == E_INVALID
    assert L.pk_mi355_online_recognizer_push_i16(None, 0, (C.c_int16 * 4)(), 4) == E_INVALID
    assert L.pk_mi355_online_recognizer_step(None) == E_INVALID
    assert L.pk_mi355_online_recognizer_partial(None, 0) is None and L.pk_mi355_last_error_code() == E_INVALID
    assert L.pk_mi355_online_recognizer_hyp(None, 0) is None and L.pk_mi355_last_error_code() == E_INVALID
    assert math.isnan(L.pk_mi355_online_recognizer_loglikelihood_per_frame(None, 0))
    L.pk_mi355_online_recognizer_destroy(None)

    # pk_load's own keys, in the reference's words and its order (pocketkaldi.cc:81-124), before any device is needed
    D = os.path.join(G, "refmodel")
    good = open(os.path.join(D, "recognizer.conf")).read()
    for name in os.listdir(D):
        if not name.endswith(".conf"):
            os.symlink(os.path.join(D, name), str(tmp_path / name))

    def load(text, capacity=(2, 1600)):
        p = tmp_path / "model.conf"
        p.write_text(text)
        h = L.pk_mi355_online_recognizer_load(str(p).encode(), capacity[0], capacity[1], 0)
        assert h is None
        return L.pk_mi355_last_error_code(), L.pk_mi355_last_error().decode()

    without = lambda key: "".join(l + "\n" for l in good.splitlines() if not l.startswith(key))
    assert load(without("symbol_table")) == (E_IO, "Unable to find key 'symbol_table' in %s" % (tmp_path / "model.conf"))
    assert load(without("fst")) == (E_IO, "Unable to find key 'fst' in %s" % (tmp_path / "model.conf"))
    assert load(without("fst").replace("symbol_table", "#"))[1].startswith("Unable to find key 'fst'")
    assert load(without("cmvn_stats").replace("symbol_table", "#"))[1].startswith("Unable to find key 'cmvn_stats'")
    os.symlink(FIXTURES["symboltable_test.bin"], str(tmp_path / "four.bin"))
    code, msg = load(good.replace("wordloop_words.bin", "four.bin"))
    assert code == E_INVALID and "output label" in msg and "4 symbols" in msg
    assert load(good, capacity=(0, 1600))[0] == E_INVALID and load(good, capacity=(2, 0))[0] == E_INVALID
    (tmp_path / "nosym.conf").write_text(without("symbol_table"))
    with pytest.raises(pk.PkError, match="Unable to find key 'symbol_table'"):
        pk.OnlineRecognizer(str(tmp_path / "nosym.conf"))
    # the batch recognizer reports the same, word for word: one loader
    p = tmp_path / "model.conf"
    p.write_text(without("fst"))
    assert L.pk_mi355_recognizer_load(str(p).encode(), 0, 2, 16000, 0) is None
    assert L.pk_mi355_last_error().decode() == load(without("fst"))[1]


def test_online_only_flags_are_refused_without_online(capsys):
    from pocketkaldi_amd import recognize
    for argv in (["m.conf", "x.wav", "--partials"], ["m.conf", "x.wav", "--chunk-ms", "50"], ["m.conf", "x.wav", "--ctm", "--partials"],
                 ["m.conf", "x.wav", "--online", "--chunk-ms", "0"], ["m.conf", "x.wav", "--online", "--chunk-ms"]):
        assert recognize.main(argv) == 1
        assert capsys.readouterr().out.startswith("Usage:"), argv
