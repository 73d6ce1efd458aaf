"""Host-only: the symbol-table reader and the word-segment function of csrc/pk_files.cc in a process of their own
(tests/cpp/symtab_test.cc: no HIP, no library, no Python), built plain and with ASan + UBSan.  The strings it prints
must be those of an independent parse of the fixtures' bytes (and the reference's four known answers,
test/symbol_table_test.cc:24-27); its sweep over every header field, every truncation, an offset == buffer_size and a
buffer without its final NUL must end in error codes only; its segments must be the hand-worked ones.  Through the
library, without a device: null handles and a model file without a symbol_table key are refused.  No GPU needed."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
CSRC = os.path.join(REPO, "pocketkaldi_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "symtab_test.cc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FIXTURES = {"symboltable_test.bin": os.path.join(G, "symboltable_test.bin"),
            "wordloop_words.bin": os.path.join(G, "refmodel", "wordloop_words.bin")}


def parse_symtab(path):
    """symbol_table.cc:23-73, restated: -> the strings."""
    raw = open(path, "rb").read()
    assert raw[:4] == b"SYM0"
    section, size, buffer_size = struct.unpack("<iii", raw[4:16])
    assert section == 8 + 4 * size + buffer_size == len(raw) - 8
    offsets = struct.unpack("<%di" % size, raw[16:16 + 4 * size])
    buf = raw[16 + 4 * size:]
    return [buf[o:buf.index(b"\0", o)].decode() for o in offsets]


# the graph of symtab_test.cc: arc id -> (ilabel, olabel, weight), and the acoustic cost of frames 0..3
ARCS = [(0, 0, 0.25), (3, 0, 0.5), (0, 5, 0.125), (4, 6, 1.5), (2, 7, 0.1), (1, 0, 0.2), (0, 8, 0.3)]
AC = [1.0, 2.5, 0.3, 0.7]
# hand-worked: case -> [(word, start_frame, num_frames, the segment's arc weights, its frames' costs)]
SEGMENTS = {
    # path 1 2 3 5: an emitting arc without a word, then word 5 ON AN EPSILON ARC (no frame), then word 6 over two frames
    "eps_olabel": [(0, 0, 1, [0.5], [1.0]), (5, 1, 0, [0.125], []), (6, 1, 2, [1.5, 0.2], [2.5, 0.3])],
    # path 3 2 6 5 4: words 5 and 8 follow each other with no frame between
    "two_olabels_no_frame": [(6, 0, 1, [1.5], [1.0]), (5, 1, 0, [0.125], []), (8, 1, 1, [0.3, 0.2], [2.5]), (7, 2, 1, [0.1], [0.3])],
    # path 0 0 1 3 4: two leading epsilons and an emitting arc before the first word
    "leading_eps": [(0, 0, 1, [0.25, 0.25, 0.5], [1.0]), (6, 1, 1, [1.5], [2.5]), (7, 2, 1, [0.1], [0.3])],
    # path 0 1 5 1 0: no olabel at all -- one segment, word 0
    "no_olabel": [(0, 0, 3, [0.25, 0.5, 0.2, 0.5, 0.25], [1.0, 2.5, 0.3])],
    "empty": [],
    "no_ac": [(0, 0, 1, [0.5], None), (5, 1, 0, [0.125], None), (6, 1, 2, [1.5, 0.2], None)],
}


def f32_sum_bits(values):
    """(float) of the sum in double, in order, of float values."""
    total = 0.0
    for v in values:
        total += float(np.float32(v))
    return struct.unpack("<I", struct.pack("<f", np.float32(total)))[0]


@pytest.mark.parametrize("flavour", [
    "plain",
    pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                       reason="a GPU is present: sanitizer builds run on CPU machines only")),
])
def test_symtab_and_segments_stand_alone(flavour, tmp_path):
    binary = os.path.join(REPO, "tests", "cpp", "symtab_test_%s.bin" % flavour)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1"] + (SANITIZE if flavour == "sanitized" else []) +
                          [SRC, os.path.join(CSRC, "pk_files.cc"), "-o", binary])
    run = subprocess.run([binary, G, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stderr == ""                               # a sanitizer reports there
    out = run.stdout.splitlines()
    assert out[-1] == "symtab_test ok"

    # ---- the strings
    want = []
    for name, path in FIXTURES.items():
        strings = parse_symtab(path)
        want.append("symtab %s size %d" % (name, len(strings)))
        want += ["sym %s %d %s" % (name, i, s) for i, s in enumerate(strings)]
    assert out[:len(want)] == want
    assert parse_symtab(FIXTURES["symboltable_test.bin"]) == ["hello", "world", "cat", "milk"]
    assert len(parse_symtab(FIXTURES["wordloop_words.bin"])) == 7

    # ---- the sweep
    swept = {}
    for line in out:
        m = re.fullmatch(r"sweep (\S+) fields (\d+) cases (\d+) codes((?: -?\d+)+)", line)
        if m:
            swept[m.group(1)] = (int(m.group(2)), int(m.group(3)), {int(c) for c in m.group(4).split()})
    assert sorted(swept) == sorted(FIXTURES)
    for name, (nfields, cases, codes) in swept.items():
        size = len(parse_symtab(FIXTURES[name]))
        assert nfields == 3 + size                         # section size, size, buffer_size and every offset
        assert cases == 8 * nfields + os.path.getsize(FIXTURES[name]) + 2      # x 8 values, and every length 0 .. len + 1
        assert codes == {0, -1, -3}, name                  # a good file, a bad offset, a malformed file
        assert "case %s offset_eq_buffer_size: -1" % name in out
        assert "case %s no_final_nul: -3" % name in out
    assert "case directory_and_missing: -3" in out
    assert "case empty_table: 0" in out

    # ---- the segments
    got = {}
    for line in out:
        if line.startswith("segments "):
            head, *segs = line.split(" | ")
            _, name, n = head.split()
            assert int(n) == len(segs)
            got[name] = [tuple(int(x, 16) if i >= 3 else int(x) for i, x in enumerate(s.split())) for s in segs]
    assert sorted(got) == sorted(SEGMENTS)
    for name, want_segs in SEGMENTS.items():
        assert len(got[name]) == len(want_segs), name
        for (word, start, frames, graph, acoustic), seg in zip(want_segs, got[name]):
            assert seg[:4] == (word, start, frames, f32_sum_bits(graph)), (name, seg)
            if acoustic is None:
                assert math.isnan(struct.unpack("<f", struct.pack("<I", seg[4]))[0]), (name, seg)
            else:
                assert seg[4] == f32_sum_bits(acoustic), (name, seg)


def test_symbol_table_through_the_library(tmp_path):
    st = pk.SymbolTable(FIXTURES["symboltable_test.bin"])
    assert len(st) == 4 and [st[i] for i in range(4)] == ["hello", "world", "cat", "milk"]
    for bad in (-1, 4):
        with pytest.raises(IndexError):
            st[bad]
        assert pk.lib().pk_mi355_last_error_code() == -1
    words = pk.SymbolTable(FIXTURES["wordloop_words.bin"])
    assert [words[i] for i in range(len(words))] == parse_symtab(FIXTURES["wordloop_words.bin"])
    with pytest.raises(pk.PkError) as e:
        pk.SymbolTable(str(tmp_path / "absent.bin"))
    assert e.value.code == -3
    raw = open(FIXTURES["symboltable_test.bin"], "rb").read()
    (tmp_path / "offset.bin").write_bytes(raw[:16] + struct.pack("<i", 21) + raw[20:])     # == buffer_size
    with pytest.raises(pk.PkError) as e:
        pk.SymbolTable(str(tmp_path / "offset.bin"))
    assert e.value.code == -1 and "offset 21" in str(e.value)
    (tmp_path / "cut.bin").write_bytes(raw[:-1])
    with pytest.raises(pk.PkError) as e:
        pk.SymbolTable(str(tmp_path / "cut.bin"))
    assert e.value.code == -3


def test_null_handles_and_missing_keys_are_refused_without_a_device(tmp_path):
    L = pk.lib()
    word = pk.pk_mi355_word_t()
    assert L.pk_mi355_symtab_read(None) is None and L.pk_mi355_last_error_code() == -1
    assert L.pk_mi355_symtab_size(None) == -1
    assert L.pk_mi355_symtab_get(None, 0) is None and L.pk_mi355_last_error_code() == -1
    L.pk_mi355_symtab_destroy(None)
    assert L.pk_mi355_decoder_set_alignment(None, 1) == -1 and b"null decoder" in L.pk_mi355_last_error()
    assert L.pk_mi355_decoder_alignment(None, 0, None, None, None, 0) == -1
    assert L.pk_mi355_decoder_word_segments(None, 0, C.byref(word), 1) == -1
    assert L.pk_mi355_online_decoder_word_segments(None, 0, C.byref(word), 1) == -1
    assert L.pk_mi355_recognizer_load(None, 0, 1, 1000, 0) is None and L.pk_mi355_last_error_code() == -1
    for entry in ("am", "batch", "decoder", "symtab"):
        assert getattr(L, "pk_mi355_recognizer_" + entry)(None) is None and b"null recognizer" in L.pk_mi355_last_error()
    assert L.pk_mi355_recognizer_process(None, None, 0) == -1
    assert L.pk_mi355_recognizer_hyp(None, 0) is None
    assert math.isnan(L.pk_mi355_recognizer_loglikelihood_per_frame(None, 0))
    L.pk_mi355_recognizer_destroy(None)

    # pk_load's own keys, in the reference's words and its order (pocketkaldi.cc:81-124), before any device is needed
    D = os.path.join(G, "refmodel")
    good = open(os.path.join(D, "recognizer.conf")).read()
    for name in os.listdir(D):
        if not name.endswith(".conf"):
            os.symlink(os.path.join(D, name), str(tmp_path / name))

    def load(text, capacity=(2, 16000)):
        p = tmp_path / "model.conf"
        p.write_text(text)
        h = L.pk_mi355_recognizer_load(str(p).encode(), 0, capacity[0], capacity[1], 0)
        assert h is None
        return L.pk_mi355_last_error_code(), L.pk_mi355_last_error().decode()

    without = lambda key: "".join(l + "\n" for l in good.splitlines() if not l.startswith(key))
    assert load(without("symbol_table")) == (-3, "Unable to find key 'symbol_table' in %s" % (tmp_path / "model.conf"))
    assert load(without("fst")) == (-3, "Unable to find key 'fst' in %s" % (tmp_path / "model.conf"))
    assert load(without("fst") .replace("symbol_table", "#"))[1].startswith("Unable to find key 'fst'")
    assert load(without("cmvn_stats").replace("symbol_table", "#"))[1].startswith("Unable to find key 'cmvn_stats'")
    code, msg = load(good.replace("wordloop_words.bin", "absent.bin"))
    assert code == -3 and "cannot open" in msg and "absent.bin" in msg
    # every olabel of the graph needs a name: the reference's four-word table is too short for wordloop.fst's six words
    os.symlink(FIXTURES["symboltable_test.bin"], str(tmp_path / "four.bin"))
    code, msg = load(good.replace("wordloop_words.bin", "four.bin"))
    assert code == -1 and "output label" in msg and "4 symbols" in msg
    assert load(good, capacity=(0, 16000))[0] == -1
    (tmp_path / "nosym.conf").write_text(without("symbol_table"))
    with pytest.raises(pk.PkError, match="Unable to find key 'symbol_table'"):
        pk.Recognizer(str(tmp_path / "nosym.conf"))
