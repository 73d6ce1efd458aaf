"""Host-only: the Kaldi archive / script-file reader (csrc/pk_ark.cc), from Python and in a
process of its own (tests/cpp/ark_test.cc: no HIP, no library, no Python; built plain and with ASan + UBSan).  The
files are written here with struct.pack, from the format's public definition -- an independent writer.  Values are
compared as bits; doubles and text go through a numpy float32 cast.  No GPU needed."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pocketkaldi_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "ark_test.cc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
E_INVALID, E_IO = -1, -3


def fnv(data):
    h = 14695981039346656037
    for byte in bytes(data):
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def binary(a, double=False, token=None, size=4):
    a = np.asarray(a)
    head = b"\0B" + (token or (b"DM " if double else b"FM "))
    head += struct.pack("<Bi", size, a.shape[0]) + struct.pack("<Bi", size, a.shape[1])
    return head + np.ascontiguousarray(a, "<f8" if double else "<f4").tobytes()


def text(a):
    a = np.asarray(a, np.float64)
    if a.shape[0] == 0:
        return b" [ ]\n"
    rows = ["  " + " ".join(repr(float(v)) for v in row) for row in a]
    return (" [\n" + " \n".join(rows) + " ]\n").encode()


def as_float32(a, how):
    """What the reader must return for a matrix written as `how`."""
    a = np.asarray(a)
    if how == "float":
        return np.ascontiguousarray(a, np.float32)
    with np.errstate(over="ignore"):                         # (1e300 narrows to inf, as the reader's cast does)
        return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))  # one cast from double


def same_bits(got, want):
    want = np.ascontiguousarray(want, np.float32)
    return got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes()


def entries():
    """(key, matrix, how written): float, double and text mixed, a 0 x D matrix, keys of 1 and of 200 bytes."""
    rng = np.random.default_rng(0xA4C)
    f = rng.standard_normal((7, 13)).astype(np.float32)
    f.reshape(-1)[:4] = np.array([0x7FC00001, 0x80000000, 0x00000001, 0xFF800000], np.uint32).view(np.float32)   # payload, -0.0, subnormal, -inf
    d = rng.standard_normal((5, 80)) * 1e3
    d[0, :3] = [1e300, -1e-300, np.pi]                       # narrowed to inf, -0.0, the nearest float
    t = rng.standard_normal((4, 3))
    t[1] = [np.nan, np.inf, -np.inf]
    return [("a", f, "float"), ("utt-double", d, "double"), ("k" * 200, t, "text"), ("empty", np.zeros((0, 13), np.float32), "float"),
            ("empty-text", np.zeros((0, 0)), "text"), ("one-row", rng.standard_normal((1, 41)).astype(np.float32), "float")]


def write_archive(path, items):
    """-> {key: byte offset of its object}"""
    offsets = {}
    with open(path, "wb") as f:
        for key, m, how in items:
            f.write(key.encode() + b" ")
            offsets[key] = f.tell()
            f.write(text(m) if how == "text" else binary(m, double=how == "double"))
    return offsets


def check_entries(got, items):
    assert [k for k, _ in got] == [k for k, _, _ in items]
    for (key, m), (_, want, how) in zip(got, items):
        if how == "text" and want.shape[0] == 0:
            assert m.shape[0] == 0, key
            continue
        w = as_float32(want, how)
        nan = np.isnan(w)
        assert m.shape == w.shape and np.array_equal(np.isnan(m), nan), key
        if how == "float":
            assert same_bits(m, w), key                      # NaN payloads too
        else:
            assert np.array_equal(m.view(np.uint32)[~nan], w.view(np.uint32)[~nan]), key


# ---------------------------------------------------------------- reading

def test_mixed_archive_and_script_files(tmp_path):
    items = entries()
    ark = str(tmp_path / "feats.ark")
    offsets = write_archive(ark, items)
    for spec in (ark, "ark:" + ark, "ark,t:" + ark):
        check_entries(list(pk.ArkReader(spec)), items)
    # scp with offsets into the archive, in another order; and without offsets, one keyless object per file
    order = [items[i] for i in (3, 0, 5, 2, 1, 4)]
    with_offsets = str(tmp_path / "feats.scp")
    with open(with_offsets, "w") as f:
        f.write("".join("%s %s:%d\n" % (k, ark, offsets[k]) for k, _, _ in order))
    check_entries(list(pk.ArkReader(with_offsets)), order)
    check_entries(list(pk.ArkReader("scp:" + with_offsets)), order)
    plain = str(tmp_path / "list.txt")
    with open(plain, "w") as f:
        for i, (k, m, how) in enumerate(items):
            p = str(tmp_path / ("obj%d.mat" % i))
            open(p, "wb").write(text(m) if how == "text" else binary(m, double=how == "double"))
            f.write("%s %s\n" % (k, p))
        f.write("\n")
    check_entries(list(pk.ArkReader("scp:" + plain)), items)
    with pk.ArkReader(ark) as r:                             # entry by entry: the reader can be left early
        assert next(r)[0] == "a"


def test_keyless_objects_and_global_statistics(tmp_path):
    D = 80
    stats = np.zeros((2, D + 1))
    stats[0, :D], stats[0, D] = np.arange(D) * 1234.5678, 2500
    stats[1, :D] = 1e9
    for name, blob in (("bin", binary(stats, double=True)), ("text", text(stats)), ("float", binary(stats.astype(np.float32)))):
        p = str(tmp_path / ("cmvn." + name))
        open(p, "wb").write(blob)
        assert same_bits(pk.read_kaldi_matrix(p), stats.astype(np.float32)), name
        g = pk.kaldi_global_stats(p)
        assert g.shape == (D + 1,) and same_bits(g, stats[0].astype(np.float32)) and g[D] == 2500
    p = str(tmp_path / "padded.bin")
    open(p, "wb").write(b"xyz" + binary(stats, double=True))
    assert same_bits(pk.read_kaldi_matrix(p + ":3"), stats.astype(np.float32))
    for rows in (1, 3):                                      # any other row count is refused
        open(p, "wb").write(binary(np.zeros((rows, D + 1), np.float32)))
        with pytest.raises(pk.PkCodeError, match="2 x") as e:
            pk.kaldi_global_stats(p)
        assert e.value.code == E_INVALID


# ---------------------------------------------------------------- refusals, by code and by a word of the text

def refusal(spec, read_object=False):
    with pytest.raises(pk.PkCodeError) as e:
        pk.read_kaldi_matrix(spec) if read_object else list(pk.ArkReader(spec))
    return e.value.code, str(e.value)


def test_every_refusal(tmp_path):
    good = np.arange(6, dtype=np.float32).reshape(2, 3)
    n = [0]

    def ark(blob, suffix=".ark"):
        n[0] += 1
        p = str(tmp_path / ("case%d%s" % (n[0], suffix)))
        open(p, "wb").write(blob)
        return p

    def expect(got, code, word):
        assert got[0] == code and word in got[1], got

    # PK_MI355_E_IO
    expect(refusal(str(tmp_path / "missing.ark")), E_IO, "cannot open")
    expect(refusal(str(tmp_path / "missing.scp")), E_IO, "cannot open")
    expect(refusal(str(tmp_path / "missing.bin"), True), E_IO, "cannot open")
    expect(refusal(ark(b"k " + binary(good)[:-1])), E_IO, "truncated")
    expect(refusal(ark(b"k " + binary(good)[:9])), E_IO, "truncated")
    expect(refusal(ark(b"k ")), E_IO, "truncated")
    expect(refusal(ark(b"k " + binary(good, size=8))), E_IO, "size byte")
    expect(refusal(ark(b"k " + binary(good, size=0))), E_IO, "size byte")
    expect(refusal(ark(b"k \0BFM " + struct.pack("<BiBi", 4, -2, 4, 3))), E_IO, "negative")
    expect(refusal(ark(b"k \0BFM " + struct.pack("<BiBi", 4, 1 << 30, 4, 1 << 30) + b"\0" * 64)), E_IO, "truncated")
    expect(refusal(ark(b"k  [\n 1 2 3\n 4 5 ]\n")), E_IO, "ragged")
    expect(refusal(ark(b"k  [\n 1 2 3\n 4 5 6\n")), E_IO, "truncated")
    expect(refusal(ark(b"k  [\n 1 2 x3 ]\n")), E_IO, "number")
    expect(refusal(ark(b"k \0XFM ")), E_IO, "garbage")
    expect(refusal(ark(b"k \0BQ!? ")), E_IO, "token")
    expect(refusal(ark(b"k \0BZZ " + b"\0" * 16)), E_IO, "token")
    expect(refusal(ark(b"k hello\n")), E_IO, "garbage")
    expect(refusal(ark(b"a " + binary(good) + b"\0\0\0\0 ")), E_IO, "key")
    expect(refusal(ark(b"a " + binary(good) + b"lonelykey")), E_IO, "key")
    expect(refusal(ark(b"justakey\n", ".scp")), E_IO, "expected")
    obj = ark(binary(good), ".mat")
    expect(refusal(ark(("a %s\nb %s:100000\n" % (obj, obj)).encode(), ".scp")), E_IO, "line 2")
    # PK_MI355_E_INVALID: well-formed, not taken
    for token in (b"CM ", b"CM2 ", b"CM3 "):
        got = refusal(ark(b"k \0B" + token + b"\0" * 40))
        expect(got, E_INVALID, "compressed")
        assert "uncompressed" in got[1] and token.decode().strip() in got[1]
    for token in (b"FV ", b"DV "):
        expect(refusal(ark(b"k \0B" + token + struct.pack("<Bi", 4, 3) + b"\0" * 24)), E_INVALID, "vector")
    got = refusal(ark(("a %s\nb %s[0:1]\n" % (obj, obj)).encode(), ".scp"))
    expect(got, E_INVALID, "range")
    assert "line 2" in got[1]
    got = refusal(ark(("a %s\nb %s\nc gunzip -c x.gz |\n" % (obj, obj)).encode(), ".scp"))
    expect(got, E_INVALID, "pipe")
    assert "line 3" in got[1]
    expect(refusal(ark(b"a -\n", ".scp")), E_INVALID, "standard input")
    expect(refusal("ark:-"), E_INVALID, "standard input")
    expect(refusal("ark:gunzip -c feats.ark.gz |"), E_INVALID, "pipe")
    expect(refusal("-", True), E_INVALID, "standard input")
    # a reader that met an error repeats it
    r = pk.ArkReader(ark(b"a " + binary(good) + b"b " + binary(good)[:12]))
    assert next(r)[0] == "a"
    for _ in range(2):
        with pytest.raises(pk.PkCodeError) as e:
            next(r)
        assert e.value.code == E_IO


# ---------------------------------------------------------------- the stand-alone program

@pytest.mark.parametrize("flavour", [
    "plain",
    pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                       reason="a GPU is present: sanitizer builds run on CPU machines only")),
])
def test_reader_stand_alone(flavour, tmp_path):
    binary_path = os.path.join(REPO, "tests", "cpp", "ark_test_%s.bin" % flavour)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1"] + (SANITIZE if flavour == "sanitized" else []) +
                          [SRC, os.path.join(CSRC, "pk_ark.cc"), os.path.join(CSRC, "pk_files.cc"), "-o", binary_path])
    items = entries()
    ark = str(tmp_path / "feats.ark")
    offsets = write_archive(ark, items)
    scp = str(tmp_path / "feats.scp")
    with open(scp, "w") as f:
        f.write("".join("%s %s:%d\n" % (k, ark, offsets[k]) for k, _, _ in items))
    rng = np.random.default_rng(3)
    three_items = [("first", rng.standard_normal((3, 5)).astype(np.float32), "float"), ("second", rng.standard_normal((2, 4)), "text"),
                   ("third", rng.standard_normal((4, 3)), "double")]
    three = str(tmp_path / "three.ark")
    write_archive(three, three_items)
    assert os.path.getsize(three) < 600
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    run = subprocess.run([binary_path, str(scratch), three, ark, "scp:" + scp, three], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-4000:]
    assert run.stderr == ""                                  # a sanitizer reports there
    out = run.stdout.splitlines()
    assert out[-1] == "ark_test ok"

    def lines_of(its):
        got = []
        for k, m, how in its:
            w = as_float32(m, how)
            if how == "text" and m.shape[0] == 0:
                w = np.zeros((0, 0), np.float32)
            got.append("entry %s %d %d %s" % (k, w.shape[0], w.shape[1], fnv(w.tobytes())))
        return got

    # (the text entry with NaN is compared from Python above; its hash depends on the NaN's bits, which strtod chooses)
    want = lines_of(items) + ["end %s 0" % ark] + lines_of(items) + ["end scp:%s 0" % scp] + lines_of(three_items) + ["end %s 0" % three]
    skip = {i for i, line in enumerate(want) if line.startswith("entry " + "k" * 200)}
    got = out[:len(want)]
    assert [g for i, g in enumerate(got) if i not in skip] == [w for i, w in enumerate(want) if i not in skip]
    for i in skip:
        assert got[i].rsplit(" ", 1)[0] == want[i].rsplit(" ", 1)[0]
    m = [re.fullmatch(r"sweep prefixes (\d+) clean (\d+) io (\d+)", line) for line in out]
    (m,) = [x for x in m if x]
    size = os.path.getsize(three)
    assert int(m.group(1)) == size + 1 and int(m.group(2)) + int(m.group(3)) == size + 1
    assert int(m.group(2)) >= 4 and int(m.group(3)) > size // 2          # the empty file and the three entry ends read clean
    for name in ("rows -1", "cols -1", "rows 2^31-1", "cols 2^31-1", "2^30 x 2^30", "size byte 0 (rows)", "size byte 8 (rows)",
                 "size byte 0 (cols)", "size byte 8 (cols)", "scp offset past the end", "DM 2^31-1 x 2^31-1", "DM count x 8 wraps",
                 "DM 2^30 x 2^30"):
        assert "field %s: -3" % name in out, name
    assert "field healthy 2 x 3: 0" in out and "field DM healthy 2 x 3: 0" in out
