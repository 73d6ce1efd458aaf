"""Host-only: the any-rate WAV reader (pk_mi355_wave_read) and the resampler's table builder in a process of their own
(tests/cpp/wave_test.cc: no HIP, no library, no Python), built plain and with ASan + UBSan.  The test writes its own
files -- 1 / 2 / 8 channels, 8 / 16 / 32 bits, three rates -- and the program's sample hashes must be those of the
test's own de-interleaving; its sweep over every header field and every truncation must end in error codes only.
Through the library: pk.read_wave against the same files, and pk_mi355_16kpcm_read keeps its refusals.  No GPU needed."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "pocketkaldi_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "wave_test.cc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FMT = {8: ("b", np.int8), 16: ("<h", np.int16), 32: ("<i", np.int32)}
CASES = [(2, 16, 44100), (1, 16, 16000), (1, 8, 8000), (8, 32, 96000), (2, 8, 22050), (8, 16, 48000), (1, 32, 11025)]


def write_wave(path, samples, bits, rate):
    """samples: integer array [frames][channels] -> a 44-byte-header PCM file."""
    frames, channels = samples.shape
    payload = samples.astype(FMT[bits][1]).astype(np.dtype(FMT[bits][1]).newbyteorder("<")).tobytes()
    align = channels * bits // 8
    header = (b"RIFF" + struct.pack("<i", 36 + len(payload)) + b"WAVEfmt " +
              struct.pack("<ihhiihh", 16, 1, channels, rate, rate * align, align, bits) + b"data" + struct.pack("<i", len(payload)))
    with open(path, "wb") as f:
        f.write(header + payload)


def fnv(data):
    h = 14695981039346656037
    for byte in data:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("waves")
    rng = np.random.default_rng(5)
    out = []
    for channels, bits, rate in CASES:
        lim = 2 ** (bits - 1)
        samples = rng.integers(-lim, lim, (41 + channels, channels), dtype=np.int64)
        samples[0, 0], samples[1, 0] = -lim, lim - 1                   # both ends of the range
        path = str(d / ("c%d_b%d_r%d.wav" % (channels, bits, rate)))
        write_wave(path, samples, bits, rate)
        out.append((path, samples, bits, rate))
    return d, out


@pytest.mark.parametrize("flavour", [
    "plain",
    pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                       reason="a GPU is present: sanitizer builds run on CPU machines only")),
])
def test_wave_reader_and_table_builder_stand_alone(flavour, files, tmp_path):
    _, waves = files
    binary = os.path.join(REPO, "tests", "cpp", "wave_test_%s.bin" % flavour)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off"] + (SANITIZE if flavour == "sanitized" else []) +
                          [SRC, os.path.join(CSRC, "pk_files.cc"), os.path.join(CSRC, "pk_tables.cc"), "-o", binary])
    run = subprocess.run([binary, str(tmp_path)] + [w[0] for w in waves], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-4000:]
    assert run.stderr == ""                               # a sanitizer reports there
    out = run.stdout.splitlines()
    assert out[-1] == "wave_test ok"

    # ---- every file, every channel
    want = []
    for path, samples, bits, rate in waves:
        for c in range(samples.shape[1]):
            data = samples[:, c].astype(np.float32).tobytes()
            want.append("wave %s ch %d rate %d channels %d n %d fnv %016x" % (path, c, rate, samples.shape[1], samples.shape[0], fnv(data)))
    assert out[:len(want)] == want

    # ---- the sweep: nine header fields x eight values x two channels, and every length 0 .. len + 1
    (sweep,) = [l for l in out if l.startswith("sweep ")]
    m = re.fullmatch(r"sweep fields (\d+) cases (\d+) codes((?: -?\d+)+)", sweep)
    size = os.path.getsize(waves[0][0])
    assert int(m.group(1)) == 9 and int(m.group(2)) == 9 * 8 * 2 + size + 2
    # the good file and malformed ones (the header is checked before the channel: a single changed field never gets that far)
    assert {int(c) for c in m.group(3).split()} == {0, -3}

    # ---- the named cases
    for line in ("case ragged_payload: 0 n 10", "case truncated_payload: -3", "case channels_0: -3", "case channels_9: -3",
                 "case mono_byte_rate: -3", "case mono_block_align: -3", "case mono16k_8: same 1", "case mono16k_16: same 1",
                 "case mono16k_32: same 1", "case strict_stereo: -3 0", "case strict_rate: -3 0", "case null_arguments: -1 -1"):
        assert line in out, line

    # ---- the table builder over every rate: the seven everyday rates are among the supported ones
    (tables,) = [l for l in out if l.startswith("tables ")]
    m = re.fullmatch(r"tables supported (\d+) largest (\d+) at (\d+)", tables)
    assert int(m.group(1)) >= 7 and int(m.group(2)) <= 16384


def test_read_wave_through_the_library(files, tmp_path):
    d, waves = files
    for path, samples, bits, rate in waves:
        for c in range(samples.shape[1]):
            got, got_rate = pk.read_wave(path, channel=c)
            assert got_rate == rate and got.dtype == np.float32
            assert np.array_equal(got, samples[:, c].astype(np.float32))
        for bad in (-1, samples.shape[1]):
            with pytest.raises(pk.PkError) as e:
                pk.read_wave(path, channel=bad)
            assert e.value.code == -1 and "channel" in str(e.value)
        mono16k = samples.shape[1] == 1 and rate == 16000
        if mono16k:
            assert np.array_equal(pk.read_wav(path), pk.read_wave(path)[0])
        else:                                             # pk_16kpcm_read keeps the reference's refusals, in its words
            with pytest.raises(pk.PkError, match="num_channels == 1|sample_rate == 16000"):
                pk.read_wav(path)
    with pytest.raises(pk.PkError) as e:
        pk.read_wave(str(tmp_path / "absent.wav"))
    assert e.value.code == -3
    # the reference's own file through both readers
    hello = os.path.join(REPO, "tests", "golden", "en-us-hello.wav")
    w, rate = pk.read_wave(hello)
    assert rate == 16000 and np.array_equal(w, pk.read_wav(hello))
