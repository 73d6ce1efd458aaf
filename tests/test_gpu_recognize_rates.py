"""Recognizer.process(waves, rates) and the command line on files that are not 16 kHz mono.  The yardstick is the
recognizer on the same audio converted by the numpy model over the library's table (tests/resample_model.py): every
field of every Result, and the lines the command line prints (a WAV file holds integers and the converted samples are
not, so the expected line is formatted here from that Result, not read back from a converted file)."""
import os
import struct

import numpy as np
import pytest

import pocketkaldi_amd as pk

import resample_model as M
from refmodel_text import DIR
from test_gpu_online_resample import comparable
from test_gpu_resample import lib_table

pytestmark = pytest.mark.gpu

CONF = os.path.join(DIR, "recognizer.conf")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def stretched(wave, rate):
    """A 16 kHz wave brought to `rate` by linear interpolation, integer sample values (test audio, not a yardstick)."""
    n = len(wave) * rate // 16000
    return np.round(np.interp(np.arange(n) * (16000.0 / rate), np.arange(len(wave)), wave)).astype(np.float32)


@pytest.fixture(scope="module")
def audio():
    hello = pk.read_wav(os.path.join(GOLDEN, "en-us-hello.wav"))
    cat = pk.read_wav(os.path.join(GOLDEN, "en-us-cat.wav"))[:8000]
    rates = [48000, 16000, 44100, 8000]
    waves = [stretched(hello, 48000), cat, stretched(cat, 44100), stretched(hello, 8000)]
    converted = [w if r == 16000 else M.resample(lib_table(r), w) for w, r in zip(waves, rates)]
    return waves, rates, converted


def test_process_with_rates_equals_process_of_the_converted_waves(audio):
    waves, rates, converted = audio
    total = sum(len(w) for w in converted)
    rec = pk.Recognizer(CONF, max_utts=4, max_total_samples=total)
    want = rec.process(converted)
    got = rec.process(waves, rates=rates)
    assert [comparable(r) for r in got] == [comparable(r) for r in want]
    assert sum(1 for r in want if r.text) >= 3
    # a recognizer that holds two waves per call and not all of the samples splits the list by 16 kHz sizes
    small = pk.Recognizer(CONF, max_utts=2, max_total_samples=max(len(w) for w in converted) + 100)
    assert [comparable(r) for r in small.process(waves, rates=rates)] == [comparable(r) for r in want]
    with pytest.raises(pk.PkError) as e:
        small.process(waves, rates=[16001] * 4)
    assert e.value.code == -1 and "16001" in str(e.value)
    small.close()
    rec.close()


def test_command_line_on_a_48_khz_stereo_file(audio, tmp_path, capsys):
    from pocketkaldi_amd import recognize
    waves, rates, converted = audio
    speech = waves[0].astype(np.int16)
    other = np.random.default_rng(3).integers(-3000, 3000, len(speech)).astype(np.int16)
    payload = np.stack([other, speech], axis=1).astype("<i2").tobytes()
    path = str(tmp_path / "stereo48k.wav")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<i", 36 + len(payload)) + b"WAVEfmt " +
                struct.pack("<ihhiihh", 16, 1, 2, 48000, 48000 * 4, 4, 16) + b"data" + struct.pack("<i", len(payload)))
        f.write(payload)
    got_wave, got_rate = pk.read_wave(path, channel=1)
    assert got_rate == 48000 and np.array_equal(got_wave, waves[0])

    rec = pk.Recognizer(CONF, max_utts=1, max_total_samples=len(converted[0]))
    (want,) = rec.process([converted[0]])
    rec.close()
    assert want.text
    line = "%s\t%s\t%f\n" % (path, want.text, want.loglikelihood_per_frame)
    names = pk.SymbolTable(os.path.join(DIR, "wordloop_words.bin"))
    ctm = "".join("%s 1 %.2f %.2f %s\n" % (path, s.start_frame * 0.01, s.num_frames * 0.01, names[s.word])
                  for s in want.segments if s.word != 0)
    for extra in ([], ["--online"], ["--online", "--chunk-ms", "70"]):
        assert recognize.main([CONF, path, "--channel", "1"] + extra) == 0
        assert capsys.readouterr().out == line, extra
        assert recognize.main([CONF, path, "--channel", "1", "--ctm"] + extra) == 0
        assert capsys.readouterr().out == ctm, extra
    # the other channel is other audio; a channel the file does not have is refused in the program's words
    assert recognize.main([CONF, path]) == 0
    assert capsys.readouterr().out != line
    assert recognize.main([CONF, path, "--channel", "2"]) == 1
    assert capsys.readouterr().out.startswith("pocketkaldi: channel 2")
    assert recognize.main([CONF, path, "--channel"]) == 1
    capsys.readouterr()
