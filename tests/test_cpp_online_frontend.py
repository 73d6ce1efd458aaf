"""tests/cpp/online_frontend_example.cc: a wave as live audio through pocketkaldi::OnlineRecognizer::Load(model file,
FrontendSpec::Fbank(80), ...) (include/pocketkaldi_amd.hpp) -- an 80-bin Povey-window fbank in front
of an 80-dim model written into tmp_path.  Its line is python -m pocketkaldi_amd.recognize --frontend's, with and without
--online."""
import os
import shutil
import subprocess

import pytest

import pocketkaldi_amd as pk

import refmodel_files as RF
from test_cpp_stream import build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_online_frontend_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("online_frontend_example"), "--link-only"], text=True)


@pytest.mark.gpu
def test_online_frontend_example_prints_the_command_lines_bytes(tmp_path, capsys):
    from pocketkaldi_amd import recognize
    from refmodel_text import load_text_model
    from test_gpu_frontend_recognizer import CAT, DIR, HELLO, L, R, STATS, model_layers
    layers, prior = model_layers()
    conf = RF.write_model(tmp_path, layers, prior, L, R, tid2pdf=load_text_model()[4], cmvn_stats=STATS)
    for name in ("wordloop.fst", "wordloop_words.bin"):
        shutil.copy(os.path.join(DIR, name), str(tmp_path / name))
    with open(conf, "a") as f:
        f.write("fst = wordloop.fst\nsymbol_table = wordloop_words.bin\n")
    for wav in (HELLO, CAT):
        got = subprocess.run([build("online_frontend_example"), conf, wav], capture_output=True, text=True)
        assert got.returncode == 0, got.stdout + got.stderr
        for extra in ([], ["--online"]):
            assert recognize.main([conf, wav, "--frontend", "num_mel_bins=80,window=povey"] + extra) == 0
            want = capsys.readouterr().out
            assert want.count("\t") == 2 and want.split("\t")[1]          # a sentence, not an empty hypothesis
            assert got.stdout == want, extra
        assert any(line.startswith(wav + "\t") for line in got.stderr.splitlines())     # partials were shown
