"""tests/cpp/online_commit_example.cc: tests/cpp/stream_example.cc with pocketkaldi::OnlineDecoder::SetCommit on.  It
checks OnlineDecoder::Committed against every partial hypothesis itself; what it prints -- every partial and the final
lines -- must be what the mode-off example prints."""
import os
import subprocess

import pytest

from refmodel_text import DIR
from test_cpp_stream import G, build


def test_online_commit_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("online_commit_example"), "--link-only"], text=True)


@pytest.mark.gpu
@pytest.mark.parametrize("wav", ["en-us-hello.wav", "en-us-cat.wav"])
def test_online_commit_example_prints_the_mode_off_lines(wav):
    args = [os.path.join(DIR, "refmodel.conf"), os.path.join(G, wav), os.path.join(DIR, "wordloop.fst")]
    got = subprocess.run([build("online_commit_example")] + args, capture_output=True, text=True)
    assert got.returncode == 0 and "online_commit_example ok" in got.stdout, got.stdout + got.stderr
    want = subprocess.run([build("stream_example")] + args, capture_output=True, text=True)
    assert want.returncode == 0 and "stream_example ok" in want.stdout, want.stdout + want.stderr
    lines = got.stdout.splitlines()
    assert [l.split(" stable ")[0] for l in lines[:-1]] == want.stdout.splitlines()[:-1]
    stable = [int(l.split(" stable ")[1].split()[0]) for l in lines if l.startswith("partial ")]
    assert len(stable) >= 3 and stable == sorted(stable)
