"""The online recognizer (pk_mi355_online_recognizer_*, pk.OnlineRecognizer): pk_load + a live pk_process.  Waves fed
in chunks, two slots at once, must end in what pk.Recognizer.process gives on the whole waves -- text, words, weight
bits, ok, log-likelihood-per-frame bits, segments with their acoustic cost, the decoder's alignment -- with partial
text on the way; empty and short waves and a reused slot by the same rules; the command-line tool with --online and
the C++ example print the offline tool's bytes."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import pocketkaldi_amd as pk

from refmodel_text import DIR
from test_gpu_align import TRACE, bits
from test_gpu_decoder import G
from test_symtab_host import parse_symtab

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(DIR, "recognizer.conf")
HELLO, CAT = (os.path.join(G, w) for w in ("en-us-hello.wav", "en-us-cat.wav"))
NAMES = parse_symtab(os.path.join(DIR, "wordloop_words.bin"))
E_STATE = -4


def build_example():
    """As tests/test_gpu_recognizer.py builds recognize_example."""
    pk.lib()
    libdir = os.path.dirname(pk.lib_path())
    out = os.path.join(REPO, "tests", "cpp", "online_recognize_example.bin")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp", "online_recognize_example.cc"), "-o", out,
                           "-L", libdir, "-l:libpk_mi355.so", "-Wl,-rpath," + libdir])
    return out


def test_online_recognize_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build_example(), "--link-only"], text=True)


def comparable(r):
    return (r.text, r.words, bits(r.weight), r.ok, bits(r.loglikelihood_per_frame),
            [(s.word, s.start_frame, s.num_frames, bits(s.graph_cost), bits(s.acoustic_cost)) for s in r.segments])


@pytest.fixture(scope="module")
def pair():
    """The batch recognizer's results on the two waves (computed once), and an online recognizer of two slots."""
    waves = [pk.read_wav(HELLO), pk.read_wav(CAT)]
    rec = pk.Recognizer(CONF, max_utts=2, max_total_samples=sum(len(w) for w in waves), trace_capacity=TRACE)
    rec.am.set_softmax("reference")
    want = rec.process(waves)
    alignments = [[a.tobytes() for a in rec.decoder.alignment(u)] for u in range(2)]
    empty = rec.process([np.zeros(0, np.float32), waves[0][:300]])
    rec.close()
    online = pk.OnlineRecognizer(CONF, max_streams=2, max_step_samples=2 * 4001, trace_capacity=TRACE)
    online.am.set_softmax("reference")
    yield waves, want, alignments, empty, online
    online.destroy()


def stream(online, waves, plans, slots):
    """Wave u into slots[u], its chunk sizes cycling through plans[u]; closed with its last chunk.
    -> ({u: Result}, the partial texts seen while live)"""
    pos, turn, live, out, partials = [0] * len(waves), [0] * len(waves), set(range(len(waves))), {}, []
    for s in slots:
        online.open(s)
        assert not online.finished(s) and online.partial(s) == ""
    while live:
        closing = []
        for u in sorted(live):
            n = plans[u][turn[u] % len(plans[u])]
            online.push(slots[u], waves[u][pos[u]:pos[u] + n])
            pos[u] += n
            turn[u] += 1
            if pos[u] >= len(waves[u]):
                online.close(slots[u])
                closing.append(u)
        online.step()
        for u in sorted(live):
            if u in closing:
                assert online.finished(slots[u])
                out[u] = online.result(slots[u])
                live.discard(u)
            else:
                assert not online.finished(slots[u])
                with pytest.raises(pk.PkCodeError) as e:
                    online.result(slots[u])
                assert e.value.code == E_STATE
                partials.append(online.partial(slots[u]))
    return out, partials


@pytest.mark.gpu
def test_chunked_streaming_equals_the_batch_recognizer(pair):
    waves, want, alignments, _, online = pair
    assert [online.symbols[i] for i in range(len(online.symbols))] == NAMES
    out, partials = stream(online, waves, [[1600], [37, 4001, 160]], [0, 1])
    for u in range(2):
        assert comparable(out[u]) == comparable(want[u]), u
        assert out[u].ok == 1 and out[u].text and not out[u].text.endswith(" ")
        assert all(not math.isnan(s.acoustic_cost) for s in out[u].segments)
        assert [a.tobytes() for a in online.decoder.alignment(u)] == alignments[u], u
        assert online.decoder.num_frames(u) == pk.num_frames(len(waves[u]))
    spoken = [p for p in partials if p]
    assert len(spoken) >= 4 and all(w in NAMES for p in spoken for w in p.split(" "))


@pytest.mark.gpu
def test_empty_and_short_waves_and_slot_reuse(pair):
    waves, want, _, empty, online = pair
    out, _ = stream(online, [np.zeros(0, np.float32), waves[0][:300]], [[1600], [100]], [0, 1])
    for u in range(2):
        r = out[u]
        assert comparable(r) == comparable(empty[u])
        assert r.text == "" and r.loglikelihood_per_frame == 0.0 and r.words == [] and r.segments == []
        assert math.copysign(1.0, r.loglikelihood_per_frame) == 1.0
    for u in (0, 1):                                   # slot 1 for hello, then again for cat
        out, _ = stream(online, [waves[u]], [[1600, 801]], [1])
        assert comparable(out[0]) == comparable(want[u]), u


@pytest.mark.gpu
@pytest.mark.parametrize("wav", [HELLO, CAT])
def test_cli_online_and_cpp_example_print_the_offline_bytes(wav, capsys):
    from pocketkaldi_amd import recognize
    offline = {}
    for name, extra in (("plain", []), ("ctm", ["--ctm"])):      # the yardstick, in this process (its own process:
        assert recognize.main([CONF, wav] + extra) == 0           # tests/test_gpu_recognizer.py)
        offline[name] = capsys.readouterr().out
    assert offline["plain"].count("\t") == 2 and offline["ctm"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    tool = [sys.executable, "-m", "pocketkaldi_amd.recognize", CONF, wav, "--online"]
    plain = subprocess.run(tool, capture_output=True, text=True, env=env)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    assert plain.stdout == offline["plain"]
    ctm = subprocess.run(tool + ["--ctm", "--partials", "--chunk-ms", "130"], capture_output=True, text=True, env=env)
    assert ctm.returncode == 0, ctm.stdout + ctm.stderr
    assert ctm.stdout == offline["ctm"]
    shown = [l.split("\t") for l in ctm.stderr.splitlines() if l.startswith(wav + "\t")]
    assert shown and all(len(l) == 3 and float(l[1]) > 0 for l in shown)
    assert shown[-1][2] == offline["plain"].rstrip("\n").split("\t")[1]              # the last partial is the sentence
    example = subprocess.run([build_example(), CONF, wav], capture_output=True, text=True)
    assert example.returncode == 0, example.stdout + example.stderr
    assert example.stdout == offline["plain"]
