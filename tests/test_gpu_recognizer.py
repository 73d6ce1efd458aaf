"""The recognizer (pk_mi355_recognizer_*, pk.Recognizer): pk_load + pk_process -- model file and waves to a sentence
and a log-likelihood per frame.  Words and weight bits against the reference's own decoder
(oracle/_ref/libpkref_decoder.so) on the reference's own log-likelihoods (tests/golden/ref_am_path.npz); the text
against an independent parse of the symbol table; the command-line tool against the C++ example; the online decoder's
word segments against the batch decoder's."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import pocketkaldi_amd as pk

from refmodel_files import load_ref_am_path
from refmodel_text import DIR
from test_gpu_align import TRACE, bits, check_alignment, got_segments
from test_gpu_decode import flat_arcs, ref_decode
from test_gpu_decoder import DECLIB, G
from test_symtab_host import parse_symtab

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(DIR, "recognizer.conf")
FST = os.path.join(DIR, "wordloop.fst")
HELLO, CAT = (os.path.join(G, w) for w in ("en-us-hello.wav", "en-us-cat.wav"))
NAMES = parse_symtab(os.path.join(DIR, "wordloop_words.bin"))


def build_example():
    """As tests/test_cpp_decode.py builds gpu_decode_example."""
    pk.lib()
    libdir = os.path.dirname(pk.lib_path())
    out = os.path.join(REPO, "tests", "cpp", "recognize_example.bin")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp", "recognize_example.cc"), "-o", out,
                           "-L", libdir, "-l:libpk_mi355.so", "-Wl,-rpath," + libdir])
    return out


def test_recognize_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build_example(), "--link-only"], text=True)


@pytest.fixture(scope="module")
def recognizer():
    waves = [pk.read_wav(HELLO), pk.read_wav(CAT)]
    rec = pk.Recognizer(CONF, max_utts=2, max_total_samples=sum(len(w) for w in waves), trace_capacity=TRACE)
    rec.am.set_softmax("reference")
    yield rec, waves
    rec.close()


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(DECLIB), reason="oracle/_ref/libpkref_decoder.so not built")
def test_hello_and_cat_against_the_reference(recognizer):
    rec, waves = recognizer
    z = load_ref_am_path()
    assert len(rec.symbols) == len(NAMES) and [rec.symbols[i] for i in range(len(NAMES))] == NAMES
    results = rec.process(waves)
    tid2pdf = np.fromfile(os.path.join(DIR, "refmodel_tid2pdf.bin"), "<i4", offset=12)
    arcs = flat_arcs(FST)
    for u, (r, ref_ll) in enumerate(zip(results, (z["ll_refmodel_hello"], z["ll_refmodel_cat"]))):
        ref_ll = np.ascontiguousarray(ref_ll, np.float32)
        words, weight, ok = ref_decode(FST, ref_ll, rec.am.handle)
        assert ok == r.ok == 1 and r.words == words and len(words) >= 1
        assert bits(r.weight) == bits(weight)
        assert r.text == " ".join(NAMES[w] for w in words) and not r.text.endswith(" ")
        T = ref_ll.shape[0]
        assert rec.batch.num_frames(u) == T
        assert bits(r.loglikelihood_per_frame) == bits(np.float32(weight) / np.float32(T))
        # the owned decoder ran with alignment on: the segments are the restatement's over the reference's rows
        assert check_alignment(rec.decoder, u, arcs, ref_ll, lambda t: int(tid2pdf[t])) == T
        assert [(s.word, s.start_frame, s.num_frames, bits(s.graph_cost), bits(s.acoustic_cost)) for s in r.segments] == \
            got_segments(rec.decoder, u)


@pytest.mark.gpu
def test_empty_and_short_waves_and_splitting(recognizer):
    rec, waves = recognizer
    hello = waves[0]
    empty = rec.process([np.zeros(0, np.float32), hello[:300]])
    for r in empty:
        assert r.text == "" and r.loglikelihood_per_frame == 0.0 and r.words == [] and r.segments == []
        assert math.copysign(1.0, r.loglikelihood_per_frame) == 1.0
    # five waves through a recognizer that holds two per call (and not all of their samples): three calls
    many = [waves[0], waves[1], hello[:300], waves[1][:6000], waves[0][1000:]]
    assert sum(len(w) for w in many) > rec.max_total_samples and len(many) > rec.max_utts
    split = rec.process(many)
    assert len(split) == len(many)
    for w, r in zip(many, split):
        (solo,) = rec.process([w])
        assert (r.text, r.words, bits(r.weight), r.ok, bits(r.loglikelihood_per_frame)) == \
            (solo.text, solo.words, bits(solo.weight), solo.ok, bits(solo.loglikelihood_per_frame))
        assert [tuple(s[:3]) + (bits(s[3]), bits(s[4])) for s in r.segments] == [tuple(s[:3]) + (bits(s[3]), bits(s[4])) for s in solo.segments]
    assert split[0].text and split[1].text and split[2].text == ""
    with pytest.raises(pk.PkError, match="samples"):          # a single wave that cannot fit is refused, nothing is cut
        rec.process([np.zeros(rec.max_total_samples + 1, np.float32)])


@pytest.mark.gpu
@pytest.mark.parametrize("wav", [HELLO, CAT])
def test_cli_and_cpp_example_print_the_same_line(wav):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cli = subprocess.run([sys.executable, "-m", "pocketkaldi_amd.recognize", CONF, wav], capture_output=True, text=True, env=env)
    assert cli.returncode == 0, cli.stdout + cli.stderr
    example = subprocess.run([build_example(), CONF, wav], capture_output=True, text=True)
    assert example.returncode == 0, example.stdout + example.stderr
    assert cli.stdout == example.stdout
    name, text, value = cli.stdout.rstrip("\n").split("\t")                 # main.cc:28: "%s\t%s\t%f\n"
    assert name == wav and len(text.split(" ")) >= 1 and all(w in NAMES for w in text.split(" "))
    assert value == "%f" % float(value) and float(value) != 0.0
    ctm = subprocess.run([sys.executable, "-m", "pocketkaldi_amd.recognize", CONF, wav, "--ctm"], capture_output=True, text=True, env=env)
    assert ctm.returncode == 0, ctm.stdout + ctm.stderr
    lines = [l.split(" ") for l in ctm.stdout.splitlines()]
    assert [l[4] for l in lines] == text.split(" ") and all(l[0] == wav and l[1] == "1" for l in lines)
    starts, durations = [float(l[2]) for l in lines], [float(l[3]) for l in lines]
    assert starts == sorted(starts) and all(d >= 0 for d in durations)
    assert abs(starts[-1] + durations[-1] - 0.01 * pk.num_frames(len(pk.read_wav(wav)))) < 1e-6     # the last word ends with the wave


@pytest.mark.gpu
def test_online_word_segments_equal_the_batch_decoders(recognizer):
    rec, waves = recognizer
    rec.process(waves)
    lls = [rec.batch.fetch(u).log_prob() for u in range(2)]
    want = [got_segments(rec.decoder, u) for u in range(2)]
    fst = pk.Fst(FST)
    online = pk.OnlineDecoder(fst, rec.am, 2, trace_capacity=TRACE)
    for u in range(2):
        online.open(u)
    step, live, pos, done = 9, 0, [0, 0], [False, False]
    while not all(done):
        chunks = {}
        for u, ll in enumerate(lls):
            if not done[u]:
                end = min(pos[u] + step, ll.shape[0])
                chunks[u] = (ll[pos[u]:end], end == ll.shape[0])
                pos[u], done[u] = end, end == ll.shape[0]
        online.advance_host(chunks)
        for u, (_, fin) in chunks.items():
            segs = online.word_segments(u)
            assert [s.word for s in segs if s.word] == online.partial(u)[0]                # while live: partial's words
            assert all(math.isnan(s.acoustic_cost) for s in segs)
            live += not fin
    assert live >= 4
    for u in range(2):
        assert online.result(u)[0] == rec.decoder.result(u)[0]
        final = online.word_segments(u)
        assert [(s.word, s.start_frame, s.num_frames, bits(s.graph_cost)) for s in final] == [w[:4] for w in want[u]]
        assert final and all(math.isnan(s.acoustic_cost) for s in final)
