"""Endpointing at the online recognizer (pk_mi355_online_recognizer_set_endpointing / _utterance*,
pk.OnlineRecognizer.set_endpointing / utterances: csrc/capi_online_recognizer.hip): the golden model on the two golden
waves joined around half a second of silence.  The stream is cut where the host model (tests/endpoint_model.py) cuts
it, given the frames each step decoded; every utterance is Decoder.decode on the batch scorer's rows of its frames; the
pieces add up to the wave; partial and stable restart with every piece; two slots do not disturb each other; a silence
set under which nothing fires leaves one utterance, the batch recognizer's; the command-line tool prints the pieces."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pocketkaldi_amd as pk

import endpoint_cases as EC
import endpoint_model as EM
from commit_cases import with_ids
from refmodel_text import DIR, load_text_model
from test_gpu_align import TRACE
from test_gpu_decoder import read_fst
from test_gpu_online_recognizer import CAT, CONF, HELLO, REPO, comparable

pytestmark = pytest.mark.gpu

# How the inputs were chosen, on the CPU: the oracle's log-likelihoods of the joined wave (oracle.Nnet.am_compute over
# its fbank and CMVN, 149 frames) were decoded by the host model over wordloop.fst.  The best path emits pdfs 15, 17 and
# then stays on pdf 10 for as long as the audio lasts -- and does so again from wherever it is restarted -- while the
# best final token costs 1.65 to 2.3 more than the best token.  With pdf 10 declared silence, "speech, then 25 frames
# of silence, at a relative cost of at most 2.0" fires about every 28 to 30 frames wherever the cost allows it, and
# where it does not the second rule ends the utterance at 60 frames: with steps of 7 or 10 frames the model cuts the
# 149 frames into 4 or 5 utterances, and both rules fire.
SILENCE = [10]
RULES = [pk.EndpointRule(True, 0.25, 2.0, 0.0), pk.EndpointRule(False, 0.0, np.inf, 0.60)]
RULES_FRAMES = [(1, 25, 2.0, 0), (0, 0, np.inf, 60)]
GAP = 8000
STEP = 2 * 4001


@pytest.fixture(scope="module")
def setup():
    """The joined wave, the batch recognizer's result and rows on it (computed once), piece(a, b) = the batch decoder on
    rows [a, b) as a Result, the model's graph, and an online recognizer of two slots with endpointing on."""
    wave = np.concatenate([pk.read_wav(HELLO), np.zeros(GAP, np.float32), pk.read_wav(CAT)]).astype(np.float32)
    rec = pk.Recognizer(CONF, max_utts=1, max_total_samples=len(wave), trace_capacity=TRACE)
    rec.am.set_softmax("reference")
    (whole,) = rec.process([wave])
    rows = rec.batch.fetch(0).log_prob()
    assert rows.shape[0] == pk.num_frames(len(wave))
    cache = {}

    def piece(a, b):
        if (a, b) not in cache:
            rec.decoder.decode([rows[a:b]])
            words, weight, ok = rec.decoder.result(0)
            spoken = bool(ok and words)
            cache[a, b] = pk.Result(" ".join(rec.symbols[w] for w in words) if spoken else "", words, weight, ok,
                                    float(np.float32(weight) / np.float32(b - a)) if spoken else 0.0, rec.decoder.word_segments(0))
        return cache[a, b]
    start, final, arcs = read_fst(os.path.join(DIR, "wordloop.fst"))
    tid2pdf = load_text_model()[4]
    fst = with_ids(dict(start=start, final=np.asarray(final, np.float32), arcs=arcs))
    online = pk.OnlineRecognizer(CONF, max_streams=2, max_step_samples=STEP, trace_capacity=TRACE)
    online.am.set_softmax("reference")
    online.set_endpointing(SILENCE, RULES)
    yield wave, whole, rows, piece, (fst, lambda t: int(tid2pdf[t])), online
    online.destroy()
    rec.close()


def stream(online, wave, plans, slots):
    """The wave into every one of `slots`, slot slots[u]'s chunk sizes cycling through plans[u], closed with the last
    chunk.  -> per u: the frames each step decoded, and (partial, stable, utterances so far) after each step."""
    n = len(slots)
    pos, turn, live = [0] * n, [0] * n, set(range(n))
    counts, seen = [[] for _ in range(n)], [[] for _ in range(n)]
    for s in slots:
        online.open(s)
        assert online.utterances(s) == []
    while live:
        closing = []
        for u in sorted(live):
            c = plans[u][turn[u] % len(plans[u])]
            online.push(slots[u], wave[pos[u]:pos[u] + c])
            pos[u] += c
            turn[u] += 1
            if pos[u] >= len(wave):
                online.close(slots[u])
                closing.append(u)
        online.step()
        for u in sorted(live):
            pieces = online.utterances(slots[u])
            decoded = sum(p.num_frames for p in pieces) + (0 if u in closing else online.decoder.num_frames(slots[u]))
            counts[u].append(decoded - sum(counts[u]))
            seen[u].append((online.partial(slots[u]), online.stable(slots[u]), len(pieces)))
            if u in closing:
                assert online.finished(slots[u])
                live.discard(u)
    return counts, seen


def check_pieces(online, slot, wave, rows, piece, model, counts):
    fst, pdf_of = model
    pieces = online.utterances(slot)
    want = EM.utterances(fst, rows, pdf_of, lambda f, t, c: EC.eval_frames(RULES_FRAMES, f, t, c), counts, silence=SILENCE)
    assert [(p.first_frame, p.num_frames, p.rule) for p in pieces] == want
    assert len(pieces) >= 3 and pieces[-1].rule == 0 and all(p.rule for p in pieces[:-1])
    assert sum(p.num_frames for p in pieces) == pk.num_frames(len(wave))
    for p in pieces:
        assert comparable(p.result) == comparable(piece(p.first_frame, p.first_frame + p.num_frames)), p
    assert comparable(online.result(slot)) == comparable(pieces[-1].result)        # hyp and per-frame: the last piece's
    return pieces


def test_the_stream_is_cut_where_the_model_cuts_it(setup):
    wave, whole, rows, piece, model, online = setup
    counts, seen = stream(online, wave, [[1600]], [0])
    pieces = check_pieces(online, 0, wave, rows, piece, model, counts[0])
    assert {p.rule for p in pieces} == {0, 1, 2} and any(p.result.text for p in pieces)
    # partial and stable are the current piece's: after a step that cut, they are empty
    cuts = [i for i in range(1, len(seen[0])) if seen[0][i][2] > seen[0][i - 1][2]]
    assert len(cuts) >= 3 and all(seen[0][i][:2] == ("", "") for i in cuts[:-1])
    assert any(text for text, _, _ in seen[0])


def test_two_slots_with_different_chunk_plans(setup):
    wave, whole, rows, piece, model, online = setup
    online.decoder.set_commit(True)
    try:
        counts, seen = stream(online, wave, [[1120], [37, 4001, 160, 2400]], [1, 0])
        a = check_pieces(online, 1, wave, rows, piece, model, counts[0])
        b = check_pieces(online, 0, wave, rows, piece, model, counts[1])
        assert counts[0] != counts[1]
        assert [(p.first_frame, p.num_frames) for p in a] != [(p.first_frame, p.num_frames) for p in b]
        cuts = [i for i in range(1, len(seen[0])) if seen[0][i][2] > seen[0][i - 1][2]]
        assert all(seen[0][i][:2] == ("", "") for i in cuts[:-1])      # stable restarts too, with commit on
    finally:
        online.decoder.set_commit(False)


def test_nothing_fires_under_a_silence_set_that_never_occurs(setup):
    wave, whole, rows, piece, model, online = setup
    online.set_endpointing([], [RULES[0]])               # no silence at all: the one rule left needs 25 frames of it
    try:
        stream(online, wave, [[1600]], [0])
        (only,) = online.utterances(0)
        assert (only.first_frame, only.num_frames, only.rule) == (0, pk.num_frames(len(wave)), 0)
        assert comparable(only.result) == comparable(whole) == comparable(online.result(0))
    finally:
        online.set_endpointing(SILENCE, RULES)


def test_the_command_line_tool_prints_the_pieces(setup, tmp_path):
    wave, whole, rows, piece, model, online = setup
    counts, _ = stream(online, wave, [[1600]], [0])
    pieces = online.utterances(0)
    path = str(tmp_path / "joined.wav")
    write_wav(path, wave)
    args = [sys.executable, "-m", "pocketkaldi_amd.recognize", CONF, path, "--online", "--reference-softmax",
            "--endpoint-silence", "10", "--endpoint-rule", "1,0.25,2.0,0", "--endpoint-rule", "0,0,inf,0.6"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    got = subprocess.run(args, capture_output=True, text=True, cwd=REPO, env=env)
    assert got.returncode == 0, got.stdout + got.stderr
    assert got.stdout == "".join("%s[%.2f-%.2f]\t%s\t%f\n" % (path, p.first_frame * 0.01, (p.first_frame + p.num_frames) * 0.01,
                                                             p.result.text, p.result.loglikelihood_per_frame) for p in pieces)
    ctm = subprocess.run(args + ["--ctm"], capture_output=True, text=True, cwd=REPO, env=env)
    assert ctm.returncode == 0, ctm.stdout + ctm.stderr
    assert ctm.stdout == "".join("%s 1 %.2f %.2f %s\n" % (path, (p.first_frame + s.start_frame) * 0.01, s.num_frames * 0.01,
                                                         online.symbols[s.word])
                                 for p in pieces for s in p.result.segments if s.word != 0)
    assert ctm.stdout


def write_wav(path, wave):
    """16 kHz mono 16-bit PCM, as the golden waves are."""
    import wave as W
    with W.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.asarray(wave, np.int16).tobytes())
