"""The command line on feature files: Kaldi archives and script files next to .npy / .npz, and
--features with --online.  The features are the wave call's fbank (40-dim refmodel fixtures), so every form must print
what the wave files print: batch and online, under the archive's keys, with --ctm, --partials --commit and
--endpoint-silence.  The tool's main() runs in this process."""
import os
import struct

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import recognize

pytestmark = pytest.mark.gpu

ENDPOINT = ["--endpoint-silence", "10", "--endpoint-rule", "1,0.25,2.0,0", "--endpoint-rule", "0,0,inf,0.6"]


def binary_matrix(a):
    a = np.ascontiguousarray(a, "<f4")
    return b"\0BFM " + struct.pack("<BiBi", 4, a.shape[0], 4, a.shape[1]) + a.tobytes()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The two golden waves and their joined wave: fbank through the recognizer, written as .npz, .npy, a Kaldi archive
    (binary float entries under the keys hello and cat) and a script file with offsets into it (the other order)."""
    from test_gpu_recognizer import CAT, CONF, HELLO
    from test_gpu_online_utterances import GAP, write_wav
    d = tmp_path_factory.mktemp("recognize_features")
    joined = np.concatenate([pk.read_wav(HELLO), np.zeros(GAP, np.float32), pk.read_wav(CAT)]).astype(np.float32)
    rec = pk.Recognizer(CONF, max_utts=1, max_total_samples=len(joined))
    fb = {}
    for name, wave in (("hello", pk.read_wav(HELLO)), ("cat", pk.read_wav(CAT)), ("joined", joined)):
        rec.process([wave])
        fb[name] = rec.batch.fetch_fbank(0)
    rec.close()
    p = {k: str(d / k) for k in ("feats.npz", "hello.npy", "joined.npy", "feats.ark", "feats.scp", "waves.scp", "joined.wav")}
    np.savez(p["feats.npz"], hello=fb["hello"], cat=fb["cat"])
    np.save(p["hello.npy"], fb["hello"])
    np.save(p["joined.npy"], fb["joined"])
    offsets = {}
    with open(p["feats.ark"], "wb") as f:
        for key in ("hello", "cat"):
            f.write(key.encode() + b" ")
            offsets[key] = f.tell()
            f.write(binary_matrix(fb[key]))
    with open(p["feats.scp"], "w") as f:
        f.write("".join("%s %s:%d\n" % (k, p["feats.ark"], offsets[k]) for k in ("cat", "hello")))
    with open(p["waves.scp"], "w") as f:
        f.write(HELLO + "\n" + CAT + "\n")
    write_wav(p["joined.wav"], joined)
    return CONF, {"hello": HELLO, "cat": CAT}, p, fb


def run(capsys, conf, *args):
    capsys.readouterr()
    rc = recognize.main([conf] + list(args))
    out = capsys.readouterr()
    assert rc == 0, out.out + out.err
    return out.out.splitlines(), out.err.splitlines()


def renamed(lines, names, sep):
    for short, path in names.items():
        lines = [l.replace(path + sep, short + sep, 1) if l.startswith(path + sep) else l for l in lines]
    return lines


def test_features_online_print_the_lines_of_the_batch_call_and_of_the_waves(files, capsys):
    conf, waves, p, _ = files
    want, _ = run(capsys, conf, p["feats.npz"], "--features", "raw")
    assert len(want) == 2 and all(l.split("\t")[1] for l in want)
    assert run(capsys, conf, p["feats.npz"], "--features", "raw", "--online")[0] == want
    assert renamed(run(capsys, conf, p["waves.scp"], "--online")[0], waves, "\t") == want
    assert run(capsys, conf, p["feats.npz"], "--features", "raw", "--online", "--chunk-ms", "5")[0] == want      # one frame a push


@pytest.mark.parametrize("online", [False, True])
def test_archives_and_script_files_print_the_same_lines_under_their_keys(files, capsys, online):
    conf, waves, p, _ = files
    flags = ["--features", "raw"] + (["--online"] if online else [])
    want, _ = run(capsys, conf, p["feats.npz"], "--features", "raw")
    for spec in (p["feats.ark"], "ark:" + p["feats.ark"]):
        assert run(capsys, conf, spec, *flags)[0] == want
    for spec in (p["feats.scp"], "scp:" + p["feats.scp"]):
        assert run(capsys, conf, spec, *flags)[0] == want[::-1]             # the script file lists cat first


def test_archive_entries_are_processed_in_groups(files, capsys, monkeypatch):
    """MAX_UTTS = 1: every entry is a group of its own (read, decoded and printed before the next one is read)."""
    conf, waves, p, _ = files
    want, _ = run(capsys, conf, p["feats.npz"], "--features", "raw")
    monkeypatch.setattr(recognize, "MAX_UTTS", 1)
    seen = []
    real = recognize.emit
    monkeypatch.setattr(recognize, "emit", lambda files_, *a, **k: (seen.append(list(files_)), real(files_, *a, **k))[1])
    assert run(capsys, conf, p["feats.ark"], "--features", "raw")[0] == want
    assert seen == [["hello"], ["cat"]]
    seen.clear()
    assert run(capsys, conf, p["feats.scp"], "--features", "raw", "--online")[0] == want[::-1]
    assert seen == [["cat"], ["hello"]]


def test_ctm_partials_commit_and_endpointing_from_features(files, capsys):
    conf, waves, p, fb = files
    # --ctm, one utterance: the word times of the wave file
    from_wave, _ = run(capsys, conf, waves["hello"], "--online", "--ctm")
    from_feats, _ = run(capsys, conf, p["hello.npy"], "--features", "raw", "--online", "--ctm")
    assert from_feats == renamed(from_wave, {p["hello.npy"]: waves["hello"]}, " ") and from_feats
    # --partials --commit: stdout unchanged; every partial line is "<name> TAB <seconds of frames fed> TAB <text> TAB <stable>"
    plain, _ = run(capsys, conf, p["hello.npy"], "--features", "raw")
    out, err = run(capsys, conf, p["hello.npy"], "--features", "raw", "--online", "--partials", "--commit")
    assert out == plain and err
    T = fb["hello"].shape[0]
    last = None
    for line in err:
        name, seconds, text, stable = line.split("\t")
        fed = round(float(seconds) * 100)
        assert name == p["hello.npy"] and 0 < fed <= T and (fed % 10 == 0 or fed == T)
        assert text.split()[:len(stable.split())] == stable.split()
        last = text
    assert last == plain[0].split("\t")[1]
    # --endpoint-silence: the utterances OnlineRecognizer cuts when it is fed the same frames in the same steps
    out, _ = run(capsys, conf, p["joined.npy"], "--features", "raw", "--online", "--reference-softmax", *ENDPOINT)
    from test_gpu_online_utterances import RULES, SILENCE
    rec = pk.OnlineRecognizer(conf, max_streams=1, max_step_samples=1600)
    rec.am.set_softmax("reference")
    rec.set_endpointing(SILENCE, RULES)
    rec.open_features(0, "raw")
    x = fb["joined"]
    for at in range(0, x.shape[0], 10):
        rec.push_features(0, x[at:at + 10])
        if at + 10 >= x.shape[0]:
            rec.close(0)
        rec.step()
    pieces = rec.utterances(0)
    rec.destroy()
    assert len(pieces) >= 3
    assert out == ["%s[%.2f-%.2f]\t%s\t%f" % (p["joined.npy"], q.first_frame * 0.01, (q.first_frame + q.num_frames) * 0.01, q.result.text,
                                              q.result.loglikelihood_per_frame) for q in pieces]
    # ... which are the audio tool's cuts at the same frames per step: compare the texts, piece by piece
    audio, _ = run(capsys, conf, p["joined.wav"], "--online", "--reference-softmax", *ENDPOINT)
    assert [l.split("\t")[1] for l in audio if l.split("\t")[1]] == [l.split("\t")[1] for l in out if l.split("\t")[1]]
