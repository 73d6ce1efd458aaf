"""CPU-only: the front-end spec for live audio and the recognizers -- the four entries' names,
their refusals that come before the device, pk_mi355_load_stats' reader (also as a stand-alone program under the host
sanitizers: tests/cpp/files_stats_test.cc), the --frontend parser and the routing of frontend= in the Python classes.
The refusals that need a finalized model, which needs a device -- the spec's dimension against the model's, the statistics'
length and a capacity <= 0 at pk_mi355_frontend_stream_create -- are in tests/test_gpu_frontend_stream.py's
test_failure_codes; the recognizers' refusal of a spec of another dimension is in tests/test_gpu_frontend_recognizer.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import recognize
from pocketkaldi_amd import synth

import frontend_any_cases as FA
import refmodel_files as RF

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(REPO, "tests", "golden", "refmodel")
CSRC = os.path.join(REPO, "pocketkaldi_amd", "csrc")
E_INVALID, E_DEVICE, E_IO, E_STATE = -1, -2, -3, -4
NEW_ENTRIES = ["pk_mi355_frontend_stream_create", "pk_mi355_load_stats", "pk_mi355_frontend_recognizer_load",
               "pk_mi355_frontend_online_recognizer_load"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
f32p = C.POINTER(C.c_float)


def last():
    return pk.lib().pk_mi355_last_error_code(), pk.lib().pk_mi355_last_error().decode()


def fp(a):
    return a.ctypes.data_as(f32p)


# ------------------------------------------------------------------ names

def test_new_names_in_header_map_and_exports():
    header = open(os.path.join(REPO, "include", "pk_mi355.h")).read()
    vmap = open(os.path.join(REPO, "pocketkaldi_amd", "csrc", "libpk_mi355.map")).read()
    L = pk.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pk.EXPORTS and hasattr(L, name), name
    assert "pk_mi355_*;" in vmap
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    for name in NEW_ENTRIES:
        assert re.search(r" T %s$" % name, dyn, re.M), name
    hpp = open(os.path.join(REPO, "include", "pocketkaldi_amd.hpp")).read()
    for name in NEW_ENTRIES[:1] + NEW_ENTRIES[2:]:
        assert name in hpp, name


# ------------------------------------------------------------------ refusals before the device

def model(precision=0):
    am = pk.lib().pk_mi355_am_create()
    assert am and pk.lib().pk_mi355_am_set_precision(am, precision) == 0
    return am


def test_stream_create_refusals():
    L = pk.lib()
    good, g = FA.BATCH_SPECS[80].struct(), np.zeros(81, np.float32)
    assert not L.pk_mi355_frontend_stream_create(None, C.byref(good), fp(g), 81, 2, 1600)
    assert last() == (E_INVALID, "null model")
    am = model()
    try:
        assert not L.pk_mi355_frontend_stream_create(am, None, fp(g), 81, 2, 1600)
        assert last() == (E_INVALID, "null argument")
        assert not L.pk_mi355_frontend_stream_create(am, C.byref(good), None, 81, 2, 1600)
        assert last() == (E_INVALID, "null argument")
        # a bad spec, in pk_mi355_frontend_check's words
        for spec, field in ((FA.S(bins=129), "num_mel_bins"), (FA.S("mfcc", 23, 24), "num_ceps"), (FA.S(window=2), "window"),
                            (FA.S(low=4000.0, high=4000.0), "high_freq"), (FA.S(bins=127), "empty triangle")):
            st = spec.struct()
            assert L.pk_mi355_frontend_check(C.byref(st)) == E_INVALID
            words = last()[1]
            assert field in words
            assert not L.pk_mi355_frontend_stream_create(am, C.byref(st), fp(g), 81, 2, 1600)
            assert last() == (E_INVALID, words)
        assert not L.pk_mi355_frontend_stream_create(am, C.byref(good), fp(g), 81, 2, 1600)      # f32, not finalized
        assert last() == (E_STATE, "model not finalized")
    finally:
        L.pk_mi355_am_destroy(am)
    for precision in (1, 2):                     # PK_MI355_PRECISION_F16X3, _F16: refused, as on every online scorer
        am = model(precision)
        try:
            assert not L.pk_mi355_frontend_stream_create(am, C.byref(good), fp(g), 81, 2, 1600)
            code, words = last()
            assert code == E_INVALID and "f32" in words
        finally:
            L.pk_mi355_am_destroy(am)


def test_python_constructor_raises_with_the_code():
    am = pk.AcousticModel.__new__(pk.AcousticModel)
    am._h = model(1)
    try:
        with pytest.raises(pk.PkCodeError) as e:
            pk.OnlineScorer(am, np.zeros(81, np.float32), 2, 1600, frontend=FA.BATCH_SPECS[80])
        assert e.value.code == E_INVALID and "f32" in str(e.value)
        with pytest.raises(pk.PkCodeError) as e:
            pk.OnlineScorer(am, np.zeros(81, np.float32), 2, 1600, frontend=FA.S(bins=2))
        assert e.value.code == E_INVALID and "num_mel_bins" in str(e.value)
        with pytest.raises(pk.PkError, match="41 entries"):          # without frontend=: the old constructor
            pk.OnlineScorer(am, np.zeros(81, np.float32), 2, 1600)
    finally:
        am.close()


def recognizer_files(tmp_path, D, stats_len, L=2, R=1):
    """A model file of a D-dim model with the fixture's graph and word list beside it -> the .conf."""
    layers, prior, _, _ = synth.model("tiny", feat_dim=D, left=L, right=R)
    conf = RF.write_model(tmp_path, layers, prior, L, R, cmvn_stats=np.arange(stats_len, dtype=np.float32) + 0.5)
    for name in ("wordloop.fst", "wordloop_words.bin"):
        shutil.copy(os.path.join(DIR, name), str(tmp_path / name))
    with open(conf, "a") as f:
        f.write("fst = wordloop.fst\nsymbol_table = wordloop_words.bin\n")
    return conf


def test_recognizer_load_refusals(tmp_path):
    L = pk.lib()
    good = FA.BATCH_SPECS[80].struct()
    conf = recognizer_files(tmp_path, 80, 14).encode()
    batch = lambda c, s, utts=2, samples=16000, trace=0: L.pk_mi355_frontend_recognizer_load(c, s, 0, utts, samples, trace)
    online = lambda c, s, streams=2, samples=1600, trace=0: L.pk_mi355_frontend_online_recognizer_load(c, s, streams, samples, trace)
    for load in (batch, online):
        assert not load(None, C.byref(good))
        assert last() == (E_INVALID, "null argument")
        assert not load(conf, None)
        assert last() == (E_INVALID, "null argument")
        bad = FA.S("mfcc", 23, 0).struct()                            # a bad spec: refused first, the field named
        assert not load(b"/nowhere/model.conf", C.byref(bad))
        code, words = last()
        assert code == E_INVALID and "num_ceps" in words
        for args in ((0, 1600, 0), (2, 0, 0), (2, 1600, -1)):
            assert not load(conf, C.byref(good), *args)
            code, words = last()
            assert code == E_INVALID and "capacity" in words
        assert not load(b"/nowhere/model.conf", C.byref(good))
        code, words = last()
        assert code == E_IO and "/nowhere/model.conf" in words
        # statistics that are not the model's: pk_mi355_load_stats' refusal, both numbers and the file named
        assert not load(conf, C.byref(good))
        code, words = last()
        assert code == E_IO and "14 entries" in words and "80-dim" in words and "81" in words and "cmvn.bin" in words, words
    # more statistics than any spec has features
    conf = recognizer_files(tmp_path, 80, 130).encode()
    for load in (batch, online):
        assert not load(conf, C.byref(good))
        code, words = last()
        assert code == E_IO and "130 entries" in words and "129" in words and "cmvn.bin" in words, words
    # the 40-dim entries keep their words on the same file
    assert not L.pk_mi355_recognizer_load(conf, 0, 2, 16000, 0)
    assert last()[0] == E_IO and "has 130 entries, 41 expected" in last()[1]
    assert not L.pk_mi355_online_recognizer_load(conf, 2, 1600, 0)
    assert last()[0] == E_IO and "has 130 entries, 41 expected" in last()[1]
    for cls in (pk.Recognizer, pk.OnlineRecognizer):
        with pytest.raises(pk.PkCodeError) as e:
            cls(conf.decode(), frontend=FA.BATCH_SPECS[80])
        assert e.value.code == E_IO and "130 entries" in str(e.value)


# ------------------------------------------------------------------ pk_mi355_load_stats

def load_stats(conf, cap=129, precision=0):
    am, n, stats = C.c_void_p(), C.c_int(-7), np.full(max(cap, 1), -1.0, np.float32)
    rc = pk.lib().pk_mi355_load_stats(os.fspath(conf).encode(), precision, C.byref(am), fp(stats), cap, C.byref(n))
    return rc, am, n.value, stats


@pytest.mark.parametrize("D", [13, 80])
def test_load_stats_on_written_model_files(D, tmp_path):
    L = pk.lib()
    layers, prior, _, _ = synth.model("tiny", feat_dim=D, left=2, right=1)
    g = (np.arange(D + 1) * 3 + 0.25).astype(np.float32)
    conf = RF.write_model(tmp_path, layers, prior, 2, 1, cmvn_stats=g)
    rc, am, n, stats = load_stats(conf)
    if L.pk_mi355_device_count() > 0:
        assert rc == 0 and n == D + 1 and np.array_equal(stats[:n], g) and np.all(stats[n:] == -1.0)
        assert L.pk_mi355_am_feat_dim(am) == D and L.pk_mi355_am_num_pdfs(am) == len(prior)
        L.pk_mi355_am_destroy(am)
        model, got = pk.AcousticModel.load_stats(conf)
        assert model.feat_dim() == D and np.array_equal(got, g)
        model.close()
    else:                                        # every file read and found fitting; what fails is the device
        assert rc == E_DEVICE and not am.value and n == 0, last()
    # pk_mi355_load is unchanged on the same file
    out, s41 = C.c_void_p(), np.zeros(41, np.float32)
    assert L.pk_mi355_load(conf.encode(), 0, C.byref(out), fp(s41)) == E_IO
    assert last()[1] == "cmvn_stats in %s has %d entries, 41 expected" % (os.path.join(str(tmp_path), "cmvn.bin"), D + 1)
    with pytest.raises(pk.PkError, match="41 expected"):
        pk.AcousticModel.load(conf)
    # a capacity the vector does not fit
    rc, am, n, _ = load_stats(conf, cap=D)
    assert rc == E_IO and not am.value and n == 0
    words = last()[1]
    assert "%d entries" % (D + 1) in words and " %d " % D in words and "cmvn.bin" in words, words
    for cap in (0, -1):
        assert load_stats(conf, cap=cap)[0] == E_INVALID
    # statistics of another dimension than the model's: refused before the device, both numbers and the files named
    other = 81 if D == 13 else 14
    conf = RF.write_model(tmp_path, layers, prior, 2, 1, cmvn_stats=np.zeros(other, np.float32))
    rc, am, n, _ = load_stats(conf)
    assert rc == E_IO and not am.value and n == 0
    words = last()[1]
    assert "%d entries" % other in words and "%d-dim" % D in words and "needs %d" % (D + 1) in words, words
    assert "cmvn.bin" in words and "model.conf" in words
    with pytest.raises(pk.PkCodeError) as e:
        pk.AcousticModel.load_stats(conf)
    assert e.value.code == E_IO


def test_load_stats_null_arguments(tmp_path):
    L = pk.lib()
    am, n, stats = C.c_void_p(), C.c_int(), np.zeros(129, np.float32)
    assert L.pk_mi355_load_stats(None, 0, C.byref(am), fp(stats), 129, C.byref(n)) == E_INVALID
    assert L.pk_mi355_load_stats(b"x.conf", 0, None, fp(stats), 129, C.byref(n)) == E_INVALID
    assert L.pk_mi355_load_stats(b"x.conf", 0, C.byref(am), None, 129, C.byref(n)) == E_INVALID
    assert L.pk_mi355_load_stats(b"x.conf", 0, C.byref(am), fp(stats), 129, None) == E_INVALID
    assert last() == (E_INVALID, "null argument")
    assert L.pk_mi355_load_stats(str(tmp_path / "none.conf").encode(), 0, C.byref(am), fp(stats), 129, C.byref(n)) == E_IO


@pytest.mark.parametrize("flavour", [
    "plain",
    pytest.param("sanitized", marks=pytest.mark.skipif(pk.lib().pk_mi355_device_count() > 0,
                                                       reason="a GPU is present: sanitizer builds run on CPU machines only")),
])
def test_stats_reader_stands_alone(flavour, tmp_path):
    binary = os.path.join(REPO, "tests", "cpp", "files_stats_test_%s.bin" % flavour)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1"] + (SANITIZE if flavour == "sanitized" else []) +
                          [os.path.join(REPO, "tests", "cpp", "files_stats_test.cc"), os.path.join(CSRC, "pk_files.cc"), "-o", binary])
    run = subprocess.run([binary, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stderr == ""                               # a sanitizer reports there
    out = run.stdout.splitlines()
    assert out[-1] == "files_stats_test ok"
    assert out[:2] == ["good 14 ok", "good 81 ok"] and "truncated ok" in out and "capacity ok" in out
    assert any(re.fullmatch(r"poisoned \d\d ok", line) for line in out)


# ------------------------------------------------------------------ the --frontend parser

def test_parser_defaults_and_every_key():
    d = pk.parse_frontend("")
    assert (d.kind, d.num_mel_bins, d.num_ceps, d.window, d.low_freq, d.high_freq, d.cepstral_lifter) == (0, 40, 0, 0, 20.0, 0.0, 22.0)
    s = pk.parse_frontend("kind=mfcc,num_mel_bins=23,num_ceps=13,window=povey,low_freq=20,high_freq=-400,cepstral_lifter=22")
    assert (s.kind, s.num_mel_bins, s.num_ceps, s.window, s.low_freq, s.high_freq, s.cepstral_lifter) == (1, 23, 13, 1, 20.0, -400.0, 22.0)
    assert s.dim == 13
    assert pk.parse_frontend("kind=mfcc").num_ceps == 13                 # FrontendSpec's default for MFCC
    one = {"kind": ("mfcc", "kind", 1), "num_mel_bins": ("80", "num_mel_bins", 80), "num_ceps": ("7", "num_ceps", 7),
           "window": ("povey", "window", 1), "low_freq": ("100.5", "low_freq", 100.5), "high_freq": ("-400", "high_freq", -400.0),
           "cepstral_lifter": ("0", "cepstral_lifter", 0.0)}
    for key, (text, field, want) in one.items():
        got = pk.parse_frontend(" %s = %s " % (key, text))
        assert getattr(got, field) == want, key
        rest = [k for k in one if k != key and not (key == "kind" and k == "num_ceps")]
        assert all(getattr(got, k) == getattr(pk.FrontendSpec(), k) for k in rest), key
    e80 = pk.parse_frontend("num_mel_bins=80,window=povey,high_freq=-400")
    ref = FA.BATCH_SPECS[80]
    assert (e80.kind, e80.num_mel_bins, e80.window, e80.low_freq, e80.high_freq, e80.dim) == (ref.kind, 80, ref.window, 20.0, -400.0, 80)


@pytest.mark.parametrize("text,key", [("bins=80", "bins"), ("num_mel_bins=80,colour=red", "colour"), ("=3", "''"),
                                      ("num_mel_bins=eighty", "num_mel_bins"), ("num_mel_bins=80.5", "num_mel_bins"),
                                      ("num_ceps=", "num_ceps"), ("kind=plp", "kind"), ("window=hann", "window"),
                                      ("low_freq=low", "low_freq"), ("high_freq=nan", "high_freq"), ("cepstral_lifter", "cepstral_lifter"),
                                      ("num_ceps=3,num_ceps=4", "num_ceps")])
def test_parser_names_the_key(text, key):
    with pytest.raises(ValueError) as e:
        pk.parse_frontend(text)
    assert key in str(e.value)


def test_command_line_usage_errors_name_the_key(capsys):
    for argv, key in ((["m.conf", "x.wav", "--frontend", "bins=80"], "bins"),
                      (["m.conf", "x.wav", "--online", "--frontend", "num_ceps=many"], "num_ceps")):
        assert recognize.main(argv) == 1
        out = capsys.readouterr().out
        assert "--frontend" in out and "'%s'" % key in out and "Usage:" in out
    assert recognize.main(["m.conf", "x.wav", "--frontend"]) == 1       # no value
    assert "Usage:" in capsys.readouterr().out


# ------------------------------------------------------------------ routing of frontend= in the Python classes

def test_frontend_routing_in_python(monkeypatch):
    calls = []

    class Fake:
        def __getattr__(self, name):
            def entry(*args):
                calls.append((name, args))
                return 1234 if name.endswith(("create", "load")) else 0
            return entry

    class Am:
        handle = 77

    monkeypatch.setattr(pk, "lib", lambda: Fake())
    monkeypatch.setattr(pk.SymbolTable, "_borrowed", classmethod(lambda cls, h, owner: None))
    spec = FA.BATCH_SPECS[80]

    def spec_of(arg):
        st = arg._obj
        return (st.kind, st.num_mel_bins, st.num_ceps, st.window, st.low_freq, st.high_freq)

    sc = pk.OnlineScorer(Am(), np.zeros(81, np.float32), 3, 4800, frontend=spec)
    name, args = calls[0]
    assert name == "pk_mi355_frontend_stream_create" and args[0] == 77 and args[3:] == (81, 3, 4800)
    assert spec_of(args[1]) == (0, 80, 0, 1, 20.0, -400.0)
    sc._h = None
    calls.clear()
    sc = pk.OnlineScorer(Am(), np.zeros(41, np.float32), 3, 4800)
    assert calls[0][0] == "pk_mi355_stream_create"
    sc._h = None
    calls.clear()
    rec = pk.Recognizer("m.conf", "f32", 4, 32000, 5, frontend=spec)
    name, args = calls[0]
    assert name == "pk_mi355_frontend_recognizer_load" and args[0] == b"m.conf" and args[2:] == (0, 4, 32000, 5)
    assert spec_of(args[1]) == (0, 80, 0, 1, 20.0, -400.0)
    rec._h = None
    calls.clear()
    rec = pk.Recognizer("m.conf", "f32", 4, 32000, 5)
    assert calls[0] == ("pk_mi355_recognizer_load", (b"m.conf", 0, 4, 32000, 5))
    rec._h = None
    calls.clear()
    rec = pk.OnlineRecognizer("m.conf", 4, 6400, 5, frontend=spec)
    name, args = calls[0]
    assert name == "pk_mi355_frontend_online_recognizer_load" and args[0] == b"m.conf" and args[2:] == (4, 6400, 5)
    assert spec_of(args[1]) == (0, 80, 0, 1, 20.0, -400.0)
    rec._h = None
    calls.clear()
    rec = pk.OnlineRecognizer("m.conf", 4, 6400, 5)
    assert calls[0] == ("pk_mi355_online_recognizer_load", (b"m.conf", 4, 6400, 5))
    rec._h = None
