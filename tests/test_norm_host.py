"""The normalisation spec, what holds without a device:
  * pk.cmvn_normalize (pk_mi355_norm_apply: the C lines the kernel shares) equals the numpy restatement of the rule
    (tests/norm_cases.py) as bits, outputs and statistics, in every mode and switch pair;
  * the tests' inputs tell the rule from float accumulation, from a fused apply step and -- through the statistics,
    compared as doubles -- from another summation order (counts re-measured here and printed);
  * every refusal of the spec by code and field name, null arguments, the new names in header, map and EXPORTS;
  * pk.kaldi_cmvn_stats keeps the doubles of binary and text files; the command line's usage errors."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import recognize

import norm_cases as NC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_IO, E_STATE = -1, -3, -4
D = 97
FRAMES = (0, 1, 2, 65, 700, 1307)
NEW_ENTRIES = ["pk_mi355_norm_check", "pk_mi355_norm_apply", "pk_mi355_norm_set", "pk_mi355_norm_set_speaker_stats",
               "pk_mi355_norm_fetch_stats", "pk_mi355_ark_matrix_f64"]

_inputs = {}


def inputs(T):
    """(x, its record): computed once, shared, left unchanged."""
    if T not in _inputs:
        x = NC.features(T, D)
        _inputs[T] = (x, NC.accumulate(x))
    return _inputs[T]


# ---------------------------------------------------------------- the host entry is the restatement

@pytest.mark.parametrize("T", FRAMES)
def test_host_rule_is_the_restatement(T):
    x, rec = inputs(T)
    got, none = pk.cmvn_normalize(x, pk.NormSpec("none"))
    assert NC.bits_equal(got, x) and none is None
    for means, variances in NC.SWITCHES:
        want, want_rec = NC.normalize(x, "utterance", means, variances)
        got, got_rec = pk.cmvn_normalize(x, pk.NormSpec("utterance", means, variances))
        assert NC.bits_equal(got, want), (T, means, variances)
        assert NC.bits_equal(got_rec, want_rec) and NC.bits_equal(got_rec, rec), (T, means, variances)       # as doubles
        if T == 0:
            continue
        spk, none = pk.cmvn_normalize(x, pk.NormSpec("speaker", means, variances), stats=rec)
        assert NC.bits_equal(spk, want) and none is None                       # its own record: the utterance call's bits
        other = rec * 3.0 + 1.0                                                  # any other record
        want, _ = NC.normalize(x, "speaker", means, variances, stats=other)
        got, _ = pk.cmvn_normalize(x, pk.NormSpec("speaker", means, variances), stats=other)
        assert NC.bits_equal(got, want), (T, means, variances)


def test_one_frame_meets_the_variance_floor_and_edge_values_stay_in_their_column():
    x, _ = inputs(1)
    got, _ = pk.cmvn_normalize(x, pk.NormSpec("utterance", True, True))
    assert NC.bits_equal(got, NC.normalize(x, "utterance", True, True)[0])
    offs, scale = NC.finalize(NC.accumulate(x), True, True)
    assert (scale == np.float32(1e10)).all()                                      # 1 / sqrt(1e-20)
    x = inputs(65)[0].copy()
    x[7, 3], x[9, 5], x[11, 8] = np.nan, np.inf, -0.0
    for means, variances in NC.SWITCHES:
        want, want_rec = NC.normalize(x, "utterance", means, variances)
        got, got_rec = pk.cmvn_normalize(x, pk.NormSpec("utterance", means, variances))
        touched = np.zeros(D, bool)
        touched[[3, 5]] = True
        assert np.isnan(want[:, 3]).all() and np.isfinite(want[:, ~touched]).all()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok])
        ok = ~np.isnan(want_rec)
        assert np.array_equal(np.isnan(got_rec), np.isnan(want_rec)) and np.array_equal(got_rec.view(np.uint64)[ok], want_rec.view(np.uint64)[ok])


# ---------------------------------------------------------------- the inputs tell the rule from what it might be mistaken for

def test_inputs_tell_the_rule_from_its_variants():
    """Outputs pin double accumulation and the unfused apply; the statistics, compared as doubles, pin the order."""
    for T in (2, 65, 700, 1307):
        x, rec = inputs(T)
        for means, variances in ((True, True), (True, False)):
            table = np.stack(NC.finalize(rec, means, variances))
            single = np.stack(NC.finalize(NC.accumulate(x, np.float32), means, variances))
            y = NC.apply(x, table[0], table[1], variances)
            cols_float = NC.columns_differing(table, single)
            fused = int((NC.apply(x, table[0], table[1], variances, fused=True).view(np.uint32) != y.view(np.uint32)).sum())
            inter = NC.accumulate_interleaved(x)
            ti = np.stack(NC.finalize(inter, means, variances))
            out_inter = NC.columns_differing(NC.apply(x, ti[0], ti[1], variances), y)
            s1_inter = NC.columns_differing(rec[1:2], inter[1:2])
            print("T=%d means=%d vars=%d: float accumulation changes the table in %d of %d columns; a fused apply %d of %d outputs; "
                  "four interleaved sums %d output columns, %d columns of the sums of squares"
                  % (T, means, variances, cols_float, D, fused, y.size, out_inter, s1_inter))
            if variances:
                assert cols_float >= 60
                assert fused > (20000 if T == 700 else 0)
            else:
                assert cols_float >= 60 if T >= 65 else cols_float == 0
            assert out_inter <= 2                                               # the outputs hardly see the order ...
            assert s1_inter >= 50 if T >= 65 else s1_inter == 0                 # ... the statistics do
        got_rec = pk.cmvn_normalize(x, pk.NormSpec("utterance", True, True))[1]
        assert NC.bits_equal(got_rec, rec) and (T < 65 or not NC.bits_equal(got_rec, NC.accumulate_interleaved(x)))


# ---------------------------------------------------------------- refusals

def code_and_text(call):
    with pytest.raises(pk.PkCodeError) as e:
        call()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("spec, field", [
    (pk.NormSpec(4), "mode"), (pk.NormSpec(-1), "mode"),
    (pk.NormSpec("sliding", False, False), "norm_means"), (pk.NormSpec("sliding", True, True), "norm_vars"),
    (pk.NormSpec("utterance", 2, False), "norm_means"), (pk.NormSpec("speaker", True, -1), "norm_vars"),
    (pk.NormSpec("sliding", 2, False), "norm_means"),
    (pk.NormSpec("utterance", False, False), "use mode none"), (pk.NormSpec("speaker", False, False), "use mode none"),
])
def test_bad_specs_are_refused_by_field_name(spec, field):
    code, text = code_and_text(spec.check)
    assert code == E_INVALID and text.startswith("norm spec:") and field in text, text
    code, text2 = code_and_text(lambda: pk.cmvn_normalize(np.zeros((2, 3), np.float32), spec, stats=np.ones((2, 4))))
    assert code == E_INVALID and text2 == text


def test_good_specs_pass():
    for spec in (pk.NormSpec(), pk.NormSpec("none", 7, -3), pk.NormSpec("utterance"), pk.NormSpec("utterance", True, True),
                 pk.NormSpec("utterance", False, True), pk.NormSpec("speaker", True, True), pk.parse_norm(""),
                 pk.parse_norm("mode=utterance,norm_vars=true"), pk.parse_norm(" mode = speaker , norm_means=0,norm_vars=1 ")):
        spec.check()
    s = pk.parse_norm("mode=utterance,norm_vars=true")
    assert (s.mode, s.norm_means, s.norm_vars) == (2, True, True)
    for text, word in (("mood=none", "mood"), ("mode=global", "mode"), ("norm_vars=yes", "norm_vars"), ("mode", "mode"),
                       ("mode=none,mode=none", "twice")):
        with pytest.raises(ValueError) as e:
            pk.parse_norm(text)
        assert word in str(e.value)


def test_host_entry_refusals():
    x = np.zeros((3, 4), np.float32)
    code, text = code_and_text(lambda: pk.cmvn_normalize(x, pk.NormSpec("sliding")))
    assert code == E_INVALID and "sliding" in text
    code, text = code_and_text(lambda: pk.cmvn_normalize(x, pk.NormSpec("speaker")))
    assert code == E_INVALID and "statistics" in text
    for count in (0.0, -1.0, np.nan, np.inf):
        rec = np.ones((2, 5))
        rec[0, 4] = count
        code, text = code_and_text(lambda: pk.cmvn_normalize(x, pk.NormSpec("speaker"), stats=rec))
        assert code == E_INVALID and "count" in text and "utterance 0" in text, text
    code, text = code_and_text(lambda: pk.cmvn_normalize(x, pk.NormSpec("speaker"), stats=np.ones((2, 4))))
    assert code == E_INVALID and "[1][2][5]" in text


def test_null_arguments_are_refused():
    L = pk.lib()
    spec = pk.NormSpec("utterance").struct()
    x = np.zeros((2, 3), np.float32)
    f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
    assert L.pk_mi355_norm_check(None) == E_INVALID and "null" in L.pk_mi355_last_error().decode()
    assert L.pk_mi355_norm_apply(None, x.ctypes.data_as(f32p), 2, 3, None, x.ctypes.data_as(f32p), None) == E_INVALID
    assert L.pk_mi355_norm_apply(C.byref(spec), None, 2, 3, None, x.ctypes.data_as(f32p), None) == E_INVALID
    assert L.pk_mi355_norm_apply(C.byref(spec), x.ctypes.data_as(f32p), 2, 3, None, None, None) == E_INVALID
    assert L.pk_mi355_norm_apply(C.byref(spec), x.ctypes.data_as(f32p), -1, 3, None, x.ctypes.data_as(f32p), None) == E_INVALID
    assert L.pk_mi355_norm_apply(C.byref(spec), x.ctypes.data_as(f32p), 2, 0, None, x.ctypes.data_as(f32p), None) == E_INVALID
    assert L.pk_mi355_norm_apply(C.byref(spec), None, 0, 3, None, None, None) == 0                 # no frames: nothing to read
    d = np.zeros(8)
    assert L.pk_mi355_norm_set(None, C.byref(spec)) == E_INVALID
    assert L.pk_mi355_norm_set_speaker_stats(None, d.ctypes.data_as(f64p), 1) == E_INVALID
    assert L.pk_mi355_norm_fetch_stats(None, 0, d.ctypes.data_as(f64p)) == E_INVALID
    assert L.pk_mi355_ark_matrix_f64(None, d.ctypes.data_as(f64p), 8) == E_INVALID


def test_new_entries_in_header_map_and_exports():
    header = open(os.path.join(REPO, "include", "pk_mi355.h")).read()
    ver = open(os.path.join(REPO, "pocketkaldi_amd", "csrc", "libpk_mi355.map")).read()
    patterns = re.findall(r"^\s*([A-Za-z0-9_*]+);", ver.split("local:")[0], re.M)
    L = pk.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pk.EXPORTS, name
        assert any(re.fullmatch(p.replace("*", ".*"), name) for p in patterns), name
        assert hasattr(L, name), name
    assert "pk_mi355_norm_spec_t" in header
    for name in ("NormSpec", "parse_norm", "cmvn_normalize", "kaldi_cmvn_stats"):
        assert name in pk.__all__ and hasattr(pk, name)


# ---------------------------------------------------------------- statistics files keep their doubles

def binary_matrix(m, token):
    m = np.ascontiguousarray(m, {"DM": "<f8", "FM": "<f4"}[token])
    return b"\0B" + token.encode() + b" " + struct.pack("<bi", 4, m.shape[0]) + struct.pack("<bi", 4, m.shape[1]) + m.tobytes()


def text_matrix(m):
    return (" [\n" + "\n".join("  " + " ".join(repr(float(v)) for v in row) for row in m) + " ]\n").encode()


def test_kaldi_cmvn_stats_keeps_the_doubles(tmp_path):
    x, rec = inputs(1307)
    assert not NC.bits_equal(rec.astype(np.float32).astype(np.float64), rec)        # a float reader would lose them
    for name, blob in (("bin", binary_matrix(rec, "DM")), ("txt", text_matrix(rec))):
        path = tmp_path / ("stats." + name)
        path.write_bytes(b"pad" + blob)
        got = pk.kaldi_cmvn_stats("%s:3" % path)
        assert got.dtype == np.float64 and NC.bits_equal(got, rec), name
        assert NC.bits_equal(pk.kaldi_global_stats("%s:3" % path), rec[0].astype(np.float32))      # stays as it is
    path = tmp_path / "stats.fm"
    path.write_bytes(binary_matrix(rec, "FM"))
    assert NC.bits_equal(pk.kaldi_cmvn_stats(path), rec.astype(np.float32).astype(np.float64))
    # an archive of records, and what is not a record
    ark = tmp_path / "spk.ark"
    ark.write_bytes(b"alice " + binary_matrix(rec, "DM") + b"bob " + text_matrix(rec * 2))
    got = pk.read_cmvn_stats_archive("ark:%s" % ark)
    assert list(got) == ["alice", "bob"] and NC.bits_equal(got["alice"], rec) and NC.bits_equal(got["bob"], rec * 2)
    for bad in (np.zeros((3, 5)), np.zeros((2, 1)), np.zeros((1, 5))):
        path.write_bytes(binary_matrix(bad, "DM"))
        code, text = code_and_text(lambda: pk.kaldi_cmvn_stats(path))
        assert code == E_INVALID and "2 x (D + 1)" in text
    path.write_bytes(binary_matrix(rec, "DM")[:-5])
    assert code_and_text(lambda: pk.kaldi_cmvn_stats(path))[0] == E_IO
    # three rows and more are features: no doubles are kept for them
    path.write_bytes(b"k " + text_matrix(np.arange(12.0).reshape(3, 4)))
    with pk.ArkReader(path) as r:
        key, m = next(r)
        assert key == "k" and m.shape == (3, 4)
        out = np.zeros(12)
        assert pk.lib().pk_mi355_ark_matrix_f64(r._h, out.ctypes.data_as(C.POINTER(C.c_double)), 12) == E_INVALID
    path.write_bytes(b"k " + binary_matrix(np.arange(8.0).reshape(2, 4), "DM"))
    with pk.ArkReader(path) as r:
        next(r)
        out = np.zeros(8)
        assert pk.lib().pk_mi355_ark_matrix_f64(r._h, out.ctypes.data_as(C.POINTER(C.c_double)), 7) == E_INVALID
        assert pk.lib().pk_mi355_ark_matrix_f64(r._h, out.ctypes.data_as(C.POINTER(C.c_double)), 8) == 8
        assert np.array_equal(out, np.arange(8.0))


# ---------------------------------------------------------------- the command line's usage errors (before any device call)

def test_command_line_usage_errors(tmp_path, capsys):
    x, rec = inputs(2)
    stats = tmp_path / "spk.ark"
    stats.write_bytes(b"a " + binary_matrix(rec, "DM"))
    bad_map = tmp_path / "utt2spk"
    bad_map.write_text("one two three\n")
    conf, wav = str(tmp_path / "no-such-model.conf"), str(tmp_path / "no-such.wav")
    for extra, words in (
            (["--cmvn"], []),
            (["--cmvn", "mood=none"], ["--cmvn", "mood"]),
            (["--cmvn", "mode=sliding,norm_vars=true"], ["--cmvn", "norm_vars"]),
            (["--cmvn", "mode=utterance,norm_means=false"], ["use mode none"]),
            (["--cmvn", "mode=utterance", "--online"], ["online objects do not take a norm spec yet"]),
            (["--cmvn", "mode=speaker"], ["--cmvn-stats"]),
            (["--cmvn", "mode=utterance", "--cmvn-stats", str(stats)], ["mode=speaker"]),
            (["--cmvn-stats", str(stats)], ["mode=speaker"]),
            (["--utt2spk", str(bad_map)], ["mode=speaker"]),
            (["--cmvn", "mode=speaker", "--cmvn-stats", str(stats), "--utt2spk", str(bad_map)], ["line 1", "<utterance> <speaker>"]),
            (["--cmvn", "mode=speaker", "--cmvn-stats"], [])):
        assert recognize.main([conf, wav] + extra) == 1, extra
        out = capsys.readouterr().out
        assert "Usage:" in out and "--cmvn" in out, extra
        for w in words:
            assert w in out, (extra, w, out)
    # an archive that cannot be read is an error of its own, not a usage error
    assert recognize.main([conf, wav, "--cmvn", "mode=speaker", "--cmvn-stats", str(tmp_path / "none.ark")]) == 1
    out = capsys.readouterr().out
    assert "cannot open" in out and "Usage:" not in out
