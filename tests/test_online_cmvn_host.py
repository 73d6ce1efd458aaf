"""Online CMVN, what holds without a device:
  * pk.cmvn_online (pk_mi355_online_cmvn_apply: the C lines the kernel shares) equals the numpy restatement of the rule
    (tests/online_cmvn_cases.py) as bits, outputs and final window state compared as doubles, at every window, frame
    count, switch and prior of the issue's list, on the `norm_cases` inputs and on the wide ones;
  * the tests' inputs tell the rule from its four wrong variants: every variant changes at least one output bit
    (counts re-measured here and printed; DESIGN.md section 20 records them);
  * every refusal by code and field name, null arguments, the new names in header, map and EXPORTS, parse_norm, the
    command line's usage errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import recognize

import norm_cases as NC
import online_cmvn_cases as OC
from test_norm_host import binary_matrix

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
D = 97
NEW_ENTRIES = ["pk_mi355_online_cmvn_check", "pk_mi355_online_cmvn_apply", "pk_mi355_norm_set_online_cmvn"]
INPUTS = {"norm_cases": OC.features, "wide": OC.wide}

_priors = {}


def priors(name):
    """(global record, speaker record of count 37, speaker record of count 0) of one input family: computed once."""
    if name not in _priors:
        make = INPUTS[name]
        _priors[name] = (OC.record(make(300, D, 3)), OC.record(make(50, D, 5), OC.SPEAKER_COUNT), OC.record(make(50, D, 5), 0))
    return _priors[name]


# ---------------------------------------------------------------- the host entry is the restatement

@pytest.mark.parametrize("name", sorted(INPUTS))
@pytest.mark.parametrize("W, speaker_frames, global_frames", OC.SPECS)
def test_host_rule_is_the_restatement(W, speaker_frames, global_frames, name):
    glob, spk, spk0 = priors(name)
    g = glob if global_frames else None
    for T in OC.frame_counts(W):
        x = INPUTS[name](T, D)
        for variances in (False, True):
            spec = pk.OnlineCmvnSpec(W, speaker_frames, global_frames, variances)
            for s in (None, spk, spk0):
                want, want_state = OC.online_cmvn(x, W, speaker_frames, global_frames, variances, g, s)
                got, got_state = pk.cmvn_online(x, spec, g, s, return_state=True)
                what = (W, T, variances, None if s is None else s[0, D])
                assert got.dtype == np.float32 and NC.bits_equal(got, want), what
                assert NC.bits_equal(got_state, want_state), what                   # as doubles
                assert got_state[0, D] == T
            # a speaker record of count 0 is no speaker record
            assert NC.bits_equal(pk.cmvn_online(x, spec, g, spk0), pk.cmvn_online(x, spec, g, None))


def test_priors_matter_only_while_the_window_fills():
    W, T = 8, 40
    glob, spk, _ = priors("norm_cases")
    x = OC.features(T, D)
    spec = pk.OnlineCmvnSpec(W, 3, 2, True)
    plain = pk.cmvn_online(x, pk.OnlineCmvnSpec(W, 0, 0, True))
    both = pk.cmvn_online(x, spec, glob, spk)
    glob_only = pk.cmvn_online(x, spec, glob)
    assert NC.bits_equal(both[W - 1:], plain[W - 1:]) and NC.bits_equal(glob_only[W - 1:], plain[W - 1:])
    assert not NC.bits_equal(both[:W - 1], glob_only[:W - 1]) and not NC.bits_equal(glob_only[:W - 1], plain[:W - 1])
    # W = 1, no priors: every frame is its own mean
    one = pk.cmvn_online(x, pk.OnlineCmvnSpec(1, 0, 0, False))
    assert (one == 0.0).all()


def test_edge_values_poison_their_column_for_good():
    W, T = 8, 40
    glob, spk, _ = priors("norm_cases")
    x = OC.features(T, D).copy()
    x[5, 3], x[9, 11], x[7, 20] = np.nan, np.inf, -0.0
    for variances in (False, True):
        want, want_state = OC.online_cmvn(x, W, 3, 2, variances, glob, spk)
        got, got_state = pk.cmvn_online(x, pk.OnlineCmvnSpec(W, 3, 2, variances), glob, spk, return_state=True)
        assert np.isnan(want[5:, 3]).all()                                         # they do not leave with the window
        assert not np.isfinite(want[9:, 11]).any() and np.isnan(want[9, 11]) and np.isnan(want[9 + W:, 11]).all()     # (inf - inf)
        assert np.isfinite(want[:5, 3]).all() and np.isfinite(want[:9, 11]).all()
        touched = np.zeros(D, bool)
        touched[[3, 11]] = True
        assert np.isfinite(want[:, ~touched]).all()
        for a, b, u in ((got, want, np.uint32), (got_state, want_state, np.uint64)):
            ok = ~np.isnan(b)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(u)[ok], b.view(u)[ok])


# ---------------------------------------------------------------- the inputs tell the rule from what it might be mistaken for

VARIANTS = ("float_state", "fused", "prefix", "subtract_first")


def test_inputs_tell_the_rule_from_its_variants():
    """On the test's own inputs, at D = 97, W = 8 and T = 65, every wrong variant changes at least one output bit: the
    float state and the fused apply on the `norm_cases` inputs, the two order variants on the wide inputs."""
    W, T = 8, 65
    counts = {}
    for name in sorted(INPUTS):
        glob, spk, _ = priors(name)
        x = INPUTS[name](T, D)
        for variances in (False, True):
            right, _ = OC.online_cmvn(x, W, 3, 2, variances, glob, spk)
            assert NC.bits_equal(pk.cmvn_online(x, pk.OnlineCmvnSpec(W, 3, 2, variances), glob, spk), right)
            for v in VARIANTS:
                wrong, _ = OC.online_cmvn(x, W, 3, 2, variances, glob, spk, **{v: True})
                counts[(name, variances, v)] = int((wrong.view(np.uint32) != right.view(np.uint32)).sum())
                print("%s vars=%d %s: %d of %d outputs change" % (name, variances, v, counts[(name, variances, v)], right.size))
    assert counts[("norm_cases", False, "float_state")] > 0 and counts[("norm_cases", True, "float_state")] > 0
    assert counts[("norm_cases", True, "fused")] > 0                              # (without variance the apply is one add)
    for variances in (False, True):
        assert counts[("wide", variances, "prefix")] > 0 and counts[("wide", variances, "subtract_first")] > 0


# ---------------------------------------------------------------- refusals

def code_and_text(call):
    with pytest.raises(pk.PkCodeError) as e:
        call()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("spec, field", [
    (pk.OnlineCmvnSpec(0), "cmn_window"), (pk.OnlineCmvnSpec(-5), "cmn_window"), (pk.OnlineCmvnSpec(6001), "cmn_window"),
    (pk.OnlineCmvnSpec(8, -1, 2), "speaker_frames"), (pk.OnlineCmvnSpec(8, 3, -2), "global_frames"),
    (pk.OnlineCmvnSpec(8, 3, 2, 2), "norm_vars"), (pk.OnlineCmvnSpec(8, 3, 2, -1), "norm_vars"),
])
def test_bad_specs_are_refused_by_field_name(spec, field):
    glob = priors("norm_cases")[0]
    code, text = code_and_text(lambda: spec.check(glob))
    assert code == E_INVALID and text.startswith("online cmvn spec:") and field in text, text
    code, text2 = code_and_text(lambda: pk.cmvn_online(np.zeros((2, D), np.float32), spec, glob))
    assert code == E_INVALID and text2 == text


def test_statistics_refusals():
    glob, spk, _ = priors("norm_cases")
    x = np.zeros((3, D), np.float32)
    spec = pk.OnlineCmvnSpec(8, 3, 2)
    code, text = code_and_text(lambda: spec.check(None, D))
    assert code == E_INVALID and "global_frames" in text and "global statistics" in text
    code, text = code_and_text(lambda: pk.cmvn_online(x, spec))
    assert code == E_INVALID and "global_frames" in text
    for count in (0.0, -1.0, np.nan, np.inf):
        bad = glob.copy()
        bad[0, D] = count
        code, text = code_and_text(lambda: spec.check(bad))
        assert code == E_INVALID and "global_frames" in text and "count" in text, text
        assert code_and_text(lambda: pk.cmvn_online(x, spec, bad))[0] == E_INVALID
        pk.OnlineCmvnSpec(8, 3, 0).check(bad)                                     # not read without global_frames
    for count in (-1.0, np.nan, np.inf):
        bad = spk.copy()
        bad[0, D] = count
        code, text = code_and_text(lambda: pk.cmvn_online(x, spec, glob, bad))
        assert code == E_INVALID and "count" in text and "utterance 0" in text, text
    assert code_and_text(lambda: pk.cmvn_online(x, spec, glob[:, :-1]))[0] == E_INVALID      # shapes, refused in Python
    assert code_and_text(lambda: pk.cmvn_online(x, spec, glob, spk[:, :-1]))[0] == E_INVALID
    assert code_and_text(lambda: pk.cmvn_online(np.zeros(3, np.float32), spec, glob))[0] == E_INVALID
    for good in (pk.OnlineCmvnSpec(), pk.OnlineCmvnSpec(1, 0, 2), pk.OnlineCmvnSpec(6000, 0, 1, True)):
        good.check(glob)
    pk.OnlineCmvnSpec(8, 3, 0, True).check(None, D)


def test_null_arguments_are_refused():
    L = pk.lib()
    spec = pk.OnlineCmvnSpec(8, 3, 0).struct()
    x = np.zeros((2, 3), np.float32)
    f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
    xp = x.ctypes.data_as(f32p)
    assert L.pk_mi355_online_cmvn_check(None, None, 3) == E_INVALID and "null" in L.pk_mi355_last_error().decode()
    assert L.pk_mi355_online_cmvn_apply(None, xp, 2, 3, None, None, xp, None) == E_INVALID
    assert L.pk_mi355_online_cmvn_apply(C.byref(spec), None, 2, 3, None, None, xp, None) == E_INVALID
    assert L.pk_mi355_online_cmvn_apply(C.byref(spec), xp, 2, 3, None, None, None, None) == E_INVALID
    assert L.pk_mi355_online_cmvn_apply(C.byref(spec), xp, -1, 3, None, None, xp, None) == E_INVALID
    assert L.pk_mi355_online_cmvn_apply(C.byref(spec), xp, 2, 0, None, None, xp, None) == E_INVALID
    state = np.ones((2, 4))
    assert L.pk_mi355_online_cmvn_apply(C.byref(spec), None, 0, 3, None, None, None, state.ctypes.data_as(f64p)) == 0      # no frames: nothing to read
    assert (state == 0.0).all()
    assert L.pk_mi355_norm_set_online_cmvn(None, C.byref(spec), None) == E_INVALID


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
    assert "pk_mi355_online_cmvn_spec_t" in header
    for name in ("OnlineCmvnSpec", "cmvn_online"):
        assert name in pk.__all__ and hasattr(pk, name)


def test_parse_norm():
    s = pk.parse_norm("mode=online,cmn_window=600,speaker_frames=600,global_frames=200,norm_vars=true")
    assert isinstance(s, pk.OnlineCmvnSpec) and (s.cmn_window, s.speaker_frames, s.global_frames, s.norm_vars) == (600, 600, 200, True)
    s = pk.parse_norm(" mode = online , cmn_window = 8 ")
    assert (s.cmn_window, s.speaker_frames, s.global_frames, s.norm_vars) == (8, 600, 200, False)
    assert isinstance(pk.parse_norm("mode=utterance"), pk.NormSpec)
    for text, word in (("cmn_window=8", "cmn_window"), ("mode=utterance,speaker_frames=3", "speaker_frames"),
                       ("mode=speaker,global_frames=3", "global_frames"), ("mode=online,norm_means=false", "norm_means"),
                       ("mode=online,cmn_window=x", "cmn_window"), ("mode=online,cmn_window", "cmn_window"),
                       ("mode=online,cmn_window=8,cmn_window=9", "twice")):
        with pytest.raises(ValueError) as e:
            pk.parse_norm(text)
        assert word in str(e.value), text


# ---------------------------------------------------------------- the command line's usage errors (before any device call)

def test_command_line_usage_errors(tmp_path, capsys):
    glob = priors("norm_cases")[0]
    stats = tmp_path / "global.stats"
    stats.write_bytes(binary_matrix(glob, "DM"))
    conf, wav = str(tmp_path / "no-such-model.conf"), str(tmp_path / "no-such.wav")
    for extra, words in (
            (["--cmvn", "mode=online"], ["--cmvn-global", "global_frames"]),
            (["--cmvn", "mode=online,cmn_window=0", "--cmvn-global", str(stats)], ["cmn_window"]),
            (["--cmvn", "mode=online,speaker_frames=-1,global_frames=0"], ["speaker_frames"]),
            (["--cmvn", "mode=utterance,cmn_window=8"], ["cmn_window"]),
            (["--cmvn", "mode=utterance", "--cmvn-global", str(stats)], ["--cmvn-global", "mode=online"]),
            (["--cmvn-global", str(stats)], ["--cmvn-global", "mode=online"]),
            (["--cmvn", "mode=utterance,norm_vars=true", "--online"], ["online objects do not take a norm spec yet", "live"]),
            (["--cmvn", "mode=online", "--online"], ["--cmvn-global", "global_frames"]),
            (["--cmvn", "mode=online", "--cmvn-global"], [])):
        assert recognize.main([conf, wav] + extra) == 1, extra
        out = capsys.readouterr().out
        assert "Usage:" in out and "--cmvn" in out, extra
        for w in words:
            assert w in out, (extra, w, out)
    # statistics that cannot be read are an error of their own, not a usage error
    assert recognize.main([conf, wav, "--cmvn", "mode=online", "--cmvn-global", str(tmp_path / "none.stats")]) == 1
    out = capsys.readouterr().out
    assert "cannot open" in out and "Usage:" not in out
