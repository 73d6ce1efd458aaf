"""Delta features, what holds without a device:
  * pk.delta_scales and pk.add_deltas (pk_mi355_deltas_scales / _apply: the C lines the kernel shares) equal the numpy
    restatement of the rule (tests/delta_cases.py) as bits, at every spec and frame count of the issue, on the
    norm_cases inputs and on wide ones;
  * the tests' inputs tell the rule from a fused multiply-add, from j descending, from zero taps that are not skipped,
    from zero padding and from scales formed in double (counts re-measured here and printed);
  * every refusal of the spec by code and field name, null arguments, parse_deltas, the new names in header, map and
    EXPORTS, the command line's usage errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import recognize

import delta_cases as DC
import norm_cases as NC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
D = 97
NEW_ENTRIES = ["pk_mi355_deltas_check", "pk_mi355_deltas_dim", "pk_mi355_deltas_scales", "pk_mi355_deltas_apply",
               "pk_mi355_deltas_batch_create", "pk_mi355_deltas_base_dim", "pk_mi355_deltas_recognizer_load"]

_inputs = {}


def inputs(T):
    """(the norm_cases input, the wide one): computed once, shared, left unchanged."""
    if T not in _inputs:
        _inputs[T] = (NC.features(T, D), DC.wide(T, D))
    return _inputs[T]


# ---------------------------------------------------------------- the host entries are the restatement

@pytest.mark.parametrize("order, window", DC.SPECS)
def test_scales_are_the_restatement(order, window):
    got = pk.delta_scales(pk.DeltaSpec(order, window))
    assert got.shape == (order + 1, 2 * order * window + 1)
    assert DC.bits_equal(got, DC.scale_table(order, window))
    if (order, window) == (2, 2):                              # Kaldi's well-known defaults
        assert np.allclose(got[1, 2:7], [-0.2, -0.1, 0.0, 0.1, 0.2], atol=1e-7)
        assert np.allclose(got[2], [0.04, 0.04, 0.01, -0.04, -0.1, -0.04, 0.01, 0.04, 0.04], atol=1e-7)


@pytest.mark.parametrize("order, window", DC.SPECS)
def test_host_rule_is_the_restatement(order, window):
    spec = pk.DeltaSpec(order, window)
    assert spec.dim(D) == (order + 1) * D
    for T in DC.frame_counts(order, window):
        for x in inputs(T):
            got = pk.add_deltas(x, spec)
            assert got.shape == (T, (order + 1) * D)
            assert DC.bits_equal(got, DC.add_deltas(x, order, window)), (order, window, T)
            assert DC.bits_equal(got[:, :D], x + np.float32(0.0))            # block 0: +0.0f + 1.0f * x


def test_edge_values():
    """-0.0 comes out of block 0 as +0.0; an inf at a centre tap of a first-order delta does not become NaN; a NaN spoils
    its own column only, within M_i frames of it."""
    order, window, T = 2, 2, 40
    x = inputs(130)[0][:T].copy()
    x[7, 3], x[20, 5], x[30, 8] = np.nan, np.inf, -0.0
    got = pk.add_deltas(x, pk.DeltaSpec(order, window))
    want = DC.add_deltas(x, order, window)
    assert DC.same_but_nan(got, want)
    assert got[30, 8].tobytes() == np.float32(0.0).tobytes()
    assert got[20, 5] == np.inf and not np.isnan(got[20, D + 5])              # the centre scale of block 1 is zero: skipped
    assert np.isnan(DC.add_deltas(x, order, window, keep_zero_taps=True)[20, D + 5])
    for i in range(order + 1):
        M = i * window
        nan_rows = np.isnan(got[:, i * D + 3])
        assert nan_rows[7 - M:7 + M + 1].sum() >= 1 and not nan_rows[:7 - M].any() and not nan_rows[7 + M + 1:].any()
    clean = np.ones(D, bool)
    clean[[3, 5]] = False
    for i in range(order + 1):
        assert np.isfinite(got[:, i * D:(i + 1) * D][:, clean]).all()


# ---------------------------------------------------------------- the inputs tell the rule from what it might be mistaken for

def variant_counts(order, window):
    """{variant: outputs changed}, summed over the frame counts and both inputs, plus the pinning inputs' own counts."""
    total = dict.fromkeys(DC.VARIANTS, 0)
    outputs = 0
    for T in DC.frame_counts(order, window):
        for x in inputs(T):
            want = DC.add_deltas(x, order, window)
            outputs += want.size
            for v in DC.VARIANTS:
                total[v] += DC.outputs_differing(DC.add_deltas(x, order, window, **{v: True}), want)
    return total, outputs


@pytest.mark.parametrize("order, window", DC.SPECS)
def test_inputs_tell_the_rule_from_its_variants(order, window):
    total, outputs = variant_counts(order, window)
    print("order=%d window=%d, %d outputs: %s" % (order, window, outputs, ", ".join("%s %d" % kv for kv in total.items())))
    assert total["zero_padding"] > 0
    if (order, window) == (1, 1):
        # two taps of scale -0.5 and 0.5: both products are exact and the first add is to +0.0, so one rounding is left --
        # a fused add and the other order give the same bits; the other specs pin these two variants
        assert total["fused"] == 0 and total["descending"] == 0
    else:
        assert total["fused"] > 0 and total["descending"] > 0
    # finite inputs never see a skipped zero tap (0 * x adds +0.0, or -0.0 to a sum that is not -0.0): an inf at a centre pins it
    assert total["keep_zero_taps"] == 0
    x = inputs(130)[0].copy()
    x[60, 11] = np.inf
    want = DC.add_deltas(x, order, window)
    kept = DC.outputs_differing(DC.add_deltas(x, order, window, keep_zero_taps=True), want)
    print("  an inf at (60, 11): keeping the zero taps changes %d outputs" % kept)
    assert kept > 0 and DC.same_but_nan(pk.add_deltas(x, pk.DeltaSpec(order, window)), want)
    # T <= M pins the edge rule on its own (T = 1 at order 1 does not: the replicated frame's products cancel exactly)
    M = order * window
    for T in sorted({2, M} - {1}):
        x = inputs(T)[0]
        want = DC.add_deltas(x, order, window)
        assert DC.bits_equal(pk.add_deltas(x, pk.DeltaSpec(order, window)), want)
        padded = DC.outputs_differing(DC.add_deltas(x, order, window, zero_padding=True), want)
        print("  T=%d: zero padding changes %d of %d outputs" % (T, padded, want.size))
        assert padded > 0, T
    # the scales formed in double differ from the float ones wherever a rounding of the float recursion shows
    dbl = np.concatenate([s for s in DC.scales(order, window, double_scales=True)])
    flt = np.concatenate([s for s in DC.scales(order, window)])
    print("  scales formed in double differ in %d of %d entries" % (int((dbl.view(np.uint32) != flt.view(np.uint32)).sum()), flt.size))
    assert (total["double_scales"] > 0) == bool((dbl.view(np.uint32) != flt.view(np.uint32)).any())


def has_inner_zero(order, window):
    """Some block i >= 1 has a zero scale strictly inside its own 2 i window + 1 taps (the centre of an odd-order block)."""
    return any((s[1:-1] == 0.0).any() for s in DC.scales(order, window)[1:])


def test_every_spec_has_a_zero_centre_tap_in_block_one():
    for order, window in DC.SPECS:
        s = DC.scales(order, window)
        assert s[1][window] == 0.0 and has_inner_zero(order, window)


# ---------------------------------------------------------------- refusals

def code_and_text(call):
    with pytest.raises(pk.PkCodeError) as e:
        call()
    return e.value.code, str(e.value)


@pytest.mark.parametrize("spec, field", [
    (pk.DeltaSpec(0, 2), "order"), (pk.DeltaSpec(4, 2), "order"), (pk.DeltaSpec(-1, 2), "order"),
    (pk.DeltaSpec(2, 0), "window"), (pk.DeltaSpec(2, 9), "window"), (pk.DeltaSpec(2, -3), "window"),
])
def test_bad_specs_are_refused_by_field_name(spec, field):
    code, text = code_and_text(spec.check)
    assert code == E_INVALID and text.startswith("deltas spec:") and field in text, text
    for call in (lambda: pk.add_deltas(np.zeros((2, 3), np.float32), spec), lambda: pk.delta_scales(spec), lambda: spec.dim(13)):
        code, text2 = code_and_text(call)
        assert code == E_INVALID and text2 == text


def test_good_specs_and_parse_deltas():
    for order in (1, 2, 3):
        for window in (1, 8):
            pk.DeltaSpec(order, window).check()
    s = pk.parse_deltas("")
    assert (s.order, s.window) == (2, 2) and pk.DeltaSpec().dim(13) == 39 and pk.DeltaSpec().dim(40) == 120
    s = pk.parse_deltas(" order = 3 , window=1 ")
    assert (s.order, s.window) == (3, 1)
    assert pk.parse_deltas("window=5").window == 5
    for text, word in (("ordr=2", "ordr"), ("order=two", "order"), ("window", "window"), ("order=1,order=1", "twice"),
                       ("order=2.5", "order")):
        with pytest.raises(ValueError) as e:
            pk.parse_deltas(text)
        assert word in str(e.value)
    code, text = code_and_text(lambda: pk.DeltaSpec().dim(0))
    assert code == E_INVALID and "base dimension" in text
    code, text = code_and_text(lambda: pk.add_deltas(np.zeros(4, np.float32), pk.DeltaSpec()))
    assert code == E_INVALID and "[T][D]" in text


def test_null_arguments_are_refused():
    L = pk.lib()
    spec = pk.DeltaSpec().struct()
    x, y = np.zeros((2, 3), np.float32), np.zeros((2, 9), np.float32)
    f32p = C.POINTER(C.c_float)
    assert L.pk_mi355_deltas_check(None) == E_INVALID and "null" in L.pk_mi355_last_error().decode()
    assert L.pk_mi355_deltas_dim(None, 3) == E_INVALID
    assert L.pk_mi355_deltas_scales(None, y.ctypes.data_as(f32p)) == E_INVALID
    assert L.pk_mi355_deltas_scales(C.byref(spec), None) == E_INVALID
    assert L.pk_mi355_deltas_apply(None, x.ctypes.data_as(f32p), 2, 3, y.ctypes.data_as(f32p)) == E_INVALID
    assert L.pk_mi355_deltas_apply(C.byref(spec), None, 2, 3, y.ctypes.data_as(f32p)) == E_INVALID
    assert L.pk_mi355_deltas_apply(C.byref(spec), x.ctypes.data_as(f32p), 2, 3, None) == E_INVALID
    assert L.pk_mi355_deltas_apply(C.byref(spec), x.ctypes.data_as(f32p), -1, 3, y.ctypes.data_as(f32p)) == E_INVALID
    assert L.pk_mi355_deltas_apply(C.byref(spec), x.ctypes.data_as(f32p), 2, 0, y.ctypes.data_as(f32p)) == E_INVALID
    assert L.pk_mi355_deltas_apply(C.byref(spec), None, 0, 3, None) == 0                        # no frames: nothing to read
    assert L.pk_mi355_deltas_base_dim(None) == 0
    assert not L.pk_mi355_deltas_batch_create(None, C.byref(spec), None, None, 0, 1, 10)
    assert not L.pk_mi355_deltas_recognizer_load(None, None, C.byref(spec), 0, 1, 16000, 0)
    assert "null" in L.pk_mi355_last_error().decode()


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
    assert "pk_mi355_deltas_spec_t" in header and C.sizeof(pk.pk_mi355_deltas_spec_t) == 8
    assert C.sizeof(pk.pk_mi355_frontend_spec_t) == 28                          # untouched: energy has its own route later
    for name in ("DeltaSpec", "parse_deltas", "delta_scales", "add_deltas"):
        assert name in pk.__all__ and hasattr(pk, name)


# ---------------------------------------------------------------- the command line's usage errors (before any device call)

def test_command_line_usage_errors(tmp_path, capsys):
    conf, wav = str(tmp_path / "no-such-model.conf"), str(tmp_path / "no-such.wav")
    for extra, words in (
            (["--deltas"], ["--deltas needs a value"]),
            (["--deltas", "ordr=2"], ["--deltas", "ordr"]),
            (["--deltas", "order=4"], ["--deltas", "order 4"]),
            (["--deltas", "order=2,window=0"], ["--deltas", "window 0"]),
            (["--deltas", "order=2,window=2", "--online"], ["the live objects do not have deltas yet"]),
            (["--deltas", "order=2", "--features", "raw", "--online"], ["the live objects do not have deltas yet"])):
        assert recognize.main([conf, wav] + extra) == 1, extra
        out = capsys.readouterr().out
        assert "Usage:" in out and "--deltas" in out, extra
        for w in words:
            assert w in out, (extra, w, out)
    recognize.usage()
    out = capsys.readouterr().out
    assert "--features normalized matrices [T][the model's dimension]" in out
    # a model file that cannot be read is an error of its own, not a usage error
    assert recognize.main([conf, wav, "--deltas", "order=2,window=2"]) == 1
    out = capsys.readouterr().out
    assert "Usage:" not in out
