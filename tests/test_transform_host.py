"""Feature transforms, what holds without a device:
  * pk.transform_feats (pk_mi355_transform_apply: the C lines the kernel shares) equals the numpy restatement of the rule
    (tests/transform_cases.py) as bits, at every spec and frame count of the issue, on the norm_cases inputs and on wide
    ones, and lies within the derived bound of a float64 product of the spliced rows;
  * the tests' inputs tell the rule from a fused multiply-add, from k descending, from the offset added first, from zero
    padding and from a neighbour's per-utterance matrix (counts re-measured here and printed);
  * NaN and inf placement, -0.0; every refusal of the spec by code and field name, null arguments, the ambiguity of cols
    at L = R = 0 without in_dim, parse_transform, the new names in header and EXPORTS."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import pocketkaldi_amd as pk

import transform_cases as XC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NEW_ENTRIES = ["pk_mi355_transform_check", "pk_mi355_transform_out_dim", "pk_mi355_transform_apply", "pk_mi355_transform_batch_create",
               "pk_mi355_transform_in_dim", "pk_mi355_transform_set_utt", "pk_mi355_transform_recognizer_load"]

_inputs = {}


def inputs(T, D):
    """(the norm_cases input, the wide one): computed once, shared, left unchanged."""
    if (T, D) not in _inputs:
        _inputs[T, D] = (XC.features(T, D), XC.wide(T, D))
    return _inputs[T, D]


def spec_of(m, L, R, in_dim):
    return pk.TransformSpec(m, L, R, in_dim=in_dim)


# ---------------------------------------------------------------- the host entry is the restatement

@pytest.mark.parametrize("in_dim, L, R, rows, affine", XC.HOST_SPECS)
def test_host_rule_is_the_restatement(in_dim, L, R, rows, affine):
    m = XC.matrix(in_dim, L, R, rows, affine)
    spec = spec_of(m, L, R, in_dim)
    assert spec.out_dim == rows
    for T in XC.frame_counts(L, R):
        for x in inputs(T, in_dim):
            got = pk.transform_feats(x, spec)
            assert got.shape == (T, rows) and got.dtype == np.float32
            assert XC.bits_equal(got, XC.transform(x, m, L, R)), (in_dim, L, R, rows, affine, T)


@pytest.mark.parametrize("in_dim, L, R, rows, affine", XC.HOST_SPECS)
def test_within_the_derived_bound_of_a_float64_product(in_dim, L, R, rows, affine):
    m = XC.matrix(in_dim, L, R, rows, affine)
    spec = spec_of(m, L, R, in_dim)
    for x in inputs(33, in_dim):
        ref, bound = XC.float64_bound(x, m, L, R)
        err = np.abs(pk.transform_feats(x, spec).astype(np.float64) - ref)
        print("spec %s: max err / bound = %.3g" % ((in_dim, L, R, rows, affine), float((err / bound).max())))
        assert (err <= bound).all()


def test_without_a_matrix_the_rows_pass():
    spec = pk.TransformSpec(None, in_dim=7)
    assert spec.out_dim == 7
    x = inputs(33, 7)[1]
    assert XC.bits_equal(pk.transform_feats(x, spec), x)


def test_splice_feats_repeats_the_edge_frames():
    x = inputs(5, 3)[0]
    got = pk.splice_feats(x, 2, 1)
    assert got.shape == (5, 12)
    for t in range(5):
        for j in range(-2, 2):
            assert XC.bits_equal(got[t, (j + 2) * 3:(j + 3) * 3], x[min(max(t + j, 0), 4)])
    assert pk.splice_feats(np.zeros((0, 3), np.float32), 2, 1).shape == (0, 12)
    # the transform at L, R is the L = R = 0 transform of the spliced rows
    m = XC.matrix(3, 2, 1, 6, True)
    assert XC.bits_equal(pk.transform_feats(x, pk.TransformSpec(m, 2, 1)), pk.transform_feats(got, pk.TransformSpec(m, in_dim=12)))


# ---------------------------------------------------------------- the inputs tell the wrong variants apart

def test_variants_differ_from_the_rule():
    """The table of DESIGN.md section 25: outputs changed of outputs total over T in {1, 2, L + R, L + R + 1, 33}, N(0, 1)
    data.  The cells that can show the variant are not zero.  At K = 1 none can: one tap has no order, is never at an
    edge, fma(m, x, +0.0f) is the rounded product, and with a single tap "offset first" is the same two adds commuted;
    the (1, 0, 0, 1) row is there to show exactly that."""
    expect_zero = {((40, 4, 4, 40, False), "offset_first")} | {((1, 0, 0, 1, True), v) for v in XC.VARIANTS}
    for sp in XC.VARIANT_SPECS:
        in_dim, L, R, rows, affine = sp
        m = XC.matrix(*sp)
        counts = dict.fromkeys(XC.VARIANTS, 0)
        total = 0
        for T in sorted({1, 2, L + R, L + R + 1, 33} - {0}):
            x = XC.normal(T, in_dim, seed=T)
            want = XC.transform(x, m, L, R)
            total += want.size
            for v in XC.VARIANTS:
                counts[v] += XC.outputs_differing(XC.transform(x, m, L, R, **{v: True}), want)
        print("spec %s: %s of %d" % (sp, counts, total))
        for v in XC.VARIANTS:
            if (sp, v) in expect_zero:
                assert counts[v] == 0, (sp, v)
            else:
                assert counts[v] > 0, (sp, v)


def test_a_neighbours_matrix_shows():
    xs = [XC.normal(T, 40, seed=T) for T in (5, 1, 9)]
    mats = [XC.matrix(40, 0, 0, 40, True, seed=20 + u) for u in range(3)]
    good, bad = XC.transform_utts(xs, mats), XC.transform_utts(xs, mats, neighbour=True)
    for g, b_, x, m in zip(good, bad, xs, mats):
        assert XC.outputs_differing(g, b_) > g.size // 2
        assert XC.bits_equal(pk.transform_feats(x, pk.TransformSpec(m, in_dim=40)), g)


# ---------------------------------------------------------------- edge values

def test_nan_spoils_frames_t_minus_R_to_t_plus_L():
    in_dim, L, R, rows = 13, 3, 2, 40
    m = XC.matrix(in_dim, L, R, rows, True)
    x = inputs(33, in_dim)[0].copy()
    x[10, 4] = np.nan
    x[0, 0] = np.nan                                   # an edge frame is read for every frame in front of the first, too
    got = pk.transform_feats(x, pk.TransformSpec(m, L, R))
    want = XC.transform(x, m, L, R)
    assert XC.same_but_nan(got, want)
    nan_rows = np.isnan(got).all(axis=1)
    assert not (np.isnan(got).any(axis=1) & ~nan_rows).any()
    assert sorted(np.flatnonzero(nan_rows)) == sorted(set(range(0, 0 + L + 1)) | set(range(10 - R, 10 + L + 1)))


def test_inf_under_a_zero_entry_is_nan_and_negative_zero_does_not_survive():
    m = np.zeros((2, 3), np.float32)
    m[0, 0] = 1.0
    m[1, 1] = 1.0
    x = np.array([[np.inf, 1.0, 2.0], [-0.0, -0.0, -0.0], [1.0, np.inf, 0.0]], np.float32)
    got = pk.transform_feats(x, pk.TransformSpec(m, in_dim=3))
    assert np.isinf(got[0, 0]) and np.isnan(got[0, 1])          # row 1's zero entry meets the inf: no tap is skipped
    assert np.isnan(got[2, 0]) and np.isinf(got[2, 1])
    assert XC.bits_equal(got[1], np.zeros(2, np.float32))       # +0.0, not -0.0
    assert XC.same_but_nan(got, XC.transform(x, m, 0, 0))
    neg = pk.transform_feats(x[1:2], pk.TransformSpec(-m, in_dim=3))
    assert XC.bits_equal(neg, np.zeros((1, 2), np.float32))


# ---------------------------------------------------------------- refusals

def raw_spec(L=0, R=0, in_dim=4, rows=2, cols=4, matrix="auto"):
    keep = None
    if isinstance(matrix, str):
        keep = np.ones((max(rows, 1), max(cols, 1)), np.float32)
        ptr = keep.ctypes.data_as(C.POINTER(C.c_float))
    elif matrix is None:
        ptr = None
    else:
        keep = matrix
        ptr = keep.ctypes.data_as(C.POINTER(C.c_float))
    return pk.pk_mi355_transform_spec_t(L, R, in_dim, rows, cols, ptr), keep


@pytest.mark.parametrize("kw, words", [
    (dict(L=-1), ["left_context", "-1"]),
    (dict(L=17, cols=72), ["left_context", "17"]),
    (dict(R=-2), ["right_context", "-2"]),
    (dict(R=17, cols=72), ["right_context", "17"]),
    (dict(L=9, R=8, cols=72), ["left_context 9", "right_context 8", "16"]),
    (dict(in_dim=0, cols=0), ["in_dim", "0"]),
    (dict(in_dim=513, cols=513), ["in_dim", "513"]),
    (dict(rows=0), ["rows", "0"]),
    (dict(rows=2049), ["rows", "2049"]),
    (dict(cols=6), ["cols 6", "4", "5"]),
    (dict(L=1, R=1, cols=14), ["cols 14", "12", "13"]),
    (dict(matrix=None), ["null matrix"]),
    (dict(matrix=None, rows=0, cols=0, L=1), ["null matrix"]),
])
def test_spec_refusals_name_the_field(kw, words):
    st, keep = raw_spec(**kw)
    L = pk.lib()
    for rc in (L.pk_mi355_transform_check(C.byref(st)), L.pk_mi355_transform_out_dim(C.byref(st))):
        assert rc == E_INVALID
        text = L.pk_mi355_last_error().decode()
        assert text.startswith("transform spec:")
        for w in words:
            assert w in text, (w, text)


def test_limits_are_accepted():
    for kw in (dict(L=16, R=0, in_dim=1, cols=17), dict(L=0, R=16, in_dim=2, cols=35), dict(in_dim=512, cols=512), dict(rows=2048, cols=5),
               dict(matrix=None, rows=0, cols=0)):
        st, keep = raw_spec(**kw)
        assert pk.lib().pk_mi355_transform_check(C.byref(st)) == 0, kw
    st, keep = raw_spec(matrix=None, rows=0, cols=0, in_dim=9)
    assert pk.lib().pk_mi355_transform_out_dim(C.byref(st)) == 9


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_the_first_entry_that_is_not_finite_is_named(bad):
    m = np.ones((3, 5), np.float32)
    m[1, 4] = bad
    m[2, 0] = bad
    with pytest.raises(pk.PkCodeError) as e:
        pk.TransformSpec(m, in_dim=4).check()
    assert e.value.code == E_INVALID and "row 1, column 4" in str(e.value) and "not finite" in str(e.value)


def test_null_arguments_and_shapes():
    L = pk.lib()
    assert L.pk_mi355_transform_check(None) == E_INVALID and b"null argument" in L.pk_mi355_last_error()
    assert L.pk_mi355_transform_out_dim(None) == E_INVALID
    st, keep = raw_spec()
    y = np.zeros((2, 2), np.float32)
    x = np.zeros((2, 4), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.pk_mi355_transform_apply(None, fp(x), 2, fp(y)) == E_INVALID
    assert L.pk_mi355_transform_apply(C.byref(st), None, 2, fp(y)) == E_INVALID and b"null argument" in L.pk_mi355_last_error()
    assert L.pk_mi355_transform_apply(C.byref(st), fp(x), 2, None) == E_INVALID
    assert L.pk_mi355_transform_apply(C.byref(st), fp(x), -1, fp(y)) == E_INVALID and b"-1 frames" in L.pk_mi355_last_error()
    assert L.pk_mi355_transform_apply(C.byref(st), fp(x), 2, fp(x)) == E_INVALID and b"may not be the input" in L.pk_mi355_last_error()
    assert L.pk_mi355_transform_apply(C.byref(st), None, 0, None) == 0                       # no frames: nothing happens
    with pytest.raises(pk.PkCodeError, match="the transform reads"):
        pk.transform_feats(np.zeros((2, 5), np.float32), pk.TransformSpec(np.ones((2, 4), np.float32), in_dim=4))
    assert pk.lib().pk_mi355_transform_in_dim(None) == 0
    assert L.pk_mi355_transform_set_utt(None, None, 0, 0, 0) == E_INVALID


def test_in_dim_is_required_where_cols_is_ambiguous():
    m = np.ones((40, 41), np.float32)
    with pytest.raises(pk.PkCodeError, match="in_dim is required when left_context = right_context = 0") as e:
        pk.TransformSpec(m)
    assert "41 -> linear or 40 -> affine" in str(e.value)
    with pytest.raises(pk.PkCodeError, match="in_dim is required without a matrix"):
        pk.TransformSpec()
    assert pk.TransformSpec(m, in_dim=41).out_dim == 40 and pk.TransformSpec(m, in_dim=40).out_dim == 40
    # with a context the width follows from cols: 92 = 7 * 13 + 1, 360 = 9 * 40
    assert pk.TransformSpec(np.ones((40, 92), np.float32), 3, 3).in_dim == 13
    assert pk.TransformSpec(np.ones((40, 360), np.float32), 4, 4).in_dim == 40
    with pytest.raises(pk.PkCodeError, match="cols 93 is neither 91 .* nor 92"):
        pk.TransformSpec(np.ones((40, 93), np.float32), 3, 3).check()


# ---------------------------------------------------------------- parse_transform

def write_kaldi_matrix(path, m):
    m = np.ascontiguousarray(m, np.float32)
    with open(path, "wb") as f:
        f.write(b"\0BFM " + struct.pack("<bibi", 4, m.shape[0], 4, m.shape[1]) + m.tobytes())


def test_parse_transform(tmp_path):
    m = XC.matrix(13, 3, 3, 40, True)
    path = str(tmp_path / "final.mat")
    write_kaldi_matrix(path, m)
    spec = pk.parse_transform("matrix=%s,left_context=3,right_context=3" % path)
    assert (spec.left_context, spec.right_context, spec.in_dim, spec.out_dim) == (3, 3, 13, 40)
    assert XC.bits_equal(spec.matrix, m)
    spec = pk.parse_transform(" in_dim=92 , matrix=%s " % path)
    assert (spec.left_context, spec.right_context, spec.in_dim) == (0, 0, 92)
    for text, words in (("left_context=3", "no matrix"), ("matrix=%s,window=2" % path, "unknown key 'window'"),
                        ("matrix=%s,matrix=%s" % (path, path), "key 'matrix' given twice"),
                        ("matrix=%s,left_context=x" % path, "bad value 'x' for key 'left_context'"),
                        ("matrix=%s,right_context" % path, "bad value '' for key 'right_context'"), ("matrix=", "bad value '' for key 'matrix'")):
        with pytest.raises(ValueError, match=re.escape(words)):
            pk.parse_transform(text)
    with pytest.raises(pk.PkError):
        pk.parse_transform("matrix=%s,in_dim=3" % str(tmp_path / "missing.mat"))
    with pytest.raises(pk.PkCodeError, match="in_dim is required"):
        pk.parse_transform("matrix=%s" % path)


# ---------------------------------------------------------------- the names

def test_new_entries_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "pk_mi355.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pk.EXPORTS
        assert hasattr(pk.lib(), name)
    assert C.sizeof(pk.pk_mi355_transform_spec_t) == 32 and pk.pk_mi355_transform_spec_t.matrix.offset == 24


# ---------------------------------------------------------------- the command line's usage errors

def test_command_line_usage_errors(tmp_path, capsys):
    from pocketkaldi_amd import recognize
    m = XC.matrix(13, 3, 3, 40, True)
    path = str(tmp_path / "final.mat")
    write_kaldi_matrix(path, m)
    good = "matrix=%s,left_context=3,right_context=3" % path
    trans = str(tmp_path / "trans.ark")
    with open(trans, "wb") as f:
        f.write(b"utt0 ")
    write_ark = open(trans, "ab")
    u = np.eye(40, 41, dtype=np.float32)
    write_ark.write(b"\0BFM " + struct.pack("<bibi", 4, 40, 4, 41) + u.tobytes())
    write_ark.close()

    def refused(args, words):
        assert recognize.main(["model.conf", "a.wav"] + args) == 1
        out = capsys.readouterr().out
        assert "Usage:" in out
        for w in words:
            assert w in out, (w, out)

    refused(["--online", "--transform", good], ["the live objects do not have transforms yet: leave out --online"])
    refused(["--online", "--utt-transforms", "ark:" + trans], ["the live objects do not have transforms yet: leave out --online"])
    refused(["--online", "--deltas", "order=2,window=2", "--transform", good], ["the live objects do not have deltas yet: leave out --online"])
    refused(["--transform"], ["--transform needs a value"])
    refused(["--utt-transforms"], ["--utt-transforms needs a value"])
    refused(["--transform", "left_context=3"], ["--transform:", "no matrix"])
    refused(["--transform", good + ",window=2"], ["--transform:", "unknown key 'window'"])
    refused(["--transform", "matrix=%s" % path], ["--transform:", "in_dim is required"])
    refused(["--transform", "matrix=%s,left_context=3,right_context=4" % path], ["--transform:", "cols 92"])
    refused(["--transform", "matrix=%s,in_dim=3" % str(tmp_path / "missing.mat")], ["--transform:"])
    refused(["--utt-transforms", "ark:" + str(tmp_path / "missing.ark")], ["--utt-transforms:"])
    empty = str(tmp_path / "empty.ark")
    open(empty, "wb").close()
    refused(["--utt-transforms", "ark:" + empty], ["--utt-transforms:", "holds no matrix"])
    refused(["--utt-transforms", "ark:" + trans, "--utt2spk"], ["--utt2spk needs a value"])
    bad_map = str(tmp_path / "utt2spk")
    with open(bad_map, "w") as f:
        f.write("utt0 spk0 extra\n")
    refused(["--utt-transforms", "ark:" + trans, "--utt2spk", bad_map], ["--utt2spk: line 1"])
    # --utt2spk without anything keyed by speaker stays --cmvn's refusal
    refused(["--utt2spk", bad_map], ["--cmvn-stats and --utt2spk go with --cmvn mode=speaker or mode=online"])
    # a missing key names it
    t = recognize.Transforms(None, {"utt0": u}, None)
    with pytest.raises(recognize.UsageError, match="--utt-transforms: no transform for utterance 'utt1'"):
        t.utt_transforms(["utt0", "utt1"])
    t = recognize.Transforms(None, {"spk0": u}, {"utt0": "spk0", "utt1": "spk1"})
    assert len(t.utt_transforms(["utt0"])) == 1
    with pytest.raises(recognize.UsageError, match="--utt-transforms: no transform for speaker 'spk1'"):
        t.utt_transforms(["utt1"])
    with pytest.raises(recognize.UsageError, match="--utt2spk: no speaker for utterance 'utt2'"):
        t.utt_transforms(["utt2"])
    for cls in (pk.OnlineScorer, pk.OnlineFeatureScorer, pk.OnlineRecognizer):    # the live objects take no transform
        with pytest.raises(TypeError):
            cls(None, None, 1, 1, transform=pk.TransformSpec(m, 3, 3))
