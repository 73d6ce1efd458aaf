"""CPU-only: the feature entries of the batch scorer exist in the header, the link map and the
binding, and their argument checks answer before the device is touched -- a null batch, null matrices, a wrong nrow, a
negative ncol and a bad kind come back as PK_MI355_E_INVALID, nothing dereferenced.  (A batch cannot be made without a
GPU, so the checks that need one -- nrow against the model's feat_dim, the capacities -- are repeated on a live batch in
test_gpu_features.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pocketkaldi_amd as pk

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pk_mi355_features_batch_create", "pk_mi355_features_set", "pk_mi355_features_set_device",
       "pk_mi355_features_dim", "pk_mi355_recognizer_process_features"]
E_INVALID, E_STATE = -1, -4


def test_names_are_in_the_header_the_map_and_the_binding():
    header = open(os.path.join(REPO, "include", "pk_mi355.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pk.EXPORTS, name
    assert re.search(r"#define\s+PK_MI355_FEATS_NORMALIZED\s+0\b", header) and re.search(r"#define\s+PK_MI355_FEATS_RAW\s+1\b", header)
    assert pk.FEATURE_KINDS == {"normalized": 0, "raw": 1}
    # the link map exports the ABI by its two prefixes: the new names are covered, and the library has them
    link_map = open(os.path.join(REPO, "pocketkaldi_amd", "csrc", "libpk_mi355.map")).read()
    assert "pk_mi355_*;" in link_map
    pk.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", pk.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NEW) <= exported
    from pocketkaldi_amd import build
    assert "features.hip" in build.HIP_SOURCES
    assert "LaunchFeatureLayout" not in open(os.path.join(build.CSRC, "pk_kernels.h")).read()


def matrix(a):
    m = pk.pk_matrix_t()
    m.ncol, m.nrow = a.shape
    m.data = a.ctypes.data_as(C.POINTER(C.c_float))
    return m


def test_null_and_malformed_arguments_are_invalid_before_any_device_call():
    L = pk.lib()
    x = np.zeros((3, 40), np.float32)
    good, wrong_nrow, negative = matrix(x), matrix(x), matrix(x)
    wrong_nrow.nrow = 39
    negative.ncol = -1
    n = (C.c_int * 1)(3)
    for kind in (0, 1, 2, -1):
        for m in (good, wrong_nrow, negative):
            assert L.pk_mi355_features_set(None, C.byref(m), 1, kind) == E_INVALID
            assert L.pk_mi355_last_error_code() == E_INVALID and L.pk_mi355_last_error()
            assert L.pk_mi355_recognizer_process_features(None, C.byref(m), 1, kind) == E_INVALID
        assert L.pk_mi355_features_set(None, None, 1, kind) == E_INVALID
        assert L.pk_mi355_features_set_device(None, None, n, 1, kind) == E_INVALID
        assert L.pk_mi355_features_set_device(None, None, None, 1, kind) == E_INVALID
        assert L.pk_mi355_recognizer_process_features(None, None, 1, kind) == E_INVALID
    assert L.pk_mi355_features_dim(None) == 0
    # create: a null or unfinished model is a call-order error, as for pk_mi355_batch_create; nothing is made
    assert not L.pk_mi355_features_batch_create(None, None, 1, 16)
    assert L.pk_mi355_last_error_code() == E_STATE
    am = L.pk_mi355_am_create()
    try:
        assert not L.pk_mi355_features_batch_create(am, None, 1, 16)
        assert L.pk_mi355_last_error_code() == E_STATE
    finally:
        L.pk_mi355_am_destroy(am)


def test_single_utterance_entries_refuse_an_unfinished_model_in_their_old_words():
    """pk_decodable_init and pk_mi355_am_calibrate answer a null or unfinished model before anything else, with the text
    they had before they became calls on the model's own features batch (the other texts need a finalized model:
    test_gpu_single_utterance.py)."""
    L = pk.lib()
    m = matrix(np.zeros((3, 40), np.float32))
    am = L.pk_mi355_am_create()
    try:
        for handle in (None, am):
            d = pk.pk_decodable_t()
            L.pk_decodable_init(C.byref(d), handle, 0.1, C.byref(m))
            assert d.log_prob.ncol == 0 and not d.log_prob.data
            assert L.pk_mi355_last_error_code() == E_STATE and L.pk_mi355_last_error() == b"model not finalized"
            assert L.pk_mi355_am_calibrate(handle, C.byref(m)) == E_STATE
            assert L.pk_mi355_last_error() == b"model not finalized"
    finally:
        L.pk_mi355_am_destroy(am)


class _Scorer(pk.BatchScorer):
    """A BatchScorer whose handle is null: what the wrappers refuse, they refuse before they call the library."""

    def __init__(self, dim):
        self._h, self._am, self._keep, self._dim = None, None, None, dim

    def feat_dim(self):
        return self._dim


@pytest.mark.parametrize("bad", [np.zeros(40, np.float32), np.zeros((2, 3, 40), np.float32), np.zeros((5, 39), np.float32),
                                 np.array([["a"] * 40]), [[1.0] * 40, [2.0] * 39], None])
def test_python_wrappers_refuse_what_is_not_a_feature_matrix(bad):
    s = _Scorer(40)
    with pytest.raises(pk.PkError):
        s.set_features([np.zeros((4, 40), np.float32), bad])
    with pytest.raises(pk.PkError, match="kind"):
        s.set_features([np.zeros((4, 40), np.float32)], kind="cmvn")
    with pytest.raises(pk.PkError, match="kind"):
        s.set_features_device(0, [4], kind=2)


def test_python_wrapper_converts_what_is_float_convertible():
    arr, keep = pk._feature_matrices([np.arange(6).reshape(2, 3), [[1, 2, 3]], np.zeros((0, 3), np.float64)], 3)
    assert [k.dtype for k in keep] == [np.float32] * 3 and [k.shape for k in keep] == [(2, 3), (1, 3), (0, 3)]
    assert [(arr[i].ncol, arr[i].nrow) for i in range(3)] == [(2, 3), (1, 3), (0, 3)]
    assert np.ctypeslib.as_array(arr[0].data, shape=(2, 3)).tolist() == [[0, 1, 2], [3, 4, 5]]


def test_command_line_refuses_features_it_cannot_take(tmp_path, capsys):
    from pocketkaldi_amd import recognize
    assert recognize.main(["model.conf", "feats.npz", "--features", "cmvn"]) == 1
    assert recognize.main(["model.conf", "feats.npz", "--features"]) == 1
    assert recognize.main(["model.conf", "feats.npz", "--features", "raw", "--online"]) == 1
    assert recognize.main(["model.conf", "feats.wav", "--features", "raw"]) == 1
    assert "--features raw|normalized" in capsys.readouterr().out
