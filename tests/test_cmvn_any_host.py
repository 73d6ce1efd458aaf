"""CMVN at any feature dimension, what holds without a device:
  * the chunk rule cmvn_any (tests/cmvn_any_cases.py) is the oracle at D = 40 and invariant under column permutation;
  * the tests' inputs tell a float-only chain from the reference's widen / add / add / narrow step;
  * the new entries are in the header, the export map and EXPORTS, and refuse null arguments;
  * pk.FeatureScorer / pk.OnlineFeatureScorer route statistics by their length before the library is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pocketkaldi_amd as pk
from oracle import oracle as O

import cmvn_any_cases as CA

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
NEW_ENTRIES = ["pk_mi355_am_feat_dim", "pk_mi355_features_batch_create_stats", "pk_mi355_features_stream_create_stats",
               "pk_mi355_ark_open", "pk_mi355_ark_next", "pk_mi355_ark_key", "pk_mi355_ark_matrix", "pk_mi355_ark_close",
               "pk_mi355_ark_read_object"]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the chunk rule

@pytest.mark.parametrize("T", [0, 1, 199, 600, 601, 1300])
def test_chunk_rule_is_the_oracle_at_40(T):
    g, x = CA.stats_for(40), CA.features(T, 40, 1)
    assert bits_equal(CA.cmvn_any(g, x), O.cmvn(g, x))


@pytest.mark.parametrize("T", [1, 401, 601, 1300])
def test_chunk_rule_is_invariant_under_column_permutation(T):
    D = 97
    g, x = CA.stats_for(D), CA.features(T, D, 2)
    want = CA.cmvn_any(g, x)
    assert np.isfinite(want).all()
    rng = np.random.default_rng(T)
    for _ in range(3):
        p = rng.permutation(D)
        gp = np.concatenate([g[:D][p], g[D:]])
        assert bits_equal(CA.cmvn_any(gp, x[:, p]), want[:, p])


def test_inputs_tell_a_float_only_chain_from_the_double_step():
    """Why these inputs: a kernel that adds in f32 where cmvn.cc:44-70 widens to f64 cannot pass.  The numpy restatement
    with the double step IS the oracle on them; without it, both kinds of column (around 3 and around 1e4) differ on
    frames past the point where the window slides."""
    D, T = 41, 700
    g, x = CA.stats_for(D), CA.features(T, D, 3)
    want = CA.cmvn_any(g, x)
    assert bits_equal(CA.restated_chain(g, x, True), want)
    single = CA.restated_chain(g, x, False)
    differs = (single.view(np.uint32) != want.view(np.uint32))
    assert not differs[:CA.WINDOW].any()                       # while the window fills, one f32 add is the rule
    per_column = differs.sum(axis=0)
    print("frames on which the float-only chain differs: big column %d, the others %d..%d"
          % (per_column[D // 2], np.delete(per_column, D // 2).min(), np.delete(per_column, D // 2).max()))
    assert per_column[D // 2] >= 10 and np.delete(per_column, D // 2).min() >= 10


# ---------------------------------------------------------------- the interface

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


def test_null_arguments_are_refused():
    L = pk.lib()
    g = np.zeros(4, np.float32)
    gp = g.ctypes.data_as(C.POINTER(C.c_float))
    assert L.pk_mi355_am_feat_dim(None) == 0
    assert L.pk_mi355_features_batch_create_stats(None, gp, 4, 1, 10) is None
    assert L.pk_mi355_last_error_code() == E_STATE                  # as pk_mi355_features_batch_create: "model not finalized"
    assert L.pk_mi355_features_stream_create_stats(None, gp, 4, 1, 10) is None
    assert L.pk_mi355_last_error_code() == E_INVALID and "null" in L.pk_mi355_last_error().decode()


class _Unfinalized:
    """What the scorers' constructors read of a model: a handle.  Null stands for a model that is not finalized (its
    dimension is 0), so the routing is checked without a device."""
    handle = None

    def num_pdfs(self):
        return 0


@pytest.mark.parametrize("cls", [pk.FeatureScorer, pk.OnlineFeatureScorer])
def test_python_routes_on_the_length_of_the_statistics(cls):
    am = _Unfinalized()
    for n in (0, 1, 2, 40, 42, 81):
        with pytest.raises(pk.PkError, match="41") as e:
            cls(am, 1, 10, global_stats=np.zeros(n, np.float32))
        assert not isinstance(e.value, pk.PkCodeError), n           # refused before the library is called
        assert "feat_dim + 1" in str(e.value)
    with pytest.raises(pk.PkError, match="41"):
        cls(am, 1, 10, global_stats=np.zeros((41, 1), np.float32))
    # 41 entries go to the 40-dim entry, which names what it refuses
    with pytest.raises(pk.PkCodeError) as e:
        cls(am, 1, 10, global_stats=np.zeros(41, np.float32))
    assert e.value.code in (E_STATE, E_INVALID)
