"""CPU-only: the front-end at a specification -- the numpy restatement against the oracle, the
library's tables against independent constructions, the refusals, the interface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pocketkaldi_amd as pk
from oracle import oracle as O

import frontend_any_cases as FA

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
NEW_ENTRIES = ["pk_mi355_frontend_check", "pk_mi355_frontend_dim", "pk_mi355_frontend_default", "pk_mi355_frontend_tables",
               "pk_mi355_frontend_compute", "pk_mi355_frontend_batch_create"]
IDS = [FA.spec_id(s) for s in FA.ALL_SPECS]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tables():
    return {FA.spec_id(s): pk.frontend_tables(s) for s in FA.ALL_SPECS}


# ------------------------------------------------------------------ the restatement is the oracle's rule

@pytest.mark.parametrize("wave", ["golden", "int16", "float"])
def test_default_spec_restatement_equals_the_oracle(wave, tables):
    if wave == "golden":
        w = O.wav_read(os.path.join(REPO, "tests", "golden", "en-us-hello.wav"))[:16000]
    else:
        w = FA.wave_i16(4000, 11) if wave == "int16" else FA.wave_float(4000, 12)
    spec = pk.frontend_default()
    assert (spec.kind, spec.num_mel_bins, spec.num_ceps, spec.window, spec.low_freq, spec.high_freq) == (0, 40, 0, 0, 20.0, 0.0)
    assert spec.dim == 40
    got = FA.frontend_any(w, spec, tables[FA.spec_id(FA.SPECS[0])])
    ref = O.Fbank().compute(w)
    assert got.shape == ref.shape and got.shape[0] > 0
    assert np.array_equal(bits(got), bits(ref))


# ------------------------------------------------------------------ the library's tables

@pytest.mark.parametrize("spec", FA.ALL_SPECS, ids=IDS)
def test_mel_tables_equal_the_independent_construction(spec, tables):
    t = tables[FA.spec_id(spec)]
    tri = FA.mel_triangles(spec)
    assert len(tri) == spec.num_mel_bins == len(t.mel_weights)
    assert int(np.sum(t.mel_len)) <= 512 and int(np.min(t.mel_len)) >= 1
    for b, (first, w) in enumerate(tri):
        assert int(t.mel_off[b]) == first and int(t.mel_len[b]) == w.size, b
        assert np.array_equal(bits(t.mel_weights[b]), bits(w)), b
        assert np.all(w > 0)


def test_eighty_bins_have_four_single_tap_triangles(tables):
    spec = FA.S(bins=80)
    assert int(np.sum(pk.frontend_tables(spec).mel_len == 1)) == 4
    assert sum(w.size == 1 for _, w in FA.mel_triangles(spec)) == 4


def ulp_distance(a, ref64):
    a, r = np.ascontiguousarray(a, np.float32), np.asarray(ref64, np.float64).astype(np.float32)
    return int(np.max(np.abs(a.view(np.int32).astype(np.int64) - r.view(np.int32).astype(np.int64)))) if a.size else 0


@pytest.mark.parametrize("spec", FA.ALL_SPECS, ids=IDS)
def test_window_dct_lifter_against_numpy_double(spec, tables):
    t = tables[FA.spec_id(spec)]
    a = np.float32(6.28318530718 / 399)                          # fbank.cc:249-256: the float angle step
    i = np.arange(400)
    if spec.window == 1:                                         # Povey: double throughout, one rounding
        assert ulp_distance(t.window, np.power(0.5 - 0.5 * np.cos(float(a) * i), 0.85)) <= 1
    else:
        # Hamming is the reference's expression: a FLOAT cosine of the float angle, then 0.54 - 0.46 c in double.  The
        # bits are pinned to the oracle above.  Against a double cosine the float cosine is off by at most one ulp of a
        # value below 1 (2^-24; the C library documents less than one ulp for cosf), which 0.46 scales, and the final
        # rounding adds half an ulp of the window value: with the smallest window value 0.08 that is up to four of ITS
        # ulps, so the bound is stated absolutely.
        angle = (a * i.astype(np.float32)).astype(np.float64)
        ref = 0.54 - 0.46 * np.cos(angle)
        assert np.all(np.abs(t.window.astype(np.float64) - ref) <= 0.46 * 2.0 ** -24 + 0.5 * np.spacing(t.window).astype(np.float64))
    B, K = spec.num_mel_bins, spec.num_ceps
    if spec.kind == 0:
        assert t.dct.size == 0 and t.lifter.size == 0
        return
    k, b = np.arange(K)[:, None], np.arange(B)[None, :]
    dct = np.sqrt(2.0 / B) * np.cos(np.pi / B * (b + 0.5) * k)
    dct[0] = np.sqrt(1.0 / B)
    assert t.dct.shape == (K, B) and ulp_distance(t.dct, dct) <= 1
    Q = float(spec.cepstral_lifter)
    lifter = 1.0 + 0.5 * Q * np.sin(np.pi * np.arange(K) / Q) if Q else np.ones(K)
    assert ulp_distance(t.lifter, lifter) <= 1
    if not Q:
        assert np.array_equal(bits(t.lifter), bits(np.ones(K, np.float32)))


@pytest.mark.parametrize("spec", FA.ALL_SPECS, ids=IDS)
def test_a_pairwise_sum_is_told_apart_on_the_tests_waves(spec, tables):
    """A kernel that tree-summed a bin's products must not pass: on the waves the GPU tests use, the variant of the
    restatement that adds pairwise differs from the sequential one."""
    t = tables[FA.spec_id(spec)]
    differing = 0
    for w in FA.waves().values():
        seq, pair = FA.frontend_any(w, spec, t), FA.frontend_any(w, spec, t, pairwise=True)
        differing += int(np.sum(bits(seq) != bits(pair)))
    assert differing > 0


# ------------------------------------------------------------------ refusals

def refused(spec, word):
    with pytest.raises(pk.PkCodeError) as e:
        spec.check()
    assert e.value.code == E_INVALID and word in str(e.value), str(e.value)
    with pytest.raises(pk.PkCodeError) as e2:
        spec.dim
    assert e2.value.code == E_INVALID
    with pytest.raises(pk.PkCodeError) as e3:
        pk.frontend_tables(spec)
    assert e3.value.code == E_INVALID
    with pytest.raises(pk.PkCodeError) as e4:                  # before any device call: also where there is no GPU
        pk.Frontend(spec).compute(np.zeros(800, np.float32))
    assert e4.value.code == E_INVALID and word in str(e4.value)


def test_refusals_name_the_field():
    S = FA.S
    refused(S(kind=2), "kind")
    refused(S(kind=-1), "kind")
    refused(S(window=2), "window")
    refused(S(bins=2), "num_mel_bins")
    refused(S(bins=129), "num_mel_bins")
    refused(S("mfcc", 23, 0), "num_ceps")
    refused(S("mfcc", 23, 24), "num_ceps")
    refused(S("fbank", 23, 5), "num_ceps")
    refused(S(low=-1.0), "low_freq")
    refused(S(low=float("nan")), "low_freq")
    refused(S(low=float("inf")), "low_freq")
    refused(S(high=float("nan")), "high_freq")
    refused(S(high=float("-inf")), "high_freq")
    refused(S("mfcc", 23, 13, lifter=-1.0), "cepstral_lifter")
    refused(S("mfcc", 23, 13, lifter=float("nan")), "cepstral_lifter")
    refused(S(high=8000.5), "high_freq")
    refused(S(low=4000.0, high=4000.0), "high_freq")
    refused(S(low=4000.0, high=-4000.0), "high_freq")
    refused(S(low=300.0, high=-7800.0), "high_freq")
    FA.S(lifter=-5.0).check()                                   # fbank ignores the lifter
    FA.S(high=8000.0).check()


@pytest.mark.parametrize("low", [20.0, 100.0, 200.0])
def test_empty_triangles_are_refused_where_the_restatement_finds_them(low):
    verdicts = {}
    for B in (80, 120, 126, 127, 128):
        spec = FA.S(bins=B, low=low)
        empty = FA.empty_bins(spec)
        verdicts[B] = not empty
        if empty:
            with pytest.raises(pk.PkCodeError) as e:
                spec.check()
            assert e.value.code == E_INVALID and "empty triangle" in str(e.value)
            assert re.search(r"mel bin %d\b" % empty[0], str(e.value)), str(e.value)
        else:
            spec.check()
            assert spec.dim == B
    assert verdicts[80] and verdicts[126]
    if low == 20.0:
        assert not verdicts[127] and not verdicts[128]
    else:
        assert verdicts[128]


# ------------------------------------------------------------------ interface

def test_new_names_in_header_map_and_exports():
    header = open(os.path.join(REPO, "include", "pk_mi355.h")).read()
    vmap = open(os.path.join(REPO, "pocketkaldi_amd", "csrc", "libpk_mi355.map")).read()
    L = pk.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pk.EXPORTS and hasattr(L, name), name
    assert "pk_mi355_*;" in vmap
    for word in ("pk_mi355_frontend_spec_t", "PK_MI355_FRONTEND_FBANK 0", "PK_MI355_FRONTEND_MFCC  1", "PK_MI355_WINDOW_HAMMING 0",
                 "PK_MI355_WINDOW_POVEY   1"):
        assert word in header, word
    assert C.sizeof(pk.pk_mi355_frontend_spec_t) == 28
    hpp = open(os.path.join(REPO, "include", "pocketkaldi_amd.hpp")).read()
    for word in ("struct FrontendSpec", "class Frontend", "const FrontendSpec &"):
        assert word in hpp, word


def test_null_arguments():
    L = pk.lib()
    st = FA.S(bins=23).struct()
    assert L.pk_mi355_frontend_check(None) == E_INVALID
    assert L.pk_mi355_frontend_dim(None) == E_INVALID
    assert L.pk_mi355_frontend_default(None) == E_INVALID
    assert L.pk_mi355_frontend_tables(None, None, None, None, None, None, None) == E_INVALID
    assert L.pk_mi355_frontend_tables(C.byref(st), None, None, None, None, None, None) == 0      # any pointer may be null
    wave, out = pk.pk_vector_t(0, None), pk.pk_matrix_t(0, 0, None)
    assert L.pk_mi355_frontend_compute(None, C.byref(wave), C.byref(out)) == E_INVALID
    assert L.pk_mi355_frontend_compute(C.byref(st), None, C.byref(out)) == E_INVALID
    assert L.pk_mi355_frontend_compute(C.byref(st), C.byref(wave), None) == E_INVALID
    g = np.zeros(24, np.float32)
    gp = g.ctypes.data_as(C.POINTER(C.c_float))
    assert L.pk_mi355_frontend_batch_create(None, C.byref(st), gp, 24, 1, 16000) is None
    assert L.pk_mi355_last_error_code() == E_STATE
    only_mel = np.zeros(512, np.float32)
    assert L.pk_mi355_frontend_tables(C.byref(st), None, None, None, only_mel.ctypes.data_as(C.POINTER(C.c_float)), None, None) == 0
    assert np.array_equal(only_mel[:int(np.sum(pk.frontend_tables(FA.S(bins=23)).mel_len))],
                          np.concatenate(pk.frontend_tables(FA.S(bins=23)).mel_weights))


def test_frontend_routing_in_python(monkeypatch):
    """BatchScorer(..., frontend=spec) goes to pk_mi355_frontend_batch_create with the spec and the statistics' length;
    without it, it is the old constructor with its old refusal."""
    calls = []

    class Fake:
        def __getattr__(self, name):
            def entry(*args):
                calls.append((name, args))
                return 1234 if name.endswith("create") else 0
            return entry

    class Am:
        handle = 77

    monkeypatch.setattr(pk, "lib", lambda: Fake())
    spec = FA.S(bins=80, window="povey")
    bs = pk.BatchScorer(Am(), np.zeros(81, np.float32), 3, 48000, frontend=spec)
    name, args = calls[0]
    assert name == "pk_mi355_frontend_batch_create" and args[0] == 77 and args[3:] == (81, 3, 48000)
    st = args[1]._obj
    assert (st.kind, st.num_mel_bins, st.num_ceps, st.window, st.low_freq, st.high_freq) == (0, 80, 0, 1, 20.0, 0.0)
    bs._h = None
    calls.clear()
    with pytest.raises(pk.PkError, match="41 entries"):
        pk.BatchScorer(Am(), np.zeros(81, np.float32), 3, 48000)
    assert not calls
    bs = pk.BatchScorer(Am(), np.zeros(41, np.float32), 3, 48000)
    assert calls[0][0] == "pk_mi355_batch_create"
    bs._h = None


def test_spec_defaults_in_python():
    s = pk.FrontendSpec()
    assert (s.kind, s.num_mel_bins, s.num_ceps, s.window, s.low_freq, s.high_freq, s.cepstral_lifter) == (0, 40, 0, 0, 20.0, 0.0, 22.0)
    assert s.dim == 40
    m = pk.FrontendSpec("mfcc", 23, 13, "povey")
    assert (m.kind, m.window, m.dim) == (1, 1, 13)
    assert pk.FrontendSpec(kind="mfcc").num_ceps == 13
