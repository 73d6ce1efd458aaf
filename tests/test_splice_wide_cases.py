"""The wide spliced-first-layer cases (tests/splice_wide_cases.py) without a GPU: every case really is what it says it
is -- its K, padded K, chunk count, padding rows, tile counts and the kernel variant those select, recomputed from the
launch rules -- every case's oracle output is finite, and for one small case of each group the oracle agrees with a
float64 restatement of AcousticModel::Compute to 1e-5 absolute (its own error against float64 is below 1e-6 at these
widths; tests/test_oracle_ref_am_wide.py pins it to the reference bit for bit)."""
import numpy as np
import pytest

from oracle import oracle as O

import splice_wide_cases as W


def oracle_rows(layers, prior, L, R, feats):
    out = O.Nnet(layers).am_compute(feats, prior, L, R, W.SCALE)
    assert out.shape == (feats.shape[0], prior.shape[0]) and np.isfinite(out).all()
    return out


# ------------------------------------------------------------------ the tables say what the rules give

def test_f32_cases_are_what_they_claim():
    want = [(128, 1, 2, 512, 512), (57, 4, 4, 513, 528), (43, 6, 5, 516, 528), (65, 4, 3, 520, 528), (79, 3, 3, 553, 560),
            (64, 4, 4, 576, 576), (80, 5, 5, 880, 880), (130, 5, 5, 1430, 1440), (130, 70, 3, 9620, 9632)]
    assert [(c["D"], c["L"], c["R"], c["K"], c["Kpad"]) for c in W.F32_CASES] == want
    for c in W.F32_CASES:
        d = W.derived(c["D"], c["L"], c["R"])
        assert {k: c[k] for k in d} == d, W.name(c)
        assert c["Kpad"] % W.SLAB_F32 == 0 and 0 <= c["pad"] < W.SLAB_F32
        assert c["big"] == (c["K"] < 9000), W.name(c)
    chunks = {W.name(c): c["chunks"] for c in W.F32_CASES}
    assert chunks == {"128-1-2": 1, "57-4-4": 2, "43-6-5": 2, "65-4-3": 2, "79-3-3": 2, "64-4-4": 2, "80-5-5": 2, "130-5-5": 3,
                      "130-70-3": 19}
    # the padding rule's threshold from both sides, and MULTICHUNK with and without it
    skip = {W.name(c): W.skip_last_half(c) for c in W.F32_CASES}
    assert skip == {"128-1-2": False, "57-4-4": True, "43-6-5": True, "65-4-3": True, "79-3-3": False, "64-4-4": False,
                    "80-5-5": False, "130-5-5": True, "130-70-3": True}
    assert W.by_shape(W.F32_CASES, (65, 4, 3))["pad"] == 8 and W.by_shape(W.F32_CASES, (79, 3, 3))["pad"] == 7
    # second chunk of 43-6-5: one slab; last chunk of 130-5-5: partial
    assert W.by_shape(W.F32_CASES, (43, 6, 5))["Kpad"] - W.CHUNK == W.SLAB_F32
    assert 0 < W.by_shape(W.F32_CASES, (130, 5, 5))["Kpad"] % W.CHUNK < W.CHUNK
    # K odd: rows 512 (real) and 513 (zero) share one two-row piece of the big-tile kernel
    assert W.by_shape(W.F32_CASES, (57, 4, 4))["K"] % 2 == 1
    # frames shorter than, and near, the context of 130-70-3
    assert [T < 74 for T in W.SMALL_T] == [True, True, False, False] and W.SMALL_T[2] < 2 * 74


def test_f32_routes():
    assert (W.SMALL_H, W.SMALL_T, W.BIG_H, W.BIG_T, W.N_PDFS) == (200, (1, 5, 130, 500), 1536, 4100, 60)
    for T in W.SMALL_T:
        assert W.decodable_passes(T, W.SMALL_H) == W.SMALL_PASSES[T]
    assert W.decodable_passes(W.BIG_T, W.BIG_H) == W.BIG_PASSES == [(4096, 384), (4, 12)]
    assert W.BIG_PASSES[0][1] == W.BIG_TILES                            # the smallest launch that takes big tiles
    assert W.decodable_passes(4096 - 128, W.BIG_H)[0][1] < W.BIG_TILES and W.decodable_passes(4096, 1408)[0][1] < W.BIG_TILES
    for c in W.F32_CASES:
        multi = c["chunks"] > 1
        for T in W.SMALL_T:
            for _, tiles in W.SMALL_PASSES[T]:
                assert W.variant(c["Kpad"], tiles) == (1, multi, 3), (W.name(c), T)
        if c["big"]:
            assert [W.variant(c["Kpad"], t) for _, t in W.BIG_PASSES] == [(2, multi, 3 if multi else 2), (1, multi, 3)], W.name(c)
    # GemmKernel<1, SPLICE, MULTICHUNK> and GemmKernel<2, SPLICE, MULTICHUNK> are both reached, and so are their
    # single-chunk twins
    reached = {W.variant(c["Kpad"], t) for c in W.F32_CASES if c["big"] for _, t in W.BIG_PASSES}
    assert reached == {(2, True, 3), (1, True, 3), (2, False, 2), (1, False, 3)}


def test_scorer_layout():
    assert W.SCORER_FRAMES == (4093, 0, 1, 3, 130, 7)
    assert sum(W.round_up(T, 4) for T in W.SCORER_FRAMES) == W.SCORER_COMPACT_ROWS == 4244
    for c in W.F32_CASES:
        if not c["big"]:
            continue
        assert c["L"] + c["R"] >= 3                                     # (compact rows exist from three context frames on)
        rows = W.scorer_rows(W.SCORER_FRAMES, c["L"], c["R"])
        assert rows == W.SCORER_COMPACT_ROWS - 1 and W.round_up(rows, W.TILE) == 34 * W.TILE
        assert W.scorer_tiles(W.SCORER_FRAMES, c["L"], c["R"], W.BIG_H) == W.SCORER_TILES == 34 * 12 == 408
        assert W.variant(c["Kpad"], W.SCORER_TILES)[0] == 2
        # the column shift an utterance leaves behind: its T + L + R columns against its rows rounded up to four.  Behind
        # utterance 0 it is non-zero (L + R = 3: behind the three-frame utterance), and it never goes negative
        left = [T + c["L"] + c["R"] - W.round_up(T, 4) for T in W.SCORER_FRAMES if T]
        assert min(left) >= 0 and sum(left[:-1]) > 0 and (left[0] > 0 or c["L"] + c["R"] == 3), W.name(c)
    for shape in W.SCORER_PADDED_LAYOUT:                                # row = column: more rows, the same 34 row tiles
        c = W.by_shape(W.F32_CASES, shape)
        rows = W.scorer_rows(W.SCORER_FRAMES, c["L"], c["R"], compact=False)
        assert rows == sum(T + c["L"] + c["R"] for T in W.SCORER_FRAMES[:-1] if T) + W.SCORER_FRAMES[-1]
        assert W.scorer_tiles(W.SCORER_FRAMES, c["L"], c["R"], W.BIG_H, compact=False) == W.SCORER_TILES
    assert W.SCORER_PADDED_LAYOUT == ((80, 5, 5), (43, 6, 5), (57, 4, 4)) and W.SCORER_STABLE in W.SCORER_PADDED_LAYOUT


def test_ring_cases():
    assert [(c["D"], c["L"], c["R"], c["K"]) for c in W.RING_CASES] == [(40, 5, 5, 440), (31, 1, 1, 93)]
    assert sorted(W.RING_VALUES) == ["2", "3"]
    for c in W.RING_CASES:
        d = W.derived(c["D"], c["L"], c["R"])
        assert {k: c[k] for k in d} == d and c["chunks"] == 1
        tiles = W.BIG_PASSES[0][1]
        assert W.variant(c["Kpad"], tiles, ring=3) == (2, False, 3) and W.variant(c["Kpad"], tiles, ring=2) == (2, False, 2)
    assert W.RING_CASES[1]["K"] % 2 == 1 and W.skip_last_half(W.RING_CASES[0]) and not W.skip_last_half(W.RING_CASES[1])


def test_f16_cases():
    want = [(88, 1, 1, 264, 288, 24), (80, 5, 5, 880, 896, 16), (128, 2, 2, 640, 640, 0), (136, 5, 5, 1496, 1504, 8)]
    assert [(c["D"], c["L"], c["R"], c["K"], c["Kpad"], c["pad"]) for c in W.F16_CASES] == want
    for c in W.F16_CASES:
        d = W.derived(c["D"], c["L"], c["R"], slab=W.SLAB_F16)
        assert (c["K"], c["Kpad"], c["pad"]) == (d["K"], d["Kpad"], d["pad"])
        assert c["D"] % 8 == 0                                          # the interleaved (hi, lo) row exists for such D only
    # the largest overhang a multiple-of-8 dimension can have: K = 8 (mod 32)
    assert W.F16_CASES[0]["pad"] == 24 == max((-8 * m) % 32 for m in range(1, 64))
    assert (W.F16_CASES[0]["D"], W.F16_CASES[0]["L"], W.F16_CASES[0]["R"]) == W.F16_OVERHANG
    assert (W.F16_SMALL_H, W.F16_SMALL_FRAMES, W.F16_BIG_H, W.F16_BIG_FRAMES) == (300, (1, 257, 700), 1536, (4500,))


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_cases_stay_inside_the_stated_ranges(seed):
    D, L, R, H, N, T, normalize = W.fuzz_case(seed)
    assert 49 <= D <= 160 and 0 <= L <= 7 and 0 <= R <= 7 and D * (L + R + 1) > 512
    assert H in (137, 1536) and T in ((2, 131, 4096, 4097) if H == 1536 else (1, 64, 500))
    assert W.fuzz_case(seed) == (D, L, R, H, N, T, normalize)
    layers, prior = W.net(D, L, R, H, N, normalize)
    assert [l[0] for l in layers].count("normalize") == int(normalize)
    oracle_rows(layers, prior, L, R, W.features(D, L, R, T, seed))


# ------------------------------------------------------------------ every case's oracle output is finite

@pytest.mark.parametrize("c", W.F32_CASES, ids=W.name)
def test_f32_oracle_outputs_are_finite(c):
    layers, prior = W.net(c["D"], c["L"], c["R"], W.SMALL_H)
    for T in W.SMALL_T:
        oracle_rows(layers, prior, c["L"], c["R"], W.features(c["D"], c["L"], c["R"], T))
    if c["big"]:
        layers, prior = W.net(c["D"], c["L"], c["R"], W.BIG_H)
        oracle_rows(layers, prior, c["L"], c["R"], W.features(c["D"], c["L"], c["R"], W.BIG_T))
        for f in W.scorer_features(c, W.SCORER_FRAMES):
            if f.shape[0]:
                oracle_rows(layers, prior, c["L"], c["R"], f)


@pytest.mark.parametrize("c", W.RING_CASES, ids=W.name)
def test_ring_oracle_outputs_are_finite(c):
    layers, prior = W.net(c["D"], c["L"], c["R"], W.BIG_H)
    oracle_rows(layers, prior, c["L"], c["R"], W.features(c["D"], c["L"], c["R"], W.BIG_T))


@pytest.mark.parametrize("c", W.F16_CASES, ids=W.name)
def test_f16_oracle_outputs_are_finite(c):
    for H, frames in ((W.F16_SMALL_H, W.F16_SMALL_FRAMES), (W.F16_BIG_H, W.F16_BIG_FRAMES)):
        layers, prior = W.net(c["D"], c["L"], c["R"], H)
        for f in W.scorer_features(c, frames):
            oracle_rows(layers, prior, c["L"], c["R"], f)


# ------------------------------------------------------------------ chunk faults move bits at these shapes

def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("c", [c for c in W.F32_CASES if c["big"] and c["chunks"] > 1], ids=W.name)
def test_wrong_chunking_changes_bits_of_the_first_layer(c):
    """On the model, never on a kernel: the first layer's products as the reference chains them (one FMA chain per
    512-chunk, chunks added in order: pko_sgemm_naive, which the blocked oracle equals bit for bit), against the chains
    a wrong kernel would build -- no restart at the chunk boundary's proper place (every boundary one slab late), and,
    where there are three chunks, the chunks added in another order.  Both differ in bits on these very inputs, so the
    bit comparison of test_gpu_splice_wide.py would notice either."""
    D, L, R, K = c["D"], c["L"], c["R"], c["K"]
    layers, _ = W.net(D, L, R, W.SMALL_H)
    A = O.splice(W.features(D, L, R, 130), L, R)
    B = np.ascontiguousarray(layers[0][1].T)
    right = O.sgemm_naive(A, B)
    assert np.array_equal(bits(right), bits(O.sgemm(A, B)))
    late = O.sgemm_naive(np.hstack([np.zeros((A.shape[0], W.SLAB_F32), np.float32), A]), np.vstack([np.zeros((W.SLAB_F32, B.shape[1]), np.float32), B]))
    assert (bits(late) != bits(right)).mean() > 0.05
    parts = [O.sgemm_naive(A[:, k0:k0 + W.CHUNK], B[k0:k0 + W.CHUNK]) for k0 in range(0, K, W.CHUNK)]
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    assert np.array_equal(bits(total), bits(right))                     # chunks are added in order, one float add each
    if len(parts) == 3:
        assert (bits(parts[0] + (parts[1] + parts[2])) != bits(right)).mean() > 0.05


# ------------------------------------------------------------------ NaN frames: what a padding row must not fetch

@pytest.mark.parametrize("c", [c for c in W.F32_CASES if c["pad"] and c["big"]], ids=W.name)
def test_nan_frames_spoil_their_context_and_no_other_row(c):
    """The oracle (and the reference: am.cc:65-88 splices L + R + 1 frames, nothing else) turns exactly the rows
    t - R .. t + L of a NaN frame t into NaN.  A first layer whose padding rows k >= K fetched feature k - K of the frame
    behind the context -- restated here as a net of context R + 1 whose extra weights are zero -- spoils row t - R - 1 as
    well, so the comparison of test_gpu_splice_wide.py tells the two apart, which it could not on finite features."""
    D, L, R, K, pad = c["D"], c["L"], c["R"], c["K"], c["pad"]
    assert 0 < pad <= D
    for T in W.NAN_FRAMES if c["big"] else [130]:
        layers, prior = W.net(D, L, R, W.SMALL_H)                      # (the rows that are NaN do not depend on the width)
        feats = W.nan_features(c, T)
        assert sorted(np.flatnonzero(np.isnan(feats).any(axis=1))) == sorted(W.NAN_FRAMES[T])
        assert set(np.flatnonzero(np.isnan(feats).any(axis=0))) == {0, pad - 1}
        got = O.Nnet(layers).am_compute(feats, prior, L, R, W.SCALE)
        want = W.nan_rows(c, T)
        assert np.array_equal(np.isnan(got).all(axis=1), want) and not np.isnan(got[~want]).any()
        assert 0 < want.sum() < T
        wide = np.zeros((W.SMALL_H, K + D), np.float32)
        wide[:, :K] = layers[0][1]
        faulty = O.Nnet([("linear", wide, layers[0][2])] + layers[1:]).am_compute(feats, prior, L, R + 1, W.SCALE)
        spoiled = np.isnan(faulty).any(axis=1)
        assert spoiled[want].all() and (spoiled & ~want).sum() >= 1
        assert not W.same_bits_and_nans(faulty, got) and W.same_bits_and_nans(got, got.copy())
        for t in W.NAN_FRAMES[T]:
            if t - R - 1 >= 0 and not want[t - R - 1]:
                assert spoiled[t - R - 1], (W.name(c), T, t)


# ------------------------------------------------------------------ the oracle against float64, one small case a group

def check_restated(D, L, R, H, T, N=W.N_PDFS, normalize=False):
    layers, prior = W.net(D, L, R, H, N, normalize)
    feats = W.features(D, L, R, T)
    got = oracle_rows(layers, prior, L, R, feats)
    want = W.restated(layers, prior, L, R, feats)
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    assert err <= 1e-5, "D %d L %d R %d H %d T %d: oracle against float64 %.3e" % (D, L, R, H, T, err)
    return want


def test_oracle_against_float64_restatement():
    c = W.by_shape(W.F32_CASES, (57, 4, 4))
    for T in W.SMALL_T[:3]:                                 # small tiles; T = 1 and 5: nothing but replicated edge frames
        check_restated(c["D"], c["L"], c["R"], W.SMALL_H, T)
    check_restated(130, 70, 3, W.SMALL_H, 5)                # 19 chunks, T far below the context
    check_restated(c["D"], c["L"], c["R"], W.BIG_H, 5)      # the big-tile group's net
    r = W.RING_CASES[1]
    check_restated(r["D"], r["L"], r["R"], W.BIG_H, 5)
    f = W.F16_CASES[0]
    check_restated(f["D"], f["L"], f["R"], W.F16_SMALL_H, 257)
    for seed in range(64):                                  # the fuzz group: the first seed with a Normalize layer
        D, L, R, H, N, T, normalize = W.fuzz_case(seed)
        if normalize:
            check_restated(D, L, R, H, min(T, 64), N, normalize)
            break
    else:
        raise AssertionError("no fuzz seed below 64 draws a Normalize layer")


def test_restatement_notices_a_wrong_splice():
    """The float64 restatement is no rubber stamp: a context shifted by one frame, the chunks' worth of k dropped, or
    the frame behind the context in place of a padding row's zero would all move the rows by far more than 1e-5."""
    c = W.by_shape(W.F32_CASES, (57, 4, 4))
    layers, prior = W.net(c["D"], c["L"], c["R"], W.SMALL_H)
    feats = W.features(c["D"], c["L"], c["R"], 130)
    want = W.restated(layers, prior, c["L"], c["R"], feats)
    assert np.max(np.abs(W.restated(layers, prior, c["L"] + 1, c["R"] - 1, feats) - want)) > 1e-2
    cut = [("linear", np.where(np.arange(c["K"]) < W.CHUNK, layers[0][1], 0).astype(np.float32), layers[0][2])] + layers[1:]
    assert np.max(np.abs(W.restated(cut, prior, c["L"], c["R"], feats) - want)) > 1e-5
    assert W.first_difference(want.astype(np.float32), want.astype(np.float32)) is None
    moved = want.astype(np.float32).copy()
    moved[7, 3] = np.nextafter(moved[7, 3], np.float32(np.inf))
    assert W.first_difference(moved, want.astype(np.float32)) == (7, 3)
