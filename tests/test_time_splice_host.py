"""The time-splice layer, kind 9, without a GPU: the host rule against the numpy restatement of
tests/time_splice_cases.py bit for bit, every refusal that needs no device with its text, the right edge rule against the
wrong one on the GPU tests' inputs (every batch of tests/test_gpu_time_splice_limits.py included, with the places its sweep
of the pass boundary visits), and the model file through the reader."""
import ctypes as C
import struct

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import build as pk_build

import layer_cases as LC
import time_splice_cases as TC
from test_layer_kinds_host import E_DEVICE, E_INVALID, E_IO, Am, am_read, everything, fp, last_error, write_prior

i32p = C.POINTER(C.c_int32)
WIDTHS = [1, 7, 16, 17, 129]
OFFSETS = [[0], [-1, 0, 1], [-3, 3], [0, 2], [-2, 1], [-7, 2], [-32, 32]]


def ip(a):
    return a.ctypes.data_as(i32p)


def add_splice(a, in_dim, offsets):
    o = np.ascontiguousarray(offsets, np.int32)
    return a.L.pk_mi355_am_add_time_splice(a.h, in_dim, ip(o), o.shape[0])


def time_context(a):
    l, r = C.c_int(-1), C.c_int(-1)
    assert a.L.pk_mi355_am_time_context(a.h, C.byref(l), C.byref(r)) == 0
    return l.value, r.value


# ---------------------------------------------------------------- 1a. the rule

@pytest.mark.parametrize("offsets", OFFSETS, ids=lambda o: "o" + "_".join(str(v) for v in o))
@pytest.mark.parametrize("D", WIDTHS)
def test_rule_equals_the_restatement(D, offsets):
    lo, hi = TC.lo_hi(offsets)
    for T in (lo + hi + 1, lo + hi + 2, lo + hi + 67):
        x = everything(T, D, 5)
        got = pk.time_splice(x, offsets)
        want = TC.time_splice(x, offsets)
        assert got.dtype == np.float32 and got.shape == (T - lo - hi, len(offsets) * D)
        assert got.tobytes() == want.tobytes(), (D, offsets, T)          # a copy: NaN payloads and signed zeros too
    x = everything(67, D, 6)
    assert np.isnan(x).any() or D == 1
    for rows in (lo + hi, max(lo + hi - 1, 0)):
        with pytest.raises(pk.PkError, match="%d rows, the offsets consume %d on the left and %d on the right" % (rows, lo, hi)):
            pk.time_splice(np.zeros((rows, D), np.float32), offsets)


def test_rule_keeps_every_bit():
    bits = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000000, 0x00000001, 0x7F800000, 0xFF800000], np.uint32)
    x = np.resize(bits, 9 * 3).view(np.float32).reshape(9, 3)
    got = pk.time_splice(x, [-2, 0, 1])
    assert got.shape == (6, 9)
    for r in range(6):
        for c, o in enumerate((-2, 0, 1)):
            assert got[r, 3 * c:3 * c + 3].tobytes() == x[r + 2 + o].tobytes()


# ---------------------------------------------------------------- 1b. refusals and what the model records

def test_add_entry_refuses_with_its_text():
    with Am() as a:
        assert add_splice(a, 0, [0]) == E_INVALID and "in_dim 0" in last_error()
        assert add_splice(a, -3, [0]) == E_INVALID and "in_dim -3" in last_error()
        assert a.L.pk_mi355_am_add_time_splice(a.h, 4, None, 0) == E_INVALID and "0 offsets, between 1 and 16" in last_error()
        assert add_splice(a, 4, np.arange(17)) == E_INVALID and "17 offsets, between 1 and 16" in last_error()
        assert add_splice(a, 4, np.arange(16)) == 0
        assert add_splice(a, 4, [-1, 2, 1]) == E_INVALID and "offset 1 (index 2) follows 2" in last_error()
        assert add_splice(a, 4, [-1, -1, 1]) == E_INVALID and "offset -1 (index 1) follows -1" in last_error()
        assert add_splice(a, 4, [0, 33]) == E_INVALID and "offset 33 (index 1) is outside [-32, 32]" in last_error()
        assert add_splice(a, 4, [-33, 0]) == E_INVALID and "offset -33 (index 0) is outside [-32, 32]" in last_error()
        assert add_splice(a, 4, [-32, 32]) == 0
        assert a.L.pk_mi355_am_add_layer(a.h, pk.TIME_SPLICE) == E_INVALID and "unexpected layer type: 9" in last_error()


def test_finalize_refusals():
    with Am() as a:                                    # 4 x (32 + 32) + one frame more than 128
        a.linear(4, 2)
        for _ in range(2):
            assert add_splice(a, 2, [-32, 32]) == 0
            a.linear(4, 2)
        assert add_splice(a, 2, [0, 1]) == 0
        a.linear(4, 2)
        assert a.finalize(2) == E_INVALID, last_error()
        assert "consume 64 frames on the left and 65 on the right, at most 128 together" in last_error()
    with Am() as a:                                    # 128 are allowed
        a.linear(4, 2)
        for _ in range(2):
            assert add_splice(a, 2, [-32, 32]) == 0
            a.linear(4, 2)
        assert a.finalize(2) in (0, E_DEVICE), last_error()
        assert time_context(a) == (64, 64)
    with Am() as a:                                    # the running width
        a.linear(6, 8)
        assert add_splice(a, 7, [-1, 1]) == 0
        a.linear(14, 3)
        assert a.finalize(3) == E_INVALID
        assert "layer 1 (time splice) is 7 wide" in last_error() and "leave 8" in last_error()
    with Am() as a:                                    # the width behind it is n in_dim
        a.linear(6, 8)
        assert add_splice(a, 8, [-1, 0, 1]) == 0
        a.linear(16, 3)
        assert a.finalize(3) == E_INVALID and "16 after 24 (layer 2)" in last_error()
    with Am() as a:                                    # no Linear behind it
        a.linear(6, 8)
        assert a.L.pk_mi355_am_add_layer(a.h, pk.RELU) == 0
        assert add_splice(a, 8, [-1, 1]) == 0
        assert a.L.pk_mi355_am_add_layer(a.h, pk.SOFTMAX) == 0
        assert a.finalize(16) == E_INVALID and "layer 2 (time splice) has no linear layer behind it" in last_error()
    with Am() as a:                                    # the very first layer
        assert add_splice(a, 6, [-1, 1]) == 0
        a.linear(12, 3)
        assert a.finalize(3, left=1, right=1) == E_INVALID and "network must start with a linear layer when splicing" in last_error()
    for precision in (1, 2):                           # f16x3 and f16: the message they have
        with Am() as a:
            assert a.L.pk_mi355_am_set_precision(a.h, precision) == 0
            a.linear(8, 8)
            assert add_splice(a, 8, [-1, 1]) == 0
            a.linear(16, 8)
            assert a.finalize(8) == E_INVALID
            assert "f16x3 / f16 precision supports (Linear [ReLU] [Normalize])+ [Softmax] networks only" in last_error()


def test_python_refusals():
    W = np.zeros((8, 8), np.float32)
    lin = ("linear", W, np.zeros(8, np.float32))
    with pytest.raises(pk.PkError, match="network must start with a linear layer when splicing"):
        pk.AcousticModel([("splice", [-1, 1]), lin], prior=np.ones(8, np.float32))
    with pytest.raises(pk.PkError, match="has no linear layer behind it"):
        pk.AcousticModel([lin, ("splice", [-1, 1])], prior=np.ones(16, np.float32))
    with pytest.raises(pk.PkError, match="0 offsets"):
        pk.AcousticModel([lin, ("splice", []), lin], prior=np.ones(8, np.float32))
    with pytest.raises(pk.PkError, match="follows 1"):
        pk.AcousticModel([lin, ("splice", [1, 1]), lin], prior=np.ones(8, np.float32))
    for precision in ("f16x3", "f16"):
        with pytest.raises(pk.PkError, match=r"f16x3 / f16 precision supports \(Linear \[ReLU\] \[Normalize\]\)\+ \[Softmax\] networks only"):
            pk.AcousticModel([lin, ("splice", [0]), lin], prior=np.ones(8, np.float32), precision=precision)


def add_layers(a, layers):
    width = 0
    for l in layers:
        if l[0] == "linear":
            W, b = np.ascontiguousarray(l[1], np.float32), np.ascontiguousarray(l[2], np.float32)
            assert a.L.pk_mi355_am_add_linear(a.h, W.shape[1], W.shape[0], fp(W), fp(b)) == 0
            width = W.shape[0]
        elif l[0] in ("add", "mul"):
            assert a.vector(pk._LAYER_KIND[l[0]], l[1]) == 0
        elif l[0] == "pnorm":
            assert a.L.pk_mi355_am_add_pnorm(a.h, width, l[1]) == 0
            width = l[1]
        elif l[0] == "splice":
            assert add_splice(a, width, l[1]) == 0
            width *= len(l[1])
        else:
            assert a.L.pk_mi355_am_add_layer(a.h, pk._LAYER_KIND[l[0]]) == 0


def up(v, m):
    return (v + m - 1) // m * m


def blob_floats(layers, with_offsets=True):
    """The weight blob's layout, restated: per Linear W^T padded to [RoundUp(K, 16)][RoundUp(N, 128)] and the bias padded
    to RoundUp(N, 128); the log priors padded to 4; the add / mul vectors padded to 4 each; then the offsets of the
    time-splice layers padded to 4 words each."""
    n, dim = 0, 0
    for l in layers:
        if l[0] == "linear":
            N, K = l[1].shape
            n += up(K, 16) * up(N, 128) + up(N, 128)
            dim = N
        elif l[0] == "pnorm":
            dim = l[1]
        elif l[0] == "splice":
            dim *= len(l[1])
    n += up(dim, 4)
    n += sum(up(len(l[1]), 4) for l in layers if l[0] in ("add", "mul"))
    if with_offsets:
        n += sum(up(len(l[1]), 4) for l in layers if l[0] == "splice")
    return n


def test_what_the_model_records():
    layers, _ = TC.stack()
    with Am() as a:                                    # the two-splice stack of the GPU tests
        assert time_context(a) == (0, 0)
        add_layers(a, layers)
        assert a.finalize(TC.PDFS, TC.LEFT, TC.RIGHT) in (0, E_DEVICE), last_error()
        assert time_context(a) == (TC.LH, TC.RH) == TC.time_context(layers)
        assert a.L.pk_mi355_am_feat_dim(a.h) in (0, TC.FEAT_DIM)
        a.L.pk_mi355_am_blob_bytes.restype = C.c_size_t
        a.L.pk_mi355_am_blob_bytes.argtypes = [C.c_void_p]
        assert a.L.pk_mi355_am_blob_bytes(a.h) == 4 * blob_floats(layers) == 4 * (blob_floats(layers, False) + 8)
    old, _ = LC.stack()
    with Am() as a:                                    # a model of today: no context, the blob it had
        add_layers(a, old)
        assert a.finalize(LC.STACK_PDFS, LC.STACK_LEFT, LC.STACK_RIGHT) in (0, E_DEVICE), last_error()
        assert time_context(a) == (0, 0)
        # 24->40 and 17->12: 32 x 128 + 128 each; 10->34, 12->9 and 9->7: 16 x 128 + 128 each; 8 log priors; 8 + 8 for mul and add
        assert a.L.pk_mi355_am_blob_bytes(a.h) == 4 * blob_floats(old) == 4 * (2 * 4224 + 3 * 2176 + 8 + 16)
    assert pk_build.gemm_source_hash() == "9d0b7a273e7b9e1f"          # what tests/test_layer_kinds_host.py pins


# ---------------------------------------------------------------- 1c. the GPU tests can tell the edge rules apart

def test_right_and_wrong_edge_rule_differ():
    layers, prior = TC.stack()
    told = 0
    for f in TC.stack_feats():
        want = TC.loglik_time(layers, f, prior, TC.LEFT, TC.RIGHT, TC.SCALE)
        wrong = TC.loglik_wrong(layers, f, prior, TC.LEFT, TC.RIGHT, TC.SCALE)
        T = f.shape[0]
        assert want.shape == wrong.shape == (T, TC.PDFS) and np.isfinite(want).all()
        if T > TC.LH + TC.RH + 1:
            differ = (want != wrong).any(axis=1)
            assert differ[:TC.LH].all() and differ[T - TC.RH:].all() and not differ[TC.LH:T - TC.RH].any(), T
            told += 1
    assert told >= 3


def test_python_refusals_at_the_limits():
    """What tests/test_gpu_time_splice_limits.py runs at the limits, one step beyond them, through pk.AcousticModel."""
    lin = ("linear", np.zeros((8, 8), np.float32), np.zeros(8, np.float32))
    wide = ("linear", np.zeros((8, 16), np.float32), np.zeros(8, np.float32))
    with pytest.raises(pk.PkError, match="17 offsets, between 1 and 16"):
        pk.AcousticModel([lin, ("splice", list(range(17))), lin], prior=np.ones(8, np.float32))
    for bad, text in (([0, 33], r"offset 33 \(index 1\) is outside \[-32, 32\]"), ([-33, 0], r"offset -33 \(index 0\) is outside \[-32, 32\]")):
        with pytest.raises(pk.PkError, match=text):
            pk.AcousticModel([lin, ("splice", bad), wide], prior=np.ones(8, np.float32))
    deep = [lin] + [("splice", [-32, 32]), wide] * 2 + [("splice", [0, 1]), wide]
    with pytest.raises(pk.PkError, match="consume 64 frames on the left and 65 on the right, at most 128 together"):
        pk.AcousticModel(deep, prior=np.ones(8, np.float32))
    for precision in ("f16x3", "f16"):                 # any f16 precision, at the largest context too
        with pytest.raises(pk.PkError, match=r"f16x3 / f16 precision supports \(Linear \[ReLU\] \[Normalize\]\)\+ \[Softmax\] networks only"):
            pk.AcousticModel(deep[:5], prior=np.ones(8, np.float32), precision=precision)


# ---------------------------------------------------------------- 1c'. the cases of the limits, the pass edges and the audio path

@pytest.fixture(scope="module")
def limit_batches():
    return list(TC.limit_batches())


def test_limit_cases_tell_the_edge_rules_apart(limit_batches):
    """Every batch of tests/test_gpu_time_splice_limits.py: the right and the wrong rule differ in at least one of the
    first Lh and one of the last Rh rows of every utterance longer than the context; the finite cases are finite, and in
    the designed ones only the rows a non-finite frame reaches are NaN.  The "alone" form is the exception it has to be:
    an identity in front of one splice, no first-layer context -- there the two rules are the same function, and the
    case is about the copy."""
    told = {}
    for name, layers, prior, left, right, feats, designed in limit_batches:
        Lh, Rh = TC.time_context(layers)
        for f in feats:
            T = f.shape[0]
            want = TC.loglik_time(layers, f, prior, left, right, TC.SCALE)
            assert want.shape == (T, len(prior)), name
            if designed:
                allowed = TC.nan_rows_allowed(layers, f, left, right)
                nan = np.isnan(want).any(axis=1)
                assert not (nan & ~allowed).any() and np.isfinite(want[~nan]).all(), (name, T)
                assert T < max(TC.LIMIT_T) or (nan.any() and (~nan).any()), (name, T)      # the longest has rows of both kinds
            else:
                assert np.isfinite(want).all(), (name, T)
            if T == 0:
                continue
            same = TC.same_rows(want, TC.loglik_wrong(layers, f, prior, left, right, TC.SCALE))
            if name.startswith("alone"):
                assert same.all(), (name, T)
            elif T > Lh + Rh:
                assert not same[:Lh].all() and not same[T - Rh:].all(), (name, T)
                told[name] = told.get(name, 0) + 1
    assert all(name.startswith("alone") or told.get(name, 0) >= 1 for name, *_ in limit_batches), told


def test_the_sweep_visits_every_place_at_the_edge():
    """Position 256, the first of the second pass, lies in turn on every kind of row and of column between utterance 0's
    last frames and utterance 1's first, derived from the layout section 29 documents."""
    ctx = (TC.MS_LEFT, TC.MS_RIGHT, TC.MS_LH, TC.MS_RH)
    assert TC.time_context(TC.multisplice()[0]) == (TC.MS_LH, TC.MS_RH) == (11, 8)
    seen = [TC.place([T0] + TC.SWEEP_REST, *ctx, TC.PASS_ROWS) for T0 in TC.sweep_lengths(*ctx)]
    assert len(seen) == 33 and all(T0 + sum(TC.SWEEP_REST) < 600 for T0 in TC.sweep_lengths(*ctx))
    rows = [(u, r) for u, r, _ in seen]
    cols = [(u, c) for u, _, c in seen]
    assert rows.count((0, "frame")) == 4 and rows.count((0, "right virtual")) == 8 and rows.count((0, "no frame")) == 4      # (3 before the last, and it)
    assert rows.count((1, "left virtual")) == 11 and rows.count((1, "frame")) == 6
    assert cols.count((0, "frame")) == 6 and cols.count((0, "right copy")) == 10 and cols.count((1, "left copy")) == 13 and cols.count((1, "frame")) == 4
    # the ends of the batch: the last frame's row on the last / first row of a tile, from row 0 and from the last pass's first row
    pad = sum(ctx)
    origin = TC.PASS_ROWS - 12                         # HaloLeft = RoundUp(11, 4)
    for name, lengths in TC.end_batches(*ctx).items():
        last = lengths[0] + pad + TC.MS_LH + lengths[1] - 1
        assert last >= TC.PASS_ROWS, name
        assert TC.place(lengths, *ctx, last)[:2] == (1, "frame") and TC.place(lengths, *ctx, last + 1)[:2] == (1, "right virtual")
        at = (last - (origin if name.endswith("pass") else 0)) % TC.TILE
        assert at == (TC.TILE - 1 if name.startswith("last") else 0), (name, last)


# ---------------------------------------------------------------- 1d. the model file

def test_write_nnet_round_trips_through_the_reader(tmp_path):
    layers, _ = TC.stack()
    nnet, prior = tmp_path / "tdnn.nnet", tmp_path / "tdnn.prior"
    pk.write_nnet(str(nnet), layers)
    write_prior(prior, TC.PDFS)
    data = nnet.read_bytes()
    head = b"LAY0" + struct.pack("<ii", 4, pk.TIME_SPLICE)
    assert pk.TIME_SPLICE == 9 and data.count(head) == 2
    at = data.index(head)
    assert data[at + 12:at + 28] == struct.pack("<iiii", 10, 2, -1, 2)           # in_dim (what the p-norm leaves), n, the offsets
    at = data.index(head, at + 1)
    assert data[at + 12:at + 28] == struct.pack("<iiii", 34, 2, -3, 3)
    L = pk.lib()
    am = L.pk_mi355_am_create()
    try:
        rc = L.pk_mi355_am_read(am, str(nnet).encode(), str(prior).encode(), None, TC.LEFT, TC.RIGHT, TC.PDFS)
        assert rc in (0, E_DEVICE), last_error()                                 # read, assembled and chained
        l, r = C.c_int(), C.c_int()
        assert L.pk_mi355_am_time_context(am, C.byref(l), C.byref(r)) == 0 and (l.value, r.value) == (TC.LH, TC.RH)
    finally:
        L.pk_mi355_am_destroy(am)
    for cut in range(len(data) - 400, len(data)):                                # every proper prefix: the whole tail byte by byte,
        (tmp_path / "cut.nnet").write_bytes(data[:cut])
        rc, err = am_read(tmp_path / "cut.nnet", prior, TC.PDFS)
        assert rc == E_IO, (cut, rc, err)
    first = data.index(head)
    for cut in list(range(0, len(data) - 400, 97)) + list(range(first, first + 40)):   # ... the rest at a stride, and all of a kind-9 section
        (tmp_path / "cut.nnet").write_bytes(data[:cut])
        rc, err = am_read(tmp_path / "cut.nnet", prior, TC.PDFS)
        assert rc == E_IO, (cut, rc, err)


def one_layer_file(path, payload):
    path.write_bytes(b"NNT0" + struct.pack("<ii", 4, 1) + b"LAY0" + struct.pack("<ii", 4, 9) + payload)


def test_reader_refusals(tmp_path):
    prior = tmp_path / "p.prior"
    write_prior(prior, 4)
    p = tmp_path / "x.nnet"
    good = struct.pack("<iiii", 4, 2, -1, 1)
    for cut in range(len(good)):
        one_layer_file(p, good[:cut])
        assert am_read(p, prior, 4)[0] == E_IO, cut
    for bad, word in ((struct.pack("<iii", 0, 1, 0), "width 0"), (struct.pack("<ii", 4, 0), "0 offsets"), (struct.pack("<ii", 4, 17) + bytes(68), "17 offsets"),
                      (struct.pack("<iiii", 4, 2, 1, 1), "out of order"), (struct.pack("<iiii", 4, 2, 1, 0), "out of order"),
                      (struct.pack("<iii", 4, 1, 33), "out of range"), (struct.pack("<iii", 4, 1, -33), "out of range")):
        one_layer_file(p, bad)
        rc, err = am_read(p, prior, 4)
        assert rc == E_IO and word in err, (bad, err)
    one_layer_file(p, good)                            # the reader takes it; the model then refuses a network that starts with it
    rc, err = am_read(p, prior, 4)
    assert rc == E_INVALID and "network must start with a linear layer when splicing" in err
