"""The layer kinds 4 to 8 without a GPU: the host rule against the numpy restatement of
tests/layer_cases.py bit for bit, the model file of all nine kinds through the reader, every refusal with its text, and the
hash that ties the GEMM's profiles to its sources."""
import ctypes as C
import struct

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import build as pk_build

import layer_cases as LC

E_INVALID, E_DEVICE, E_IO = -1, -2, -3
WIDTHS = [1, 7, 16, 17, 129]
f32p = C.POINTER(C.c_float)


def fp(a):
    return a.ctypes.data_as(f32p)


def last_error():
    return pk.lib().pk_mi355_last_error().decode()


def everything(T, D, seed):
    """The designed rows with non-finite values all over them (no affine layer stands in front here)."""
    x = LC.designed(T, D, seed)
    flat = x.reshape(-1)
    if flat.shape[0] >= 16:
        flat[1::11] = np.resize(LC.NONFINITE, flat[1::11].shape[0])
    return x


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("kind", ["sigmoid", "tanh", "add", "mul"])
def test_elementwise_rule_equals_the_restatement(kind, D):
    for T in (1, 67):
        x = everything(T, D, 1)
        v = None
        if kind in ("add", "mul"):
            v = LC.designed(1, D, 2)[0]
        got = pk.apply_layer(kind, x, v)
        assert got.dtype == np.float32 and LC.same(got, LC.apply(kind, x, v)), (kind, D, T)
    if kind in ("sigmoid", "tanh"):          # the values themselves, so that both sides cannot be wrong together
        y = pk.apply_layer(kind, np.array([[0.0, 1.0, -1.0, np.inf, -np.inf, 104.0, -104.0]], np.float32))[0]
        want = [0.5, 0.7310586, 0.26894143, 1.0, 0.0, 1.0, 0.0] if kind == "sigmoid" else [0.0, 0.7615942, -0.7615942, 1.0, -1.0, 1.0, -1.0]
        # (float expf carries half an ulp into x = +-1: within an ulp of 0.5 .. 1 there; 0 and the saturated ends exactly)
        assert np.array_equal(y[[0, 3, 4, 5, 6]], np.array(want, np.float32)[[0, 3, 4, 5, 6]]) and np.abs(y - np.array(want, np.float32)).max() <= 6e-8
        assert np.isnan(pk.apply_layer(kind, np.array([[np.nan]], np.float32))[0, 0])


@pytest.mark.parametrize("G", [1, 2, 5, 10])
@pytest.mark.parametrize("O", WIDTHS)
def test_pnorm_rule_equals_the_restatement(O, G):
    for T in (1, 67):
        x = everything(T, O * G, 3)
        got = pk.apply_layer("pnorm", x, O)
        assert got.shape == (T, O) and LC.same(got, LC.pnorm(x, O)), (O, G, T)
    y = pk.apply_layer("pnorm", np.array([[3.0, 4.0, 0.0, -0.0, 2e19, 1.0, np.inf, 1.0]], np.float32), 4)[0]
    assert np.array_equal(y, np.array([5.0, 0.0, np.inf, np.inf], np.float32))     # an overflowed sum is inf: no rescaling fallback


def test_apply_layer_refusals():
    L = pk.lib()
    x = np.zeros((2, 6), np.float32)
    y = np.zeros((2, 6), np.float32)
    for kind in (0, 1, 2, 3, 9, -1):
        assert L.pk_mi355_layer_apply_host(kind, fp(x), 2, 6, None, 6, fp(y)) == E_INVALID
        assert "unexpected layer type: %d" % kind in last_error()
    assert L.pk_mi355_layer_apply_host(pk.PNORM, fp(x), 2, 6, None, 4, fp(y)) == E_INVALID
    assert "6" in last_error() and "4" in last_error() and "multiple" in last_error()
    assert L.pk_mi355_layer_apply_host(pk.SIGMOID, fp(x), 2, 6, None, 3, fp(y)) == E_INVALID
    assert L.pk_mi355_layer_apply_host(pk.MUL, fp(x), 2, 6, None, 6, fp(y)) == E_INVALID
    with pytest.raises(pk.PkError, match="5 entries"):
        pk.apply_layer("add", x, np.zeros(5, np.float32))


# ---------------------------------------------------------------- the model file

def all_nine(rng):
    W1, b1 = rng.standard_normal((12, 8)).astype(np.float32), rng.standard_normal(12).astype(np.float32)
    W2, b2 = rng.standard_normal((5, 4)).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    return [("linear", W1, b1), ("relu",), ("normalize",), ("pnorm", 4), ("sigmoid",), ("tanh",), ("mul", rng.standard_normal(4).astype(np.float32)),
            ("add", rng.standard_normal(4).astype(np.float32)), ("linear", W2, b2), ("softmax",)]


def write_prior(path, n):
    with open(path, "wb") as f:
        f.write(b"VEC0" + struct.pack("<ii", 4 * n + 4, n) + np.full(n, 1.0 / n, np.float32).tobytes())


def am_read(nnet, prior, num_pdfs):
    """pk_mi355_am_read, the entry the file tests load models through: the reader runs, the model is assembled and its
    dimension chain checked before the device is asked for, so without a GPU a well-formed file ends in
    PK_MI355_E_DEVICE and a malformed one in the reader's code."""
    L = pk.lib()
    am = L.pk_mi355_am_create()
    try:
        return L.pk_mi355_am_read(am, str(nnet).encode(), str(prior).encode(), None, 0, 0, num_pdfs), last_error()
    finally:
        L.pk_mi355_am_destroy(am)


def test_write_nnet_round_trips_through_the_reader(tmp_path):
    layers = all_nine(np.random.default_rng(5))
    nnet, prior = tmp_path / "nine.nnet", tmp_path / "nine.prior"
    pk.write_nnet(str(nnet), layers)
    write_prior(prior, 5)
    data = nnet.read_bytes()
    assert data[:12] == b"NNT0" + struct.pack("<ii", 4, 10)
    # the layer sections in the file, in order, with what follows each kind
    assert data.count(b"LAY0") == 10 and data.count(b"MAT0") == 2
    at = data.index(b"LAY0" + struct.pack("<ii", 4, pk.PNORM))
    assert data[at + 12:at + 20] == struct.pack("<ii", 12, 4)                    # in_dim: what the layers in front leave
    at = data.index(b"LAY0" + struct.pack("<ii", 4, pk.MUL))
    assert data[at + 12:at + 24] == b"VEC0" + struct.pack("<ii", 20, 4) and data[at + 24:at + 40] == layers[6][1].tobytes()
    rc, err = am_read(nnet, prior, 5)
    assert rc in (0, E_DEVICE), err                                              # read, assembled and chained
    write_prior(tmp_path / "six.prior", 6)
    rc, err = am_read(nnet, tmp_path / "six.prior", 6)
    assert rc == E_INVALID and "num_pdfs = 6 but the network outputs 5" in err
    # every proper prefix of the file is refused by the reader, never read as a shorter model
    for cut in list(range(0, len(data), 7)) + [len(data) - 1]:
        (tmp_path / "cut.nnet").write_bytes(data[:cut])
        rc, err = am_read(tmp_path / "cut.nnet", prior, 5)
        assert rc == E_IO, (cut, rc, err)


def one_layer_file(path, kind, payload):
    path.write_bytes(b"NNT0" + struct.pack("<ii", 4, 1) + b"LAY0" + struct.pack("<ii", 4, kind) + payload)


def test_reader_refusals(tmp_path):
    prior = tmp_path / "p.prior"
    write_prior(prior, 4)
    p = tmp_path / "x.nnet"
    vec4 = b"VEC0" + struct.pack("<ii", 20, 4) + np.ones(4, np.float32).tobytes()
    for kind in (9, 10, -1, 1 << 20):
        one_layer_file(p, kind, b"")
        rc, err = am_read(p, prior, 4)
        assert rc == E_IO and "read_layer: unexpected layer type: %d" % kind in err
    for kind in (pk.ADD, pk.MUL):
        one_layer_file(p, kind, vec4)
        assert am_read(p, prior, 4)[0] in (0, E_DEVICE)
        for bad in (b"", vec4[:8], vec4[:-3], b"VEC0" + struct.pack("<ii", 4, 0), b"VEC0" + struct.pack("<ii", 20, 5) + bytes(16)):
            one_layer_file(p, kind, bad)
            assert am_read(p, prior, 4)[0] == E_IO, (kind, bad)
    one_layer_file(p, pk.PNORM, struct.pack("<ii", 8, 4))
    assert am_read(p, prior, 4)[0] in (0, E_DEVICE)
    for bad in (b"", struct.pack("<i", 8), struct.pack("<ii", 8, 4)[:-1]):
        one_layer_file(p, pk.PNORM, bad)
        rc, err = am_read(p, prior, 4)
        assert rc == E_IO and "p-norm dimensions expected" in err
    for i, o in ((9, 4), (8, 0), (0, 4), (8, -4)):
        one_layer_file(p, pk.PNORM, struct.pack("<ii", i, o))
        rc, err = am_read(p, prior, 4)
        assert rc == E_IO and "input width %d is not a multiple of the output width %d" % (i, o) in err
    for kind in (pk.SIGMOID, pk.TANH):
        one_layer_file(p, kind, b"")
        assert am_read(p, prior, 4)[0] in (0, E_DEVICE)


# ---------------------------------------------------------------- the model's own refusals

class Am:
    def __enter__(self):
        self.L = pk.lib()
        self.h = self.L.pk_mi355_am_create()
        return self

    def __exit__(self, *a):
        self.L.pk_mi355_am_destroy(self.h)

    def linear(self, n_in, n_out):
        W, b = np.zeros((n_out, n_in), np.float32), np.zeros(n_out, np.float32)
        assert self.L.pk_mi355_am_add_linear(self.h, n_in, n_out, fp(W), fp(b)) == 0

    def vector(self, kind, v):
        v = np.ascontiguousarray(v, np.float32)
        return self.L.pk_mi355_am_add_vector_layer(self.h, kind, v.shape[0], fp(v))

    def finalize(self, num_pdfs, left=0, right=0):
        return self.L.pk_mi355_am_finalize(self.h, None, num_pdfs, left, right, None, 0)


def test_add_entries_refuse_with_their_text():
    with Am() as a:
        for kind in (pk.ADD, pk.MUL, pk.PNORM):                        # bare: they need their parameter
            assert a.L.pk_mi355_am_add_layer(a.h, kind) == E_INVALID and "unexpected layer type: %d" % kind in last_error()
        assert a.L.pk_mi355_am_add_layer(a.h, 9) == E_INVALID and "unexpected layer type: 9" in last_error()
        assert a.L.pk_mi355_am_add_layer(a.h, pk.SIGMOID) == 0 and a.L.pk_mi355_am_add_layer(a.h, pk.TANH) == 0
        assert a.vector(pk.SIGMOID, np.ones(3)) == E_INVALID and "unexpected layer type: 6" in last_error()
        assert a.L.pk_mi355_am_add_vector_layer(a.h, pk.ADD, 0, fp(np.ones(1, np.float32))) == E_INVALID and "dim 0" in last_error()
        assert a.L.pk_mi355_am_add_vector_layer(a.h, pk.ADD, 3, None) == E_INVALID
        for bad in (np.nan, np.inf, -np.inf):
            v = np.ones(9, np.float32)
            v[6] = bad
            assert a.vector(pk.MUL, v) == E_INVALID and "entry 6 is not finite" in last_error()
        assert a.vector(pk.MUL, np.ones(9)) == 0
        assert a.L.pk_mi355_am_add_pnorm(a.h, 8, 0) == E_INVALID and "8 -> 0" in last_error()
        assert a.L.pk_mi355_am_add_pnorm(a.h, 10, 4) == E_INVALID
        assert "input width 10 is not a multiple of the output width 4" in last_error()
        assert a.L.pk_mi355_am_add_pnorm(a.h, 9, 3) == 0


def test_finalize_walks_every_layer():
    with Am() as a:                                                    # a vector layer against the running width
        a.linear(6, 8)
        assert a.vector(pk.MUL, np.ones(7)) == 0
        assert a.finalize(8) == E_INVALID
        assert "layer 1" in last_error() and "7 wide" in last_error() and "leave 8" in last_error()
    with Am() as a:                                                    # a p-norm's input against the running width
        a.linear(6, 8)
        assert a.L.pk_mi355_am_add_layer(a.h, pk.TANH) == 0
        assert a.L.pk_mi355_am_add_pnorm(a.h, 10, 5) == 0
        assert a.finalize(5) == E_INVALID
        assert "layer 2" in last_error() and "10 wide" in last_error() and "leave 8" in last_error()
    with Am() as a:                                                    # the next Linear against what the p-norm leaves
        a.linear(6, 8)
        assert a.L.pk_mi355_am_add_pnorm(a.h, 8, 4) == 0
        a.linear(8, 3)
        assert a.finalize(3) == E_INVALID
        assert "layer 2" in last_error() and "8 after 4" in last_error()
    with Am() as a:                                                    # the output width is what the last layer leaves
        a.linear(6, 8)
        assert a.L.pk_mi355_am_add_pnorm(a.h, 8, 4) == 0
        assert a.finalize(8) == E_INVALID and "num_pdfs = 8 but the network outputs 4" in last_error()
        assert a.finalize(4, left=1, right=0) in (0, E_DEVICE), last_error()
    with Am() as a:                                                    # the new kinds are fp32 only
        assert a.L.pk_mi355_am_set_precision(a.h, 1) == 0
        a.linear(8, 8)
        assert a.L.pk_mi355_am_add_layer(a.h, pk.SIGMOID) == 0
        assert a.finalize(8) == E_INVALID
        assert "f16x3 / f16 precision supports (Linear [ReLU] [Normalize])+ [Softmax] networks only" in last_error()


def test_python_layer_lists():
    with pytest.raises(pk.PkError, match="states the width"):
        pk.AcousticModel([("pnorm", 4)], prior=np.ones(4, np.float32))
    with pytest.raises(pk.PkError, match="input width 8 is not a multiple of the output width 3"):
        pk.AcousticModel([("linear", np.zeros((8, 4), np.float32), np.zeros(8, np.float32)), ("pnorm", 3)], prior=np.ones(3, np.float32))
    with pytest.raises(pk.PkError, match="entry 1 is not finite"):
        pk.AcousticModel([("add", np.array([0.0, np.nan], np.float32))], prior=np.ones(2, np.float32))


def test_gemm_source_hash_is_the_parents():
    """The GEMM's sources and the headers it includes are untouched: the stored roofline counters still apply."""
    assert pk_build.gemm_source_hash() == "9d0b7a273e7b9e1f"          # at commit 265265c
