"""Writer of the reference's model-file formats (NNT0 / LAY0 / MAT0 / VEC0, as tool/convert_am.py:71-118 lays them
out, and the key = value model file pk_load reads): a (layers, prior, L, R, tid2pdf) model as files in a directory, so
that the reference's own readers, the oracle's and the product's can be put on the same bytes."""
import os
import struct

import numpy as np

KIND = {"linear": 0, "relu": 1, "normalize": 2, "softmax": 3}


def write_vec(f, v, dtype="<f4"):
    v = np.ascontiguousarray(v, dtype=dtype).ravel()
    f.write(b"VEC0" + struct.pack("<ii", v.size * 4 + 4, v.size) + v.tobytes())


def write_nnet(path, layers):
    with open(path, "wb") as f:
        f.write(b"NNT0" + struct.pack("<ii", 4, len(layers)))
        for l in layers:
            f.write(b"LAY0" + struct.pack("<ii", 4, KIND[l[0]]))
            if l[0] == "linear":
                W = np.ascontiguousarray(l[1], dtype="<f4")
                f.write(b"MAT0" + struct.pack("<iii", 8, W.shape[0], W.shape[1]))
                rows = np.empty((W.shape[0], W.shape[1] + 3), dtype="<u4")     # every row is a VEC0 of its own
                rows[:, :3] = np.frombuffer(b"VEC0" + struct.pack("<ii", W.shape[1] * 4 + 4, W.shape[1]), dtype="<u4")
                rows[:, 3:] = W.view("<u4")
                f.write(rows.tobytes())
                write_vec(f, l[2])


def write_model(dirpath, layers, prior, left, right, tid2pdf=None, cmvn_stats=None):
    """-> path of the .conf; files am.nnet, am.prior, tid2pdf.bin (and cmvn.bin) beside it."""
    d = str(dirpath)
    write_nnet(os.path.join(d, "am.nnet"), layers)
    with open(os.path.join(d, "am.prior"), "wb") as f:
        write_vec(f, prior)
    with open(os.path.join(d, "tid2pdf.bin"), "wb") as f:
        write_vec(f, np.zeros(1, np.int32) if tid2pdf is None else tid2pdf, "<i4")
    text = "nnet = am.nnet\nprior = am.prior\ntid2pdf = tid2pdf.bin\nleft_context = %d\nright_context = %d\nnum_pdfs = %d\n" % (
        left, right, len(prior))
    if cmvn_stats is not None:
        with open(os.path.join(d, "cmvn.bin"), "wb") as f:
            write_vec(f, cmvn_stats)
        text += "cmvn_stats = cmvn.bin\n"
    conf = os.path.join(d, "model.conf")
    with open(conf, "w") as f:
        f.write(text)
    return conf


def fuzz_seeds(n):
    """Seeds of a fuzz test: 0..n-1 by default; PK_FUZZ_SEEDS=count and PK_FUZZ_BASE=first seed widen and move the range."""
    base = int(os.environ.get("PK_FUZZ_BASE", "0"))
    return range(base, base + int(os.environ.get("PK_FUZZ_SEEDS", n)))


def random_stack(seed):
    """The layer stacks of test_fuzz_layer_stacks_bit_exact: random widths (multiples of nothing), depths, ReLU /
    Normalize in any position, optional softmax, random frame counts.  -> (layers, x[T][dims[0]], dims)"""
    rng = np.random.default_rng(4242 + seed)
    depth = int(rng.integers(1, 5))
    dims = [int(rng.integers(1, 700))] + [int(rng.integers(1, 500)) for _ in range(depth)]
    layers = []
    for i in range(depth):
        W = (rng.standard_normal((dims[i + 1], dims[i])) * np.sqrt(2.0 / dims[i])).astype(np.float32)
        layers.append(("linear", W, (rng.standard_normal(dims[i + 1]) * 0.1).astype(np.float32)))
        if rng.random() < 0.7:
            layers.append(("relu",))
        if rng.random() < 0.3:
            layers.append(("normalize",))
    if rng.random() < 0.5:
        layers.append(("softmax",))
    T = int(rng.choice([1, 2, 63, 64, 65, 127, 129, 300, 1100]))
    x = rng.standard_normal((T, dims[0])).astype(np.float32)
    return layers, x, dims


def load_ref_am_path():
    """tests/golden/ref_am_path.npz (outputs of the real reference, tests/golden/make_ref_fixtures.py) -> dict of arrays;
    float arrays are stored as their four byte planes."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_am_path.npz"))
    out = {}
    for k in z.files:
        v = z[k]
        if k.endswith("sha256"):
            out[k] = v
        else:
            out[k] = np.ascontiguousarray(np.moveaxis(v, 0, -1)).view("<f4")[..., 0]
    return out


def sha256_rows(a):
    """SHA-256 of a float matrix's bytes, as ref_am_path.npz stores it (uint8[32])."""
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, "<f4").tobytes()).digest(), dtype=np.uint8)


def overflow_model():
    """Softmax logits beyond 88.72 (expf overflows: inf / inf = NaN, the rest e / inf = 0 -> floor) and below -103.97.
    -> (layers, prior); context-free, 40 features.  The reference as built (assertions on) ABORTS on it at
    vector.cc:336; only its -DNDEBUG flavour may be given this model."""
    N = 200
    b = np.linspace(-120.0, 95.0, N).astype(np.float32)
    return [("linear", np.zeros((N, 40), np.float32), b), ("softmax",)], np.full(N, 1.0 / N, np.float32)
