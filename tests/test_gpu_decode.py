"""The GPU decoder (pk_mi355_decoder_*: kernels in csrc/decode.hip, host object in csrc/capi_decoder.hip): words and
weight against the reference's own decoder (oracle/_ref/libpkref_decoder.so, where built), an exhaustive Viterbi and a host model of the
documented semantics (tests/decoder_model.py); every best path re-scored on the host."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth_graph as SG

import decoder_model as M
from test_gpu_decoder import DECLIB, G, decoder_lib, host_decodable, read_fst, viterbi

pytestmark = pytest.mark.gpu
HAVE_REF = os.path.exists(DECLIB)


def flat_arcs(path):
    import struct
    raw = open(path, "rb").read()
    ns, na = struct.unpack("<ii", raw[36:44])
    return [struct.unpack("<iiif", raw[48 + 8 * ns + 16 * i: 64 + 8 * ns + 16 * i]) for i in range(na)]


def ref_decode(fst_path, ll, am_handle):
    """pkref_decode: (words, weight, ok)."""
    d = host_decodable(np.ascontiguousarray(ll, np.float32), am_handle)
    words = (C.c_int * 4096)()
    weight, ok = C.c_float(0), C.c_int(0)
    n = decoder_lib().pkref_decode(fst_path.encode(), C.byref(d), words, 4096, C.byref(weight), C.byref(ok))
    assert n >= 0
    return list(words[:n]), weight.value, ok.value


def ref_decode_many(fst_path, lls, am_handle):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda ll: ref_decode(fst_path, ll, am_handle), lls))


def ident_model(num_pdfs):
    W = np.zeros((num_pdfs, 4), np.float32)
    return pk.AcousticModel([("linear", W, np.zeros(num_pdfs, np.float32))], prior=np.full(num_pdfs, 1.0 / num_pdfs, np.float32))


def check_self(dec, u, fst_path, ll, pdf_of, final, start, arcs=None):
    """Best path re-scored on the host: same weight bitwise, T emitting arcs, its olabels are the words."""
    words, weight, ok = dec.result(u)
    if not ok:
        return
    arcs = arcs or flat_arcs(fst_path)
    path = dec.best_path_arcs(u)
    if not path:                       # no final token: BestPath's empty hypothesis (or T = 0 at a non-final start)
        assert words == [] and weight == 0.0
        return
    c, t, pw = M.f32(0), 0, []
    for a in path:
        nxt, il, ol, w = arcs[a]
        if il:
            c = M.f32(M.f32(c + M.f32(w)) + M.f32(-ll[t, pdf_of(il)]))
            t += 1
        else:
            c = M.f32(c + M.f32(w))
        if ol:
            pw.append(ol)
    end = arcs[path[-1]][0]
    wt = M.f32(M.f64(c) + M.f64(final[end]))
    wt = M.f32(wt + M.f32(final[end]))
    assert t == ll.shape[0] and pw == words
    assert np.float32(weight).tobytes() == wt.tobytes(), (weight, float(wt))


def write_graph(tmp_path, name, g):
    p = str(tmp_path / name)
    SG.write_fst(p, g["start"], g["final"], g["arcs"])
    return p


# ---------------------------------------------------------------- 1. testinput.fst

def test_testinput_random_logliks():
    path = os.path.join(G, "testinput.fst")
    fst = read_fst(path)
    am = ident_model(4)
    dec = pk.Decoder(pk.Fst(path), am, 8)
    lls = [(np.random.default_rng(seed).standard_normal((2, 4)) * 2).astype(np.float32) for seed in range(8)]
    dec.decode(lls)
    for u, ll in enumerate(lls):
        words, weight, ok = dec.result(u)
        cost, want, _ = viterbi(fst, ll, lambda t: t)
        assert ok == 1 and words == want
        assert abs(weight - (cost + 3.5)) < 1e-5 * max(1, abs(weight))   # BestPath counts final() twice
        ex = M.viterbi32((fst[0], fst[1], fst[2]), ll, lambda t: t)        # the same search in float: bitwise
        assert (words, np.float32(weight).tobytes()) == (ex["words"], np.float32(ex["weight"]).tobytes())
        if HAVE_REF:
            rw, rweight, rok = ref_decode(path, ll, am.handle)
            assert (words, np.float32(weight).tobytes(), ok) == (rw, np.float32(rweight).tobytes(), rok)
        check_self(dec, u, path, ll, lambda t: t, fst[1], fst[0])


# ---------------------------------------------------------------- 2. refmodel + wordloop.fst through decode_batch

@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/libpkref_decoder.so not built")
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("softmax", ["reference", "stable"])
def test_refmodel_decode_batch(precision, softmax):
    from refmodel_text import DIR, load_text_model
    layers, prior, Lc, Rc, tid2pdf, cmvn41 = load_text_model()
    fst_path = os.path.join(DIR, "wordloop.fst")
    waves = [pk.read_wav(os.path.join(G, w)) for w in ("en-us-hello.wav", "en-us-cat.wav")]
    am = pk.AcousticModel(layers, prior, Lc, Rc, tid2pdf, precision=precision)
    am.set_softmax(softmax)
    bs = pk.BatchScorer(am, cmvn41, 2, sum(len(w) for w in waves))
    bs.set_waves(waves)
    if precision != "f32":
        bs.calibrate()
    bs.score(0.1, sync=False)
    dec = pk.Decoder(pk.Fst(fst_path), am, 2)
    dec.decode_batch(bs, sync=False)
    dec.synchronize()
    views = bs.fetch_all()
    arcs = flat_arcs(fst_path)
    fst = read_fst(fst_path)
    for u, v in enumerate(views):
        words, weight, ok = dec.result(u)
        ll = v.log_prob()
        rw, rweight, rok = ref_decode(fst_path, ll, am.handle)
        assert ok == rok == 1 and words == rw and len(words) >= 1
        assert np.float32(weight).tobytes() == np.float32(rweight).tobytes()
        assert dec.active_bound(u) < 30000
        check_self(dec, u, fst_path, ll, lambda t: int(tid2pdf[t]), fst[1], fst[0], arcs)


# ---------------------------------------------------------------- 3. synthetic graphs, three sizes

@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/libpkref_decoder.so not built")
@pytest.mark.parametrize("states,utts,frames", [(2000, 64, 100), (20000, 32, 300), (200000, 16, 1000)])
def test_synthetic_against_reference(tmp_path, states, utts, frames):
    g = SG.size_for_states(states, seed=states)
    path = write_graph(tmp_path, "g.fst", g)
    n = g["num_tids"]
    am = ident_model(n)
    lls = [SG.planted(g, frames + 37 * u % frames, seed=u)[0] for u in range(utts)]
    dec = pk.Decoder(pk.Fst(path), am, utts)
    dec.decode(lls)
    refs = ref_decode_many(path, lls, am.handle)
    arcs = flat_arcs(path)
    for u, ll in enumerate(lls):
        words, weight, ok = dec.result(u)
        assert dec.active_bound(u) < 30000
        assert (words, np.float32(weight).tobytes(), ok) == (refs[u][0], np.float32(refs[u][1]).tobytes(), refs[u][2]), u
        check_self(dec, u, path, ll, lambda t: t, g["final"], 0, arcs)



# ---------------------------------------------------------------- 4. max-active binds: the host model of the semantics

def test_max_active_binding_matches_model(tmp_path):
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    path = write_graph(tmp_path, "g.fst", g)
    n = g["num_tids"]
    am = ident_model(n)
    lls = [SG.flat(40, n, seed=s) for s in range(4)]
    dec = pk.Decoder(pk.Fst(path), am, 4)
    dec.set_beam(16.0, 256)
    dec.decode(lls)
    arcs = flat_arcs(path)
    by_state, k = [], 0
    for st in g["arcs"]:
        by_state.append([a + (k + i,) for i, a in enumerate(st)])
        k += len(st)
    for u, ll in enumerate(lls):
        want = M.decode((0, g["final"], by_state), ll, lambda t: t, beam=16.0, max_active=256)
        words, weight, ok = dec.result(u)
        assert want["active_bound"] > 256                       # it did bind
        assert (words, np.float32(weight).tobytes(), ok) == (want["words"], np.float32(want["weight"]).tobytes(), want["ok"])
        assert dec.best_path_arcs(u) == want["path"]
        assert dec.active_bound(u) == want["active_bound"]
        check_self(dec, u, path, ll, lambda t: t, g["final"], 0, arcs)


# ---------------------------------------------------------------- 6. negative epsilon weights, no negative cycle

def test_negative_epsilon_weights_match_viterbi(tmp_path):
    arcs = [[(1, 1, 1, 0.5), (2, 2, 2, 1.0)], [(2, 0, 0, -0.75), (3, 3, 3, 0.25)], [(3, 0, 4, -0.5), (2, 3, 0, 0.3)],
            [(0, 0, 0, -0.25), (3, 1, 0, 0.1)]]
    final = np.array([np.inf, np.inf, 1.0, 0.5], np.float32)
    path = str(tmp_path / "neg.fst")
    SG.write_fst(path, 0, final, arcs)
    fst = read_fst(path)
    am = ident_model(4)
    lls = [(np.random.default_rng(s).standard_normal((5, 4))).astype(np.float32) for s in range(6)]
    dec = pk.Decoder(pk.Fst(path), am, 6)
    dec.decode(lls)
    for u, ll in enumerate(lls):
        words, weight, ok = dec.result(u)
        cost, want, _ = viterbi(fst, ll, lambda t: t)
        assert ok == 1 and words == want
        check_self(dec, u, path, ll, lambda t: t, final, 0)


# ---------------------------------------------------------------- 7. edge cases

def test_zero_and_one_frame():
    path = os.path.join(G, "testinput.fst")
    am = ident_model(4)
    dec = pk.Decoder(pk.Fst(path), am, 2)
    lls = [np.zeros((0, 4), np.float32), np.array([[0.5, -1.0, 0.25, 2.0]], np.float32)]
    dec.decode(lls)
    assert dec.result(0) == ([], 0.0, 1)                         # start closure alone: no final state
    if HAVE_REF:
        for u, ll in enumerate(lls):
            rw, rweight, rok = ref_decode(path, ll, am.handle)
            words, weight, ok = dec.result(u)
            assert (words, np.float32(weight).tobytes(), ok) == (rw, np.float32(rweight).tobytes(), rok)


def test_dead_end_empties_the_beam(tmp_path):
    path = str(tmp_path / "dead.fst")
    SG.write_fst(path, 0, np.array([np.inf, 0.0], np.float32), [[(1, 1, 7, 0.5)], []])
    dec = pk.Decoder(pk.Fst(path), ident_model(4), 2)
    dec.decode([np.zeros((4, 4), np.float32), np.zeros((1, 4), np.float32)])
    assert dec.result(0) == ([], 0.0, 0)
    words, weight, ok = dec.result(1)
    assert ok == 1 and words == [7]


def test_negative_epsilon_cycle_is_rejected(tmp_path):
    path = str(tmp_path / "cycle.fst")
    SG.write_fst(path, 0, np.array([0.0, 0.0], np.float32), [[(1, 0, 0, -1.0), (0, 1, 0, 0.5)], [(0, 0, 0, -1.0)]])
    dec = pk.Decoder(pk.Fst(path), ident_model(4), 1)
    with pytest.raises(pk.PkError) as e:
        dec.decode([np.zeros((3, 4), np.float32)])
    assert e.value.code == -1 and "negative epsilon cycle" in str(e.value)


def test_trace_capacity_exhausted_then_fresh_decoder(tmp_path):
    g = SG.size_for_states(2000, seed=3)
    path = write_graph(tmp_path, "g.fst", g)
    am = ident_model(g["num_tids"])
    lls = [SG.planted(g, 200, seed=s)[0] for s in range(4)]
    small = pk.Decoder(pk.Fst(path), am, 4, trace_capacity=64)
    with pytest.raises(pk.PkError) as e:
        small.decode(lls)
    assert e.value.code == -6 and "utterance" in str(e.value)
    with pytest.raises(pk.PkError):
        small.result(0)
    small.close()
    dec = pk.Decoder(pk.Fst(path), am, 4)
    dec.decode(lls)
    for u, ll in enumerate(lls):
        check_self(dec, u, path, ll, lambda t: t, g["final"], 0)
        assert dec.result(u)[2] == 1


def test_ilabel_outside_tid2pdf_rejected_at_create(tmp_path):
    from refmodel_text import load_text_model
    layers, prior, Lc, Rc, tid2pdf, cmvn41 = load_text_model()
    am = pk.AcousticModel(layers, prior, Lc, Rc, tid2pdf)
    path = str(tmp_path / "bad.fst")
    SG.write_fst(path, 0, np.array([0.0], np.float32), [[(0, len(tid2pdf) + 5, 0, 0.5)]])
    with pytest.raises(pk.PkError) as e:
        pk.Decoder(pk.Fst(path), am, 1)
    assert e.value.code == -1 and "tid2pdf" in str(e.value)


# ---------------------------------------------------------------- 8. batch equals solo

def test_batch_equals_solo(tmp_path):
    g = SG.size_for_states(20000, seed=11)
    path = write_graph(tmp_path, "g.fst", g)
    am = ident_model(g["num_tids"])
    lls = [SG.planted(g, 60 + 7 * u, seed=100 + u)[0] for u in range(64)]
    fst = pk.Fst(path)
    dec = pk.Decoder(fst, am, 64)
    dec.decode(lls)
    batch = [(dec.result(u), dec.best_path_arcs(u)) for u in range(64)]
    solo = pk.Decoder(fst, am, 1)
    for u in range(0, 64, 7):
        solo.decode([lls[u]])
        (w, wt, ok), p = batch[u]
        sw, swt, sok = solo.result(0)
        assert (w, np.float32(wt).tobytes(), ok, p) == (sw, np.float32(swt).tobytes(), sok, solo.best_path_arcs(0))


def test_decode_batch_requires_the_decoders_model():
    """A batch scored with another model (same num_pdfs, possibly another tid2pdf) is refused, not decoded through
    the wrong pdf map."""
    from refmodel_text import DIR, load_text_model
    layers, prior, Lc, Rc, tid2pdf, cmvn41 = load_text_model()
    fst = pk.Fst(os.path.join(DIR, "wordloop.fst"))
    am1 = pk.AcousticModel(layers, prior, Lc, Rc, tid2pdf)
    am2 = pk.AcousticModel(layers, prior, Lc, Rc, tid2pdf)
    wave = pk.read_wav(os.path.join(G, "en-us-hello.wav"))
    bs = pk.BatchScorer(am2, cmvn41, 1, len(wave))
    bs.set_waves([wave])
    bs.score(0.1)
    dec = pk.Decoder(fst, am1, 1)
    with pytest.raises(pk.PkError) as e:
        dec.decode_batch(bs)
    assert e.value.code == -1 and "another model" in str(e.value)
    pk.Decoder(fst, am2, 1).decode_batch(bs)
