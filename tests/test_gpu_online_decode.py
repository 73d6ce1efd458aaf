"""The online decoder (pk_mi355_online_decoder_*: csrc/capi_online_decoder.hip over the decoder core, OnlineDecodeKernel
in csrc/decode.hip): log-likelihoods fed in chunks
must end in the words, weight bits, ok, best-path arcs and active_bound of Decoder.decode on the whole utterance;
partial hypotheses equal the decode of the prefix on graphs whose final weights are 0; compaction of the per-slot
backtrace arena changes no result; a refused set_beam changes no result; and OnlineScorer + OnlineDecoder equal
BatchScorer + Decoder.decode_batch."""
import os

import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth, synth_graph as SG

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_INVALID, E_CAPACITY = -1, -6


def ident_model(num_pdfs):
    W = np.zeros((num_pdfs, 4), np.float32)
    return pk.AcousticModel([("linear", W, np.zeros(num_pdfs, np.float32))], prior=np.full(num_pdfs, 1.0 / num_pdfs, np.float32))


def write_graph(tmp_path, name, g):
    p = str(tmp_path / name)
    SG.write_fst(p, g["start"], g["final"], g["arcs"])
    return p


def whole(fst, am, lls, beam=16.0, max_active=30000):
    dec = pk.Decoder(fst, am, len(lls))
    dec.set_beam(beam, max_active)
    dec.decode(lls)
    return [(dec.result(u), dec.best_path_arcs(u), dec.active_bound(u)) for u in range(len(lls))]


def split(T, how, rng):
    if how == "whole":
        return [T]
    if how == 1:
        return [1] * T
    out, left = [], T
    while left > 0:
        c = int(min(left, rng.integers(0, 12)))
        out.append(c)
        left -= c
    return out


def online(fst, am, lls, hows, beam=16.0, max_active=30000, cap=0, seed=0, partial_check=None):
    """All utterances in one OnlineDecoder, slot u fed lls[u] in chunks split(how); returns final results."""
    rng = np.random.default_rng(seed)
    dec = pk.OnlineDecoder(fst, am, len(lls), trace_capacity=cap)
    dec.set_beam(beam, max_active)
    plans = [split(ll.shape[0], h, rng) for ll, h in zip(lls, hows)]
    pos = [0] * len(lls)
    for u in range(len(lls)):
        dec.open(u)
    step = 0
    while any(step <= len(p) for p in plans):
        chunks = {}
        for u, p in enumerate(plans):
            if step < len(p):
                chunks[u] = (lls[u][pos[u]:pos[u] + p[step]], False)
                pos[u] += p[step]
            elif step == len(p):
                chunks[u] = (lls[u][pos[u]:pos[u]], True)
        dec.advance_host(chunks)
        if partial_check:
            for u in chunks:
                if not chunks[u][1]:
                    partial_check(dec, u, pos[u])
        step += 1
    return [(dec.result(u), dec.best_path_arcs(u), dec.active_bound(u)) for u in range(len(lls))]


def same(a, b):
    (wa, xa, oa), pa, ba = a
    (wb, xb, ob), pb, bb = b
    return wa == wb and np.float32(xa).tobytes() == np.float32(xb).tobytes() and oa == ob and pa == pb and ba == bb


# ---------------------------------------------------------------- 2. decoder exactness

@pytest.mark.parametrize("seed", range(3))
def test_general_graphs_dyadic(tmp_path, seed):
    g = SG.general(300, seed=40 + seed)
    fst = pk.Fst(write_graph(tmp_path, "g.fst", g))
    am = ident_model(g["num_pdfs"])
    lls = [SG.dyadic(int(T), g["num_pdfs"], seed=100 * seed + u) for u, T in enumerate([0, 1, 7, 40, 90, 130])]
    want = whole(fst, am, lls)
    for hows in ([1] * 6, ["random"] * 6, ["whole"] * 6):
        got = online(fst, am, lls, hows, seed=seed)
        for u in range(len(lls)):
            assert same(got[u], want[u]), (hows[0], u, got[u][0], want[u][0])


def test_word_loop_planted_and_max_active(tmp_path):
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    fst = pk.Fst(write_graph(tmp_path, "w.fst", g))
    am = ident_model(g["num_tids"])
    lls = [SG.planted(g, 60, seed=s)[0] for s in range(3)] + [SG.flat(40, g["num_tids"], seed=9)]
    for beam, ma in ((16.0, 30000), (16.0, 256), (0.0, 30000)):
        want = whole(fst, am, lls, beam, ma)
        if ma == 256:
            assert want[3][2] > 256                    # max-active binds
        got = online(fst, am, lls, [1, "random", "whole", "random"], beam, ma, seed=3)
        for u in range(len(lls)):
            assert same(got[u], want[u]), (beam, ma, u)


def test_testinput_with_refmodel():
    from refmodel_text import load_text_model
    layers, prior, L, R, tid2pdf, cmvn41 = load_text_model()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    fst = pk.Fst(os.path.join(G, "refmodel", "wordloop.fst"))
    waves = [pk.read_wav(os.path.join(G, w)) for w in ("en-us-hello.wav", "en-us-cat.wav")]
    bs = pk.BatchScorer(am, cmvn41, 2, sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    lls = [bs.fetch(u).log_prob() for u in range(2)]
    want = whole(fst, am, lls)
    got = online(fst, am, lls, [1, "random"], seed=4)
    assert all(same(got[u], want[u]) for u in range(2))
    tfst = pk.Fst(os.path.join(G, "testinput.fst"))
    am4 = ident_model(4)
    lls = [(np.random.default_rng(s).standard_normal((int(T), 4)) * 2).astype(np.float32) for s, T in enumerate([2, 5, 9])]
    want = whole(tfst, am4, lls)
    got = online(tfst, am4, lls, [1, 1, "random"], seed=5)
    assert all(same(got[u], want[u]) for u in range(3))


def test_nan_and_empty_frames_mid_stream(tmp_path):
    g = SG.general(200, seed=77)
    fst = pk.Fst(write_graph(tmp_path, "g.fst", g))
    am = ident_model(g["num_pdfs"])
    a = SG.dyadic(50, g["num_pdfs"], seed=1)
    a[20, 3] = np.nan                                   # N1
    b = SG.dyadic(50, g["num_pdfs"], seed=2)
    b[25, :] = -np.inf                                  # N2: ok = 0
    want = whole(fst, am, [a, b])
    assert want[1][0][2] == 0
    got = online(fst, am, [a, b], [1, "random"], seed=6)
    assert same(got[0], want[0]) and same(got[1], want[1])


def test_refused_set_beam_leaves_the_decoder_as_it_was():
    fst = pk.Fst(os.path.join(G, "testinput.fst"))
    am = ident_model(4)
    ll = (np.random.default_rng(11).standard_normal((3, 4)) * 2).astype(np.float32)

    def run(dec):
        dec.open(0)
        dec.advance_host({0: (ll, True)})
        return dec.result(0)

    want = run(pk.OnlineDecoder(fst, am, 1))               # an untouched decoder
    dec = pk.OnlineDecoder(fst, am, 1)
    for beam, max_active in ((-1.0, 10), (16.0, 0)):
        with pytest.raises(pk.PkCodeError) as e:
            dec.set_beam(beam, max_active)
        assert e.value.code == E_INVALID
    got = run(dec)
    assert got[0] == want[0] and np.float32(got[1]).tobytes() == np.float32(want[1]).tobytes() and got[2] == want[2]


# ---------------------------------------------------------------- 3. partials

def test_partials_equal_prefix_decodes(tmp_path):
    g = SG.general(250, seed=12)
    g["final"] = np.zeros_like(np.asarray(g["final"], np.float32))
    fst = pk.Fst(write_graph(tmp_path, "z.fst", g))
    am = ident_model(g["num_pdfs"])
    lls = [SG.dyadic(60, g["num_pdfs"], seed=50 + u) for u in range(2)]
    checked = []

    def check(dec, u, t):
        words, cost = dec.partial(u)
        (ww, wx, wok), _, _ = whole(fst, am, [lls[u][:t]])[0]
        if wok:
            assert words == ww and np.float32(cost).tobytes() == np.float32(wx).tobytes(), (u, t)
            checked.append(t)

    online(fst, am, lls, [1, "random"], seed=7, partial_check=check)
    assert len(checked) > 40


# ---------------------------------------------------------------- 4. compaction

def test_small_arena_compacts_to_the_same_result(tmp_path):
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    fst = pk.Fst(write_graph(tmp_path, "w.fst", g))
    am = ident_model(g["num_tids"])
    lls = [SG.planted(g, 150, seed=s)[0] for s in range(2)]
    want = whole(fst, am, lls)
    records = sum(b * ll.shape[0] for (_, _, b), ll in zip(want, lls))      # an upper bound of what the decode wrote
    cap = max(records // 20 // len(lls), 1)
    assert max(b for _, _, b in want) * 4 < cap
    got = online(fst, am, lls, [1, "random"], cap=cap, seed=8)
    assert all(same(got[u], want[u]) for u in range(2))


def test_full_arena_ends_one_slot_only(tmp_path):
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    fst = pk.Fst(write_graph(tmp_path, "w.fst", g))
    am = ident_model(g["num_tids"])
    good = SG.planted(g, 40, seed=1, bonus=30.0, noise=0.5)[0]
    T = good.shape[0]                                   # whole planted words: about 40 frames
    bad = SG.flat(T, g["num_tids"], seed=2)
    want = whole(fst, am, [good])[0]
    dec = pk.OnlineDecoder(fst, am, 2, trace_capacity=600)
    dec.open(0)
    dec.open(1)
    codes = []
    for t in range(T + 1):
        fin = t == T
        try:
            dec.advance_host({0: (bad[t:t + 1] if not fin else bad[:0], fin), 1: (good[t:t + 1] if not fin else good[:0], fin)})
        except pk.PkCodeError as e:
            codes.append(e.code)
    assert codes and set(codes) == {E_CAPACITY}
    assert dec.result(0)[2] == 0
    assert same((dec.result(1), dec.best_path_arcs(1), dec.active_bound(1)), want)


# ---------------------------------------------------------------- 5. end to end

def stream_decode(sc, dec, waves, chunk, stagger):
    """Every wave in its own slot, `chunk` samples per step, opened at step stagger[u]; -> (words, weight, ok)."""
    n = len(waves)
    pos, state, out, step = [0] * n, ["pending"] * n, [None] * n, 0
    while any(s != "done" for s in state):
        for u in range(n):
            if state[u] == "pending" and step >= stagger[u]:
                sc.open(u)
                dec.open(u)
                state[u] = "open"
            if state[u] == "open":
                if pos[u] < len(waves[u]):
                    sc.push(u, waves[u][pos[u]:pos[u] + chunk])
                    pos[u] += chunk
                    if pos[u] >= len(waves[u]):
                        sc.close(u)                   # last chunk and close in the same step
                        state[u] = "closed"
                else:
                    sc.close(u)
                    state[u] = "closed"
        if any(s in ("open", "closed") for s in state):
            sc.step(0.1, sync=False)
            dec.advance(sc)
            for u in range(n):
                if state[u] == "open":
                    dec.partial(u)
                elif state[u] == "closed":
                    out[u] = dec.result(u)
                    state[u] = "done"
        step += 1
    return out


def test_end_to_end_golden_waves():
    from refmodel_text import load_text_model
    layers, prior, L, R, tid2pdf, cmvn41 = load_text_model()
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    fst = pk.Fst(os.path.join(G, "refmodel", "wordloop.fst"))
    waves = [pk.read_wav(os.path.join(G, w)) for w in ("en-us-hello.wav", "en-us-cat.wav")]
    bs = pk.BatchScorer(am, cmvn41, 2, sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    d = pk.Decoder(fst, am, 2)
    d.decode_batch(bs)
    want = [d.result(u) for u in range(2)]
    sc = pk.OnlineScorer(am, cmvn41, 2, 4000)
    dec = pk.OnlineDecoder(fst, am, 2)
    got = stream_decode(sc, dec, waves, 1600, [0, 2])
    for u in range(2):
        assert got[u][0] == want[u][0] and np.float32(got[u][1]).tobytes() == np.float32(want[u][1]).tobytes()
        assert got[u][2] == want[u][2] == 1 and len(got[u][0]) >= 1


def test_end_to_end_32_streams(tmp_path):
    layers, prior, L, R = synth.model("S")
    am = pk.AcousticModel(layers, prior, L, R)
    g = synth.global_cmvn_stats()
    gr = SG.size_for_states(20000, seed=1)
    fst = pk.Fst(write_graph(tmp_path, "s.fst", gr))
    rng = np.random.default_rng(21)
    waves = [synth.utterance(2000 + i, seconds=float(rng.uniform(0.02, 2.5))) for i in range(32)]
    bs = pk.BatchScorer(am, g, 32, sum(len(w) for w in waves))
    bs.set_waves(waves)
    bs.score(0.1)
    d = pk.Decoder(fst, am, 32)
    d.set_beam(16.0, 2000)
    d.decode_batch(bs)
    want = [d.result(u) for u in range(32)]
    sc = pk.OnlineScorer(am, g, 32, 32 * 1600)
    dec = pk.OnlineDecoder(fst, am, 32)
    dec.set_beam(16.0, 2000)
    got = stream_decode(sc, dec, waves, 1600, [int(x) for x in rng.integers(0, 5, 32)])
    for u in range(32):
        assert got[u][0] == want[u][0] and np.float32(got[u][1]).tobytes() == np.float32(want[u][1]).tobytes(), u
        assert got[u][2] == want[u][2], u
