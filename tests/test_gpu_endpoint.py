"""Online endpointing at the decoder (pk_mi355_online_decoder_set_endpointing / _endpoint / _finish:
csrc/capi_online_decoder.hip; EndpointKernel in csrc/decode.hip).  After every advance a slot's record is the host
model's (tests/endpoint_model.py), costs bit for bit, with commit and alignment on or off; the kernel's chunk, wave and
mask-word edges; finish() against Decoder.decode on the rows seen so far; slots do not disturb each other; and with the
mode off nothing changes."""
import numpy as np
import pytest

import pocketkaldi_amd as pk
from pocketkaldi_amd import synth_graph as SG

import endpoint_cases as EC
import endpoint_model as EM
from commit_cases import PDF, with_ids
from test_gpu_align import bits
from test_gpu_decode_edges import graph
from test_gpu_online_align import batch, full
from test_gpu_online_decode import ident_model, write_graph

pytestmark = pytest.mark.gpu
E_INVALID, E_STATE, E_CAPACITY = -1, -4, -6
INF = np.inf
NONE = (0, 0, 0, 0, 0, 0, 0, 0)                 # valid = 0: everything else is 0


def in_frames(rules):
    return [(int(bool(r[0])), int(round(r[1] * 100)), r[2], int(round(r[3] * 100))) for r in rules]


def make(fst, am, n, silence, rules=EC.RULES, commit=False, align=False, cap=1 << 16, beam=16.0, max_active=30000):
    dec = pk.OnlineDecoder(fst, am, n, trace_capacity=cap)
    dec.set_beam(beam, max_active)
    if align:
        dec.set_alignment(True)
    if commit:
        dec.set_commit(True)
    dec.set_endpointing(silence, rules)
    return dec


def got(dec, slot):
    e = dec.endpoint(slot)
    return (e.valid, e.frames, e.trailing_silence_frames, e.num_final, e.rule, bits(e.best_cost), bits(e.final_cost),
            bits(e.relative_cost))


def want(step, rules=EC.RULES):
    e = step["endpoint"]
    if e is None or not step["ok"]:
        return NONE
    rule = EC.eval_frames(in_frames(rules), e["frames"], e["trailing_silence_frames"], e["relative_cost"])
    return (1, e["frames"], e["trailing_silence_frames"], e["num_final"], rule, bits(e["best_cost"]), bits(e["final_cost"]),
            bits(e["relative_cost"]))


def follow(dec, slot, ll, ends, steps, rules=EC.RULES, paths=True):
    """Slot (open) is fed ll up to each of `ends`; after every advance its record is the model's.  -> the rules fired."""
    fired, pos = [], 0
    for end in ends:
        dec.advance_host({slot: (ll[pos:end], False)})
        pos = end
        assert got(dec, slot) == want(steps[end], rules), (slot, end)
        if paths and steps[end]["determined"]:
            assert dec.best_path_arcs(slot) == (steps[end]["best"] or []), (slot, end)
        fired.append(dec.endpoint(slot).rule)
    return fired


# ---------------------------------------------------------------- 1. records against the model

@pytest.mark.parametrize("seed", EC.SEEDS)
def test_records_equal_the_models_in_every_mode(tmp_path, seed):
    g, (ll, _, _), steps = EC.graph(seed), EC.stream(seed), EC.model_steps(seed)
    assert all(s["determined"] for s in steps)                                     # no case is skipped
    fst, am = pk.Fst(write_graph(tmp_path, "w.fst", g)), ident_model(g["num_pdfs"])
    ends = EC.chunk_ends(ll.shape[0])
    crossed = 0
    for commit in (False, True):
        for align in (False, True):
            dec = make(fst, am, 1, SG.silence_pdfs(g), commit=commit, align=align)
            dec.open(0)
            assert got(dec, 0) == NONE                                             # not advanced yet
            fired, pos = [], 0
            for end in ends:
                dec.advance_host({0: (ll[pos:end], False)})
                pos = end
                assert got(dec, 0) == want(steps[end]), (commit, align, end)
                assert dec.best_path_arcs(0) == steps[end]["best"], (commit, align, end)
                fired.append(dec.endpoint(0).rule)
                if commit:                       # the silence run began among the committed arcs
                    e = dec.endpoint(0)
                    crossed += e.trailing_silence_frames > 0 and dec.committed(0)[2] > e.frames - e.trailing_silence_frames
            assert sum(1 for r in fired if r) >= 2 and any(r in (2, 3) for r in fired), fired
            dec.advance_host({0: (ll[:0], True)})
            assert got(dec, 0) == NONE                                             # finished
    assert crossed > 0


# ---------------------------------------------------------------- 2. kernel edges

def two_state():
    """State 0 loops on pdf 2 (speech) and leaves to state 1 on pdf 1 (silence), which loops on it: the path of T frames
    has exactly T arcs."""
    return graph([INF, 0.5], [[(0, 2, 1, 0.25), (1, 1, 2, 0.5)], [(1, 1, 0, 0.125)]], num_pdfs=4)


def speech_then_silence(T, speech):
    ll = np.full((T, 4), -20.0, np.float32)
    ll[:speech, 2] = -0.5
    ll[speech:, 1] = -0.25
    return ll


# (arcs of the scanned path, how many of its first arcs are speech): the scan's chunks are 512 arcs, its waves 64
EDGES = [(0, 0), (1, 0), (1, 1), (511, 0), (512, 0), (513, 0), (1025, 0), (512, 1), (513, 511), (513, 512), (513, 513),
         (1025, 63), (1025, 64), (1025, 65), (1025, 513), (1025, 1024)]
EDGE_RULES = [pk.EndpointRule(True, 0.05, INF, 0.0), pk.EndpointRule(False, 6.00, INF, 0.0)]


def test_path_lengths_at_the_scan_edges(tmp_path):
    g = two_state()
    fst, am = pk.Fst(write_graph(tmp_path, "t.fst", g)), ident_model(4)
    dec = make(fst, am, len(EDGES), [1], EDGE_RULES, cap=4096)
    lls = [speech_then_silence(T, s) for T, s in EDGES]
    for u in range(len(EDGES)):
        dec.open(u)
    dec.advance_host({u: (ll, False) for u, ll in enumerate(lls)})
    for u, (T, speech) in enumerate(EDGES):
        step = list(EM.frames(with_ids(g), lls[u], PDF, silence=[1]))[-1]
        assert len(step["tokens"]) == 1                                            # nL = 1
        assert got(dec, u) == want(step, EDGE_RULES), (T, speech)
        e = dec.endpoint(u)
        assert len(dec.best_path_arcs(u)) == T and (e.frames, e.trailing_silence_frames) == (T, T - speech)
        # an all-silent path: the rule that must contain speech stays quiet, however long the silence
        assert e.rule == (0 if T == 0 else 1 if 0 < speech and T - speech >= 5 else 2 if T - speech >= 600 else 0), (T, speech)


def test_paths_that_end_in_epsilon_arcs(tmp_path):
    # 0 -sil-> 2 -eps-> 3 -eps-> 1 -sil-> 2 ...: the epsilon arcs are cheaper than nothing, so the best path ends in two
    g = graph([INF, 0.0, INF, INF], [[(2, 1, 5, 0.5)], [(2, 1, 0, 0.25)], [(3, 0, 0, -0.25)], [(1, 0, 6, -0.25)]], num_pdfs=4)
    fst, am = pk.Fst(write_graph(tmp_path, "e.fst", g)), ident_model(4)
    ll = np.full((606, 4), -0.5, np.float32)
    ends = [1, 2, 3, 4, 5, 6, 606]                       # the last launch's path: 1818 arcs, a third of them emitting
    for silence, commit in [([1], False), ([1], True), ([], False), ([2, 3], True)]:
        steps = EC.steps_of(g, ll, silence)
        assert all(s["determined"] for s in steps) and steps[6]["best"][-2:] == [2, 3]
        dec = make(fst, am, 1, silence, EDGE_RULES, commit=commit, cap=8192)
        dec.open(0)
        follow(dec, 0, ll, ends, steps, EDGE_RULES)
        e = dec.endpoint(0)
        assert (e.frames, e.trailing_silence_frames) == (606, 606 if silence == [1] else 0)
        assert e.rule == (2 if silence == [1] else 0)


def test_silence_pdfs_at_the_mask_words_edges(tmp_path):
    # num_pdfs = 45: two mask words, the second one partly used; pdf 0 is never an arc's (ilabel 0 is epsilon)
    pdfs = [5, 31, 32, 44, 0, 33, 30, 43, 1, 44, 32, 31, 31]
    arcs = [[(i + 1, p, i + 1, 0.25)] for i, p in enumerate(pdfs)] + [[]]
    g = graph([INF] * len(pdfs) + [1.0], arcs, num_pdfs=45)
    fst, am = pk.Fst(write_graph(tmp_path, "m.fst", g)), ident_model(45)
    T = sum(1 for p in pdfs if p)
    ll = SG.dyadic(T, 45, seed=3)
    dec = make(fst, am, 1, [0, 31, 32, 44], EDGE_RULES)
    seen = set()
    for silence in ([0, 31, 32, 44], [31], [32], [44], [0], [30, 33, 43], list(range(45)), []):
        dec.set_endpointing(silence, EDGE_RULES)
        steps = EC.steps_of(g, ll, silence)
        dec.open(0)
        follow(dec, 0, ll, list(range(1, T + 1)), steps, EDGE_RULES)
        seen.add(tuple(s["endpoint"]["trailing_silence_frames"] for s in steps))
        dec.finish([0])
    assert len(seen) == 7                                # every set tells itself apart, but [0] from []: no arc has pdf 0


@pytest.mark.parametrize("final, silence", [("inf", True), ("zero", True), ("graph", False)])
def test_final_weights_all_inf_all_zero_and_an_empty_silence_set(tmp_path, final, silence):
    seed = EC.SEEDS[0]
    g, ll = dict(EC.graph(seed)), EC.stream(seed)[0]
    if final != "graph":
        g["final"] = np.full_like(g["final"], INF if final == "inf" else 0.0)
    sil = SG.silence_pdfs(g) if silence else []
    steps = EC.steps_of(g, ll, sil)
    assert all(s["determined"] for s in steps)
    fst, am = pk.Fst(write_graph(tmp_path, "w.fst", g)), ident_model(g["num_pdfs"])
    dec = make(fst, am, 1, sil)
    dec.open(0)
    fired = follow(dec, 0, ll, EC.chunk_ends(ll.shape[0]), steps)
    e = dec.endpoint(0)
    if final == "inf":                                   # no final token: only the rules that do not ask the cost
        assert e.num_final == 0 and bits(e.final_cost) == bits(e.relative_cost) == bits(INF)
        assert set(fired) <= {0, 1, 4, 5} and 4 in fired and 5 in fired
    elif final == "zero":                                # every token is final: the best one is the best final one
        assert e.num_final == len(steps[-1]["tokens"]) and e.relative_cost == 0.0 and e.final_cost == e.best_cost
        assert 2 in fired
    else:                                                # no silence: only the length rule
        assert e.trailing_silence_frames == 0 and set(fired) == {0, 5}


def test_more_tokens_than_the_workgroup_is_wide(tmp_path):
    g = SG.word_loop(80, 10, seed=3)
    g["num_pdfs"] = g["num_tids"]
    ll = SG.flat(12, g["num_pdfs"], seed=4)
    steps = EC.steps_of(g, ll, SG.silence_pdfs(g))
    assert all(s["determined"] for s in steps) and len(steps[-1]["tokens"]) > 512 > len(steps[6]["tokens"])
    fst, am = pk.Fst(write_graph(tmp_path, "w.fst", g)), ident_model(g["num_pdfs"])
    dec = make(fst, am, 1, SG.silence_pdfs(g))
    dec.open(0)
    follow(dec, 0, ll, [1, 3, 6, 7, 8, 12], steps)
    assert dec.endpoint(0).num_final == 2


# ---------------------------------------------------------------- 3. finish

@pytest.mark.parametrize("commit", [False, True])
def test_finish_equals_the_batch_decoder_on_the_rows_so_far(tmp_path, commit):
    seed = EC.SEEDS[1]
    g, ll = EC.graph(seed), EC.stream(seed)[0]
    fst, am = pk.Fst(write_graph(tmp_path, "w.fst", g)), ident_model(g["num_pdfs"])
    ks = [0, 1, 20, 33]                                  # fresh; one frame; a chunk's edge (7 + 13); inside a word
    heads, tails = batch(fst, am, [ll[:k] for k in ks]), batch(fst, am, [ll[k:] for k in ks])
    dec = make(fst, am, len(ks), SG.silence_pdfs(g), commit=commit, align=True)
    for u, k in enumerate(ks):
        dec.open(u)
    for a, b in [(0, 7), (7, 20), (20, 33)]:
        dec.advance_host({u: (ll[a:min(b, k)], False) for u, k in enumerate(ks) if min(b, k) > a})
    dec.finish(list(range(len(ks))), sync=False)
    with pytest.raises(pk.PkCodeError) as err:           # getters before synchronize
        dec.result(0)
    assert err.value.code == E_STATE
    with pytest.raises(pk.PkCodeError) as err:
        dec.endpoint(0)
    assert err.value.code == E_STATE
    dec.synchronize()
    for u, k in enumerate(ks):
        assert full(dec, u) == full(heads, u), k
        assert dec.num_frames(u) == k and got(dec, u) == NONE
    with pytest.raises(pk.PkCodeError) as err:           # a slot that is not open
        dec.finish([1])
    assert err.value.code == E_STATE
    for u, k in enumerate(ks):                           # opened again at once: the rest of the rows
        dec.open(u)
        assert got(dec, u) == NONE
    dec.advance_host({u: (ll[k:k + 50], False) for u, k in enumerate(ks)})
    for u, k in enumerate(ks):
        assert dec.endpoint(u).frames == 50              # a slot reopened after finish starts from frames = 0
    dec.advance_host({u: (ll[k + 50:], True) for u, k in enumerate(ks)})
    for u, k in enumerate(ks):
        assert full(dec, u) == full(tails, u), k


# ---------------------------------------------------------------- 4. isolation

def test_four_slots_at_different_stages_in_one_call(tmp_path):
    seed = EC.SEEDS[2]
    g, ll, steps = EC.graph(seed), EC.stream(seed)[0], EC.model_steps(seed)
    fst, am = pk.Fst(write_graph(tmp_path, "w.fst", g)), ident_model(g["num_pdfs"])
    dec = make(fst, am, 4, SG.silence_pdfs(g), commit=True)
    plans = [(7, 13, 50), (50, 7, 13), (31,), (13, 50, 7)]
    pos = [0, 0, 0, 0]
    for u in range(4):
        dec.open(u)
    dec.advance_host({3: (ll[:100], False)})             # slot 3 runs ahead
    pos[3] = 100
    kept = None
    for step in range(9):
        absent = step % 4                                # one slot sits every call out, and keeps its record
        kept = got(dec, absent)
        chunks = {}
        for u in range(4):
            if u != absent:
                n = plans[u][step % len(plans[u])]
                chunks[u] = (ll[pos[u]:pos[u] + n], False)
                pos[u] = min(pos[u] + n, ll.shape[0])
        dec.advance_host(chunks)
        assert got(dec, absent) == kept
        for u in chunks:
            assert got(dec, u) == want(steps[pos[u]]), (step, u)
    assert len(set(pos)) == 4


def test_a_slot_out_of_records_reports_nothing_and_disturbs_no_other(tmp_path):
    g = SG.size_for_states(3000, num_phones=60, seed=5)
    fst, am = pk.Fst(write_graph(tmp_path, "w.fst", g)), ident_model(g["num_tids"])
    good = SG.planted(g, 40, seed=1, bonus=30.0, noise=0.5)[0]
    T = good.shape[0]
    bad = SG.flat(T, g["num_tids"], seed=2)
    sil = SG.silence_pdfs(g)
    alone = make(fst, am, 2, sil, cap=600)
    alone.open(1)
    records = []
    for t in range(T):
        alone.advance_host({1: (good[t:t + 1], False)})
        records.append(got(alone, 1))
    assert all(r[0] == 1 for r in records)
    dec = make(fst, am, 2, sil, cap=600)
    dec.open(0)
    dec.open(1)
    codes = []
    for t in range(T):
        try:
            dec.advance_host({0: (bad[t:t + 1], False), 1: (good[t:t + 1], False)})
        except pk.PkCodeError as e:
            codes.append(e.code)
        assert got(dec, 1) == records[t], t
        assert got(dec, 0)[0] == (0 if codes else 1)
    assert codes and set(codes) == {E_CAPACITY} and got(dec, 0) == NONE


# ---------------------------------------------------------------- 5. the mode's rules; mode off

def test_mode_rules(tmp_path):
    g = two_state()
    fst, am = pk.Fst(write_graph(tmp_path, "t.fst", g)), ident_model(4)
    dec = pk.OnlineDecoder(fst, am, 2, trace_capacity=4096)

    def refused(code, *args):
        with pytest.raises(pk.PkCodeError) as err:
            dec.set_endpointing(*args)
        assert err.value.code == code

    with pytest.raises(pk.PkCodeError) as err:           # mode off
        dec.endpoint(0)
    assert err.value.code == E_STATE
    refused(E_INVALID, [4], EC.RULES)                    # a pdf outside [0, num_pdfs)
    refused(E_INVALID, [-1], EC.RULES)
    refused(E_INVALID, [1], [pk.EndpointRule(True, -0.01, 1.0, 0.0)])
    refused(E_INVALID, [1], [pk.EndpointRule(True, 0.1, 1.0, -1.0)])
    refused(E_INVALID, [1], [pk.EndpointRule(True, 0.1, float("nan"), 0.0)])
    dec.open(0)
    refused(E_STATE, [1], EC.RULES)                      # the mode is the object's: not while a slot is open
    dec.advance_host({0: (speech_then_silence(9, 2), False)})
    dec.finish([0])                                      # finish needs no mode
    assert dec.result(0)[2] == 1 and dec.num_frames(0) == 9
    dec.set_endpointing([1], EDGE_RULES)
    dec.open(1)
    dec.advance_host({1: (speech_then_silence(9, 2), False)})
    assert dec.endpoint(1).rule == 1 and dec.endpoint(1).trailing_silence_frames == 7 and dec.endpoint(0).valid == 0
    dec.finish([1])
    dec.set_endpointing([1], [])                         # off again
    with pytest.raises(pk.PkCodeError) as err:
        dec.endpoint(1)
    assert err.value.code == E_STATE
    dec.set_endpointing([], None)                        # the default rules, an empty silence set
    dec.open(0)
    dec.advance_host({0: (speech_then_silence(9, 2), False)})
    assert dec.endpoint(0).valid == 1 and dec.endpoint(0).trailing_silence_frames == 0 and dec.endpoint(0).rule == 0


def test_mode_off_results_are_the_batch_recognizers():
    from test_gpu_online_recognizer import CAT, CONF, HELLO, TRACE, comparable
    waves = [pk.read_wav(HELLO), pk.read_wav(CAT)]
    rec = pk.Recognizer(CONF, max_utts=2, max_total_samples=sum(len(w) for w in waves), trace_capacity=TRACE)
    expect = [comparable(r) for r in rec.process(waves)]
    rec.close()
    online = pk.OnlineRecognizer(CONF, max_streams=2, max_step_samples=2 * 4001, trace_capacity=TRACE)
    assert expect[0][0] and expect[1][0]
    online.decoder.set_endpointing([0], None)            # on, then off again: nothing of it stays
    online.decoder.set_endpointing([0], [])
    for u in range(2):
        online.open(u)
    for pos in range(0, max(len(w) for w in waves), 4000):
        for u, w in enumerate(waves):
            if pos < len(w):
                online.push(u, w[pos:pos + 4000])
                if pos + 4000 >= len(w):
                    online.close(u)
        online.step()
        with pytest.raises(pk.PkCodeError) as err:
            online.decoder.endpoint(0)
        assert err.value.code == E_STATE
    assert [comparable(online.result(u)) for u in range(2)] == expect
    online.destroy()
