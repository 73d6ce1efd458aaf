"""The online scorers at a normalisation spec: StreamNormKernel and StreamFeatureLayoutKernel in
StreamCmvnKernel's and StreamCmvnChainKernel's place.
  * For `none`, `speaker` (with and without variance) and online CMVN (W = 8 and W = 600, with and without variance and
    speaker records) a slot's rows over its life are the batch scorer's under the same spec on the whole input, bit for
    bit: feature slots at D in {1, 40, 41, 65, 130}, audio slots of the 40-dim scorer and of an 80-bin front-end (the
    committed waves and one at 8 kHz), chunks of 1, 7, W - 1 and W + 1 frames and everything at once with empty pushes
    between, slots closed and reopened, RAW, NORMALIZED and audio slots together in one step.
  * norm_stats(slot) is BatchScorer.norm_stats as doubles.
  * A scorer whose norm was never set, or was set to `sliding` again, gives the same bits; poisoned neighbours across
    slots change no bit; every failure code; set_norm with a slot open is refused."""
import ctypes as C
import os

import numpy as np
import pytest

import pocketkaldi_amd as pk

import frontend_any_cases as FA
import norm_cases as NC
import online_cmvn_cases as OC
from test_gpu_cmvn_any import tiny
from test_gpu_norm import code_of
from test_gpu_stream_features import chunks_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_INVALID, E_STATE = -1, -4
DIMS = [1, 40, 41, 65, 130]
L, R = 2, 1
SPECS = [("none", pk.NormSpec("none")), ("speaker", pk.NormSpec("speaker", True, False)), ("speaker-vars", pk.NormSpec("speaker", True, True)),
         ("speaker-vars-only", pk.NormSpec("speaker", False, True)),
         ("online8", pk.OnlineCmvnSpec(8, 3, 2, False)), ("online8-vars", pk.OnlineCmvnSpec(8, 3, 2, True)),
         ("online600", pk.OnlineCmvnSpec()), ("online600-vars", pk.OnlineCmvnSpec(norm_vars=True))]


def is_online(spec):
    return isinstance(spec, pk.OnlineCmvnSpec)


def set_norm(obj, spec, glob):
    if is_online(spec):
        obj.set_norm(spec, glob if spec.global_frames else None)
    else:
        obj.set_norm(spec)


def takes_records(spec):
    return is_online(spec) or spec.mode == pk.NORM_MODES["speaker"]


def batch_reference(make, spec, glob, inputs, spk, kinds=None, rates=None):
    """The batch scorer under `spec` on the whole inputs -> (rows per input, the utterance-mode records per input)."""
    bs = make()
    set_norm(bs, spec, glob)

    def feed():
        if kinds is None:
            bs.set_waves(inputs, rates)
        else:
            bs.set_features(inputs, kinds)

    if takes_records(spec) and spk is not None:
        bs.set_speaker_stats(spk)
    feed()
    bs.score(0.1)
    rows = [bs.fetch(u).log_prob() for u in range(len(inputs))]
    bs.set_norm(pk.NormSpec("utterance", True, True))
    feed()
    bs.score(0.1)
    recs = [bs.norm_stats(u) for u in range(len(inputs))]
    bs.close()
    return rows, recs


def run(sc, jobs):
    """jobs: dicts {slot, kind ("audio" | "raw" | "normalized"), data, chunks (in frames or samples), rate, spk}.  Jobs of one
    slot run one after the other; a job pushes one chunk per step and closes in a step of its own.  -> per job (rows, the
    slot's norm_stats after its flush or None)."""
    n = len(jobs)
    rows, nxt, state, k, pos, busy = [[] for _ in range(n)], [0] * n, ["pending"] * n, [0] * n, [0] * n, {}
    stats = [None] * n
    N = sc._am.num_pdfs()
    while any(s != "done" for s in state):
        for i, j in enumerate(jobs):
            if state[i] == "pending" and j["slot"] not in busy:
                if j["kind"] == "audio":
                    sc.open(j["slot"], j.get("rate", 16000), speaker_stats=j.get("spk"))
                else:
                    sc.open_features(j["slot"], j["kind"], speaker_stats=j.get("spk"))
                busy[j["slot"]] = i
                state[i] = "open"
            if state[i] == "open":
                if k[i] < len(j["chunks"]):
                    c = j["chunks"][k[i]]
                    (sc.push if j["kind"] == "audio" else sc.push_features)(j["slot"], j["data"][pos[i]:pos[i] + c])
                    pos[i] += c
                    k[i] += 1
                else:
                    sc.close(j["slot"])
                    state[i] = "closed"
        sc.step(0.1)
        for i, j in enumerate(jobs):
            if state[i] not in ("open", "closed"):
                continue
            first, r = sc.fetch(j["slot"])
            if r.shape[0]:
                assert first == nxt[i], (i, first, nxt[i])
                rows[i].append(r)
                nxt[i] += r.shape[0]
            if state[i] == "closed":
                state[i] = "done"
                if j.get("stats"):
                    stats[i] = sc.norm_stats(j["slot"])
                del busy[j["slot"]]
    return [(np.concatenate(r) if r else np.zeros((0, N), np.float32), st) for r, st in zip(rows, stats)]


def chunkings(W, T):
    return [1, 7, W - 1, W + 1, "whole", "random"] if T <= 100 else [W - 1, W + 1, "whole", "random"]


# ---------------------------------------------------------------- feature slots: identity with the batch scorer

@pytest.mark.parametrize("name, spec", SPECS, ids=[s[0] for s in SPECS])
@pytest.mark.parametrize("D", DIMS)
def test_feature_slots_are_the_batch_scorer(D, name, spec):
    W = spec.cmn_window if is_online(spec) else 8
    T = 70 if W == 8 else 1307
    rng = np.random.default_rng([D, W])
    am, _, _ = tiny(D, L, R)
    hows = chunkings(W, T)
    raw = [NC.features(T, D, 7), OC.wide(T, D, 8) if is_online(spec) else NC.features(T - 3, D, 8), NC.features(5, D, 9)]
    glob = OC.record(NC.features(300, D, 3))
    spk = [OC.record(NC.features(50, D, 100 + u), OC.SPEAKER_COUNT) for u in range(len(raw))]
    want, recs = batch_reference(lambda: pk.FeatureScorer(am, len(raw), sum(x.shape[0] for x in raw)), spec, glob, raw, spk, "raw")
    # every chunking of utterance 0 in a slot of its own, all in one object; utterances 1 and 2 share the last slot, one
    # after the other and then once more: the state of a slot does not leak into its next opening
    jobs = [dict(slot=i, kind="raw", data=raw[0], chunks=chunks_of(T, how, rng), spk=spk[0], stats=True) for i, how in enumerate(hows)]
    last = len(hows)
    for u in (1, 2, 1):
        jobs.append(dict(slot=last, kind="raw", data=raw[u], chunks=chunks_of(raw[u].shape[0], "random", rng), spk=spk[u], stats=True))
    if not takes_records(spec):
        for j in jobs:
            j["spk"], j["stats"] = None, False
    sc = pk.OnlineFeatureScorer(am, last + 1, (len(hows) + 1) * T)               # no statistics: RAW is the norm spec's alone
    set_norm(sc, spec, glob)
    got = run(sc, jobs)
    for i, (rows, st) in enumerate(got):
        u = 0 if i < last else (1, 2, 1)[i - last]
        assert NC.bits_equal(rows, want[u]), "%s D=%d job %d (utterance %d): rows differ" % (name, D, i, u)
        if takes_records(spec):
            assert NC.bits_equal(st, recs[u]), "%s D=%d job %d: norm_stats differ" % (name, D, i)
    sc.destroy()
    am.close()


def test_online_cmvn_without_speaker_records_and_without_global_frames():
    D, T = 41, 70
    rng = np.random.default_rng(5)
    am, _, _ = tiny(D, L, R)
    raw = [OC.wide(T, D, 8)]
    glob = OC.record(NC.features(300, D, 3))
    for spec in (pk.OnlineCmvnSpec(8, 3, 2, True), pk.OnlineCmvnSpec(8, 3, 0, True), pk.OnlineCmvnSpec(8, 0, 0, False)):
        want, _ = batch_reference(lambda: pk.FeatureScorer(am, 1, T), spec, glob, raw, None, "raw")
        sc = pk.OnlineFeatureScorer(am, 2, 2 * T)
        set_norm(sc, spec, glob)
        got = run(sc, [dict(slot=0, kind="raw", data=raw[0], chunks=chunks_of(T, 7, rng)),
                       dict(slot=1, kind="raw", data=raw[0], chunks=chunks_of(T, "random", rng))])
        assert NC.bits_equal(got[0][0], want[0]) and NC.bits_equal(got[1][0], want[0]), spec
        sc.destroy()
    am.close()


# ---------------------------------------------------------------- audio slots; RAW, NORMALIZED and audio in one step

AUDIO = [("stream40", None), ("fbank80", FA.SPECS[1])]


@pytest.mark.parametrize("name, fe", AUDIO, ids=[a[0] for a in AUDIO])
def test_audio_slots_are_the_batch_scorer_and_the_kinds_mix_in_one_step(name, fe):
    D = 40 if fe is None else fe.dim
    rng = np.random.default_rng(11)
    am, _, _ = tiny(D, L, R)
    g = np.concatenate([np.full(D, 10.0 * 2500.0), [2500.0]]).astype(np.float32)
    hello, cat = pk.read_wav(os.path.join(GOLDEN, "en-us-hello.wav")), pk.read_wav(os.path.join(GOLDEN, "en-us-cat.wav"))
    low = FA.wave_i16(8000, 77).astype(np.float32)                              # one second at 8 kHz
    waves, rates = [hello, cat, low], [16000, 16000, 8000]
    cap = sum(w.size for w in waves) * 2 + 1
    make = lambda: pk.BatchScorer(am, g, len(waves), cap, frontend=fe)
    bs = make()
    bs.set_waves(waves, rates)
    bs.score(0.1)
    fbank = [bs.fetch_fbank(u) for u in range(len(waves))]
    bs.close()
    glob = sum(NC.accumulate(f) for f in fbank)
    spk = [NC.accumulate(fbank[1])] * len(waves)
    for sname, spec in SPECS:
        if sname in ("speaker-vars-only", "online600"):
            continue
        want, recs = batch_reference(make, spec, glob, waves, spk, rates=rates)
        W = spec.cmn_window if is_online(spec) else 8
        sc = pk.OnlineScorer(am, g, 6, cap, frontend=fe)
        set_norm(sc, spec, glob)
        records = takes_records(spec)
        jobs = [dict(slot=0, kind="audio", data=hello, chunks=chunks_of(hello.size, 160 * 7, rng), spk=spk[0] if records else None, stats=records),
                dict(slot=1, kind="audio", data=cat, chunks=chunks_of(cat.size, 160 * (W + 1) + 13, rng), spk=spk[1] if records else None, stats=records),
                dict(slot=2, kind="audio", data=low, rate=8000, chunks=chunks_of(low.size, 799, rng), spk=spk[2] if records else None, stats=records),
                dict(slot=3, kind="raw", data=fbank[0], chunks=chunks_of(fbank[0].shape[0], "random", rng), spk=spk[0] if records else None, stats=records),
                dict(slot=0, kind="audio", data=cat, chunks=chunks_of(cat.size, "whole", rng), spk=spk[1] if records else None, stats=records)]
        # a NORMALIZED slot beside them: the batch scorer's normalised rows of `hello` (taken from a scorer in mode none)
        norm_rows = batch_normalized(make, spec, glob, waves, spk, rates)[0]
        jobs.append(dict(slot=4, kind="normalized", data=norm_rows, chunks=chunks_of(norm_rows.shape[0], 7, rng)))
        got = run(sc, jobs)
        for i, u in enumerate((0, 1, 2, 0, 1, 0)):
            assert NC.bits_equal(got[i][0], want[u]), "%s %s job %d: rows differ" % (name, sname, i)
            if records and jobs[i]["kind"] != "normalized":
                assert NC.bits_equal(got[i][1], recs[u]), "%s %s job %d: norm_stats differ" % (name, sname, i)
        sc.destroy()
    am.close()


def batch_normalized(make, spec, glob, waves, spk, rates):
    bs = make()
    set_norm(bs, spec, glob)
    if takes_records(spec):
        bs.set_speaker_stats(spk)
    bs.set_waves(waves, rates)
    bs.score(0.1)
    out = [bs.fetch_cmvn(u) for u in range(len(waves))]
    bs.close()
    return out


# ---------------------------------------------------------------- the default is the parent's path

def test_a_scorer_set_back_to_sliding_is_an_untouched_scorer():
    import cmvn_any_cases as CA
    rng = np.random.default_rng(3)
    for D in (40, 41):
        am, _, _ = tiny(D, L, R)
        g = CA.stats_for(D)
        raw = CA.features(650, D, 30)
        plain, back = (pk.OnlineFeatureScorer(am, 2, 700, global_stats=g) for _ in range(2))
        back.set_norm(pk.OnlineCmvnSpec(8, 3, 0, True))
        run(back, [dict(slot=0, kind="raw", data=raw, chunks=chunks_of(650, 100, rng))])
        back.set_norm(pk.NormSpec())
        chunks = chunks_of(650, 64, rng)
        a = run(plain, [dict(slot=0, kind="raw", data=raw, chunks=chunks)])[0][0]
        b = run(back, [dict(slot=0, kind="raw", data=raw, chunks=chunks)])[0][0]
        fs = pk.FeatureScorer(am, 1, 650, global_stats=g)
        fs.set_features([raw], "raw")
        fs.score(0.1)
        assert NC.bits_equal(a, b) and NC.bits_equal(a, fs.fetch(0).log_prob()), D
        assert code_of(lambda: back.norm_stats(0))[0] == E_STATE
        fs.close()
        plain.destroy()
        back.destroy()
        am.close()
    # audio
    am, _, _ = tiny(40, L, R)
    g = CA.stats_for(40)
    wave = FA.wave_i16(16000, 41).astype(np.float32)
    plain, back = (pk.OnlineScorer(am, g, 2, 20000) for _ in range(2))
    back.set_norm(pk.NormSpec("none"))
    run(back, [dict(slot=1, kind="audio", data=wave, chunks=chunks_of(wave.size, 1600, rng))])
    back.set_norm(pk.NormSpec("sliding", True, False))
    chunks = chunks_of(wave.size, 1234, rng)
    a = run(plain, [dict(slot=1, kind="audio", data=wave, chunks=chunks)])[0][0]
    b = run(back, [dict(slot=1, kind="audio", data=wave, chunks=chunks)])[0][0]
    bs = pk.BatchScorer(am, g, 1, 20000)
    bs.set_waves([wave])
    bs.score(0.1)
    assert NC.bits_equal(a, b) and NC.bits_equal(a, bs.fetch(0).log_prob())
    bs.close()
    plain.destroy()
    back.destroy()
    am.close()


# ---------------------------------------------------------------- isolation across slots

def test_poisoned_neighbours_across_slots_change_no_bit():
    D, T = 65, 70
    rng = np.random.default_rng(9)
    am, _, _ = tiny(D, L, R)
    x = NC.features(T, D, 7)
    glob = OC.record(NC.features(300, D, 3))
    spk = OC.record(NC.features(50, D, 100), OC.SPEAKER_COUNT)
    for spec in (pk.OnlineCmvnSpec(8, 3, 2, True), pk.NormSpec("speaker", True, True)):
        want, _ = batch_reference(lambda: pk.FeatureScorer(am, 1, T), spec, glob, [x], [spk], "raw")
        sc = pk.OnlineFeatureScorer(am, 3, 3 * T)
        set_norm(sc, spec, glob)
        nan, big = np.full((T, D), np.nan, np.float32), np.full((T, D), 1e30, np.float32)
        got = run(sc, [dict(slot=0, kind="raw", data=nan, chunks=chunks_of(T, 7, rng), spk=spk),
                       dict(slot=1, kind="raw", data=x, chunks=chunks_of(T, 7, rng), spk=spk),
                       dict(slot=2, kind="raw", data=big, chunks=chunks_of(T, 9, rng), spk=spk),
                       dict(slot=0, kind="raw", data=x, chunks=chunks_of(T, "random", rng), spk=spk)])     # reopened behind the NaNs
        assert np.isnan(got[0][0]).all()
        assert NC.bits_equal(got[1][0], want[0]) and NC.bits_equal(got[3][0], want[0]), spec
        sc.destroy()
    am.close()


# ---------------------------------------------------------------- failure codes

def test_failure_codes():
    D = 41
    am, _, _ = tiny(D, L, R)
    x = NC.features(20, D, 7)
    glob = OC.record(NC.features(300, D, 3))
    spk = OC.record(NC.features(50, D, 100), OC.SPEAKER_COUNT)
    sc = pk.OnlineFeatureScorer(am, 3, 100)
    lib, dp = pk.lib(), C.POINTER(C.c_double)
    # without a norm spec: RAW is refused, the norm entries have nothing to work on
    assert code_of(lambda: sc.open_features(0, "raw"))[0] == E_INVALID
    sc.open_features(0, "normalized")
    code, text = code_of(lambda: sc.set_norm(pk.NormSpec("none")))
    assert code == E_STATE and "slot 0" in text                                  # a slot is open
    assert code_of(lambda: sc.set_norm(pk.OnlineCmvnSpec(8, 3, 0)))[0] == E_STATE
    assert code_of(lambda: sc.set_speaker_stats(0, spk))[0] == E_STATE           # sliding
    assert code_of(lambda: sc.norm_stats(0))[0] == E_STATE
    sc.close(0)
    assert code_of(lambda: sc.set_norm(pk.NormSpec("none")))[0] == E_STATE       # closed, not yet flushed
    sc.step(0.1)
    # the spec's refusals
    code, text = code_of(lambda: sc.set_norm(pk.NormSpec("utterance", True, True)))
    assert code == E_INVALID and "utterance" in text and "live" in text
    for spec, word in ((pk.NormSpec(9), "mode"), (pk.NormSpec("speaker", False, False), "use mode none"), (pk.NormSpec("sliding", True, True), "norm_vars")):
        code, text = code_of(lambda: sc.set_norm(spec))
        assert code == E_INVALID and word in text
    for spec, g, word in ((pk.OnlineCmvnSpec(0), glob, "cmn_window"), (pk.OnlineCmvnSpec(8, -1, 2), glob, "speaker_frames"),
                          (pk.OnlineCmvnSpec(8, 3, 2, 2), glob, "norm_vars"), (pk.OnlineCmvnSpec(8, 3, 2), None, "global_frames")):
        code, text = code_of(lambda: sc.set_norm(spec, g))
        assert code == E_INVALID and word in text
    assert lib.pk_mi355_stream_norm_set(sc._h, None) == E_INVALID and lib.pk_mi355_stream_norm_set(None, None) == E_INVALID
    assert lib.pk_mi355_stream_norm_set_online_cmvn(sc._h, None, None) == E_INVALID
    assert code_of(lambda: sc.open_features(0, "raw"))[0] == E_INVALID           # the refused specs changed nothing
    # mode none: no records, no statistics
    sc.set_norm(pk.NormSpec("none"))
    sc.open_features(0, "raw")
    assert code_of(lambda: sc.set_speaker_stats(0, spk))[0] == E_STATE
    assert code_of(lambda: sc.norm_stats(0))[0] == E_STATE
    sc.close(0)
    sc.step(0.1)
    # mode speaker: the record is required, before the first frame, on an open RAW slot
    sc.set_norm(pk.NormSpec("speaker", True, True))
    assert code_of(lambda: sc.set_speaker_stats(1, spk))[0] == E_STATE           # not open
    sc.open_features(1, "raw")
    sc.open_features(2, "normalized")
    assert code_of(lambda: sc.set_speaker_stats(2, spk))[0] == E_STATE           # NORMALIZED: no norm applies
    assert code_of(lambda: sc.norm_stats(2))[0] == E_STATE
    sc.push_features(1, x)
    code, text = code_of(lambda: sc.step(0.1))
    assert code == E_STATE and "slot 1" in text and "pk_mi355_stream_norm_set_speaker_stats" in text
    for count in (0.0, -1.0, np.nan, np.inf):
        bad = spk.copy()
        bad[0, D] = count
        code, text = code_of(lambda: sc.set_speaker_stats(1, bad))
        assert code == E_INVALID and "count" in text, text
    assert code_of(lambda: sc.set_speaker_stats(1, spk[:, :-1]))[0] == E_INVALID   # the shape, refused in Python
    assert lib.pk_mi355_stream_norm_set_speaker_stats(sc._h, 1, None) == E_INVALID
    assert lib.pk_mi355_stream_norm_set_speaker_stats(sc._h, 3, spk.ctypes.data_as(dp)) == E_INVALID
    assert code_of(lambda: sc.step(0.1))[0] == E_STATE                           # the refused records handed nothing over
    sc.set_speaker_stats(1, spk)
    sc.step(0.1)                                                                 # the refused steps consumed nothing: 20 frames
    assert NC.bits_equal(sc.norm_stats(1), NC.accumulate(x))
    assert code_of(lambda: sc.set_speaker_stats(1, spk))[0] == E_STATE           # frames have been computed
    sc.close(1)
    sc.close(2)
    sc.step(0.1)
    assert NC.bits_equal(sc.norm_stats(1), NC.accumulate(x))                     # readable after the flush ...
    sc.open_features(1, "raw", speaker_stats=spk)
    assert NC.bits_equal(sc.norm_stats(1), np.zeros((2, D + 1)))                 # ... until the slot is opened again
    sc.close(1)
    sc.step(0.1)
    # online CMVN: records are optional; counts that are no counts are refused
    sc.set_norm(pk.OnlineCmvnSpec(8, 3, 2, True), glob)
    sc.open_features(0, "raw")
    for count in (-1.0, np.nan, np.inf):
        bad = spk.copy()
        bad[0, D] = count
        code, text = code_of(lambda: sc.set_speaker_stats(0, bad))
        assert code == E_INVALID and "count" in text, text
    sc.push_features(0, x)
    sc.close(0)
    sc.step(0.1)
    assert lib.pk_mi355_stream_norm_fetch_stats(sc._h, 0, None) == E_INVALID
    assert lib.pk_mi355_stream_norm_fetch_stats(sc._h, -1, np.zeros(2 * (D + 1)).ctypes.data_as(dp)) == E_INVALID
    assert lib.pk_mi355_stream_norm_fetch_stats(None, 0, np.zeros(2 * (D + 1)).ctypes.data_as(dp)) == E_INVALID
    assert NC.bits_equal(sc.norm_stats(0), NC.accumulate(x))
    sc.destroy()
    am.close()
