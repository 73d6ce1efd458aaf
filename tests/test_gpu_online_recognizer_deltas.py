"""The online recognizer and the online decoder behind delta features, on the two model files of
tests/test_gpu_recognize_deltas.py: a 39-dim model behind a 13-of-23 MFCC and a 120-dim one behind the reference's 40-bin
fbank, deltas and double deltas in between, cmvn_stats at the front-end's dimension.  The yardstick is
pk.Recognizer(..., deltas=) on the whole waves -- text, weight bits, segments and their costs -- and for the decoder
alone Decoder.decode_batch over BatchScorer(frontend=, deltas=)."""
import os
import shutil

import numpy as np
import pytest

import pocketkaldi_amd as pk

import refmodel_files as RF
from refmodel_text import load_text_model
from test_gpu_frontend_recognizer import CAT, DIR, HELLO, TRACE, comparable
from test_gpu_recognize_deltas import L, MODELS, R, model_layers

pytestmark = pytest.mark.gpu

E_INVALID, E_IO = -1, -3
M = 4                                                    # DeltaSpec(): order 2, window 2


@pytest.fixture(scope="module", params=sorted(MODELS))
def setup(request, tmp_path_factory):
    """The model file, the waves, the front-end's rows of each and the batch recognizer's Results (computed once)."""
    name = request.param
    tmp = tmp_path_factory.mktemp("online_recognizer_deltas_" + name)
    fe = pk.FrontendSpec() if MODELS[name] is None else pk.parse_frontend(MODELS[name])
    Db = fe.dim
    stats = np.concatenate([np.full(Db, (12.0 if MODELS[name] is None else 0.5) * 2500.0), [2500.0]]).astype(np.float32)
    layers, prior = model_layers(pk.DeltaSpec().dim(Db), len(name))
    tid2pdf = load_text_model()[4]
    conf = RF.write_model(tmp, layers, prior, L, R, tid2pdf=tid2pdf, cmvn_stats=stats)
    for f in ("wordloop.fst", "wordloop_words.bin"):
        shutil.copy(os.path.join(DIR, f), str(tmp / f))
    with open(conf, "a") as f:
        f.write("fst = wordloop.fst\nsymbol_table = wordloop_words.bin\n")
    waves = [pk.read_wav(HELLO), pk.read_wav(CAT)]
    frontend = None if MODELS[name] is None else fe
    rec = pk.Recognizer(conf, max_utts=2, max_total_samples=sum(len(w) for w in waves), trace_capacity=TRACE, frontend=frontend, deltas=pk.DeltaSpec())
    want = rec.process(waves)
    rows = [rec.batch.fetch_fbank(u) for u in range(2)]
    rec.close()
    front = pk.Frontend(fe)
    assert all(np.array_equal(front.compute(w).reshape(r.shape).view(np.uint32), r.view(np.uint32)) for w, r in zip(waves, rows))
    return dict(name=name, conf=conf, fe=fe, frontend=frontend, Db=Db, stats=stats, waves=waves, rows=rows, want=want,
                model=(layers, prior, tid2pdf))


def online_of(s, **kw):
    return pk.OnlineRecognizer(s["conf"], max_streams=2, max_step_samples=2 * 1600, trace_capacity=TRACE, frontend=s["frontend"],
                               deltas=pk.DeltaSpec(), **kw)


def stream(online, waves, chunk=1600, close_later=False):
    """Wave u into slot u, `chunk` samples a step, closed with its last chunk or in a step of its own -> the Results."""
    pos, live, out = [0] * len(waves), set(range(len(waves))), {}
    for u in live:
        online.open(u)
    while live:
        closing = []
        for u in sorted(live):
            if pos[u] < len(waves[u]):
                online.push(u, waves[u][pos[u]:pos[u] + chunk])
                pos[u] += chunk
                if close_later:
                    continue
            if pos[u] >= len(waves[u]):
                online.close(u)
                closing.append(u)
        online.step()
        for u in closing:
            assert online.finished(u)
            out[u] = online.result(u)
            live.discard(u)
    return [out[u] for u in range(len(waves))]


def test_online_recognizer_is_the_batch_recognizer(setup):
    s = setup
    online = online_of(s)
    assert (online.scorer.base_dim(), online.scorer.feat_dim()) == (s["Db"], 3 * s["Db"])
    for chunk, later in ((1600, False), (1237, True)):
        got = stream(online, s["waves"], chunk, later)
        for u in range(2):
            assert comparable(got[u]) == comparable(s["want"][u]), (s["name"], chunk, u)
            assert got[u].segments and all(np.isfinite(g.acoustic_cost) for g in got[u].segments)
    online.decoder.set_commit(True)                          # commit mode: the same Results
    got = stream(online, s["waves"])
    for u in range(2):
        assert comparable(got[u]) == comparable(s["want"][u]), ("commit", u)
    # the front-end's rows as RAW frames [n][Db], ten a step, into the same object
    for u in range(2):
        online.open_features(u, "raw")
    with pytest.raises(pk.PkCodeError) as e:                 # [n][feat_dim] frames are not a RAW slot's
        online.push_features(0, np.zeros((3, 3 * s["Db"]), np.float32))
    assert e.value.code == E_INVALID
    pos, live = [0, 0], {0, 1}
    while live:
        for u in sorted(live):
            online.push_features(u, s["rows"][u][pos[u]:pos[u] + 10])
            pos[u] += 10
            if pos[u] >= s["rows"][u].shape[0]:
                online.close(u)
        online.step()
        live = {u for u in live if pos[u] < s["rows"][u].shape[0]}
    for u in range(2):
        assert comparable(online.result(u)) == comparable(s["want"][u]), ("raw features", u)
    online.destroy()


def test_with_commit_and_endpointing_audio_and_raw_slots_are_cut_alike(setup):
    """A rule that fires on every utterance 30 frames long: slot 0 takes the wave 100 ms a step, slot 1 the front-end's rows
    of the same wave, as many a step as slot 0's audio completed -- the same utterances, cut at the same frames."""
    s = setup
    online = online_of(s)
    online.set_endpointing([10], [pk.EndpointRule(False, 0.0, np.inf, 0.30)])
    online.decoder.set_commit(True)
    for u, (wave, rows) in enumerate(zip(s["waves"], s["rows"])):
        online.open(0)
        online.open_features(1, "raw")
        pos = fed = 0
        while pos < len(wave):
            online.push(0, wave[pos:pos + 1600])
            pos = min(pos + 1600, len(wave))
            n = pk.num_frames(pos)
            online.push_features(1, rows[fed:n])
            fed = n
            if pos == len(wave):
                online.close(0)
                online.close(1)
            online.step()
            if pos < len(wave):
                assert online.decoder.num_frames(0) == online.decoder.num_frames(1)
                assert online.partial(0) == online.partial(1) and online.stable(0) == online.stable(1)
        assert fed == rows.shape[0] and online.finished(0) and online.finished(1)
        a, b = online.utterances(0), online.utterances(1)
        assert [(p.first_frame, p.num_frames, p.rule) for p in a] == [(p.first_frame, p.num_frames, p.rule) for p in b]
        assert len(a) >= 2 and a[-1].rule == 0 and all(p.rule == 1 for p in a[:-1])
        assert sum(p.num_frames for p in a) == rows.shape[0]
        # (an open slot decodes up to frame n - M - R: the first cut comes M frames later than without deltas)
        assert all(p.num_frames >= 30 for p in a[:-1])
        assert [comparable(p.result) for p in a] == [comparable(p.result) for p in b], u
        assert comparable(online.result(0)) == comparable(online.result(1)) == comparable(a[-1].result)
    online.destroy()


def test_online_decoder_advance_over_a_deltas_scorer(setup):
    s = setup
    layers, prior, tid2pdf = s["model"]
    am = pk.AcousticModel(layers, prior, L, R, tid2pdf)
    fst = pk.Fst(os.path.join(DIR, "wordloop.fst"))
    waves = s["waves"]
    bs = pk.BatchScorer(am, s["stats"], 2, sum(len(w) for w in waves), frontend=s["fe"], deltas=pk.DeltaSpec())
    bs.set_waves(waves)
    bs.score(0.1)
    dec = pk.Decoder(fst, am, 2)
    dec.decode_batch(bs)
    want = [dec.result(u) for u in range(2)]
    sc = pk.OnlineScorer(am, s["stats"], 2, 2 * 1600, frontend=s["fe"], deltas=pk.DeltaSpec())
    od = pk.OnlineDecoder(fst, am, 2)
    pos, live = [0, 0], {0, 1}
    for u in live:
        sc.open(u)
        od.open(u)
    while live:
        for u in sorted(live):
            sc.push(u, waves[u][pos[u]:pos[u] + 1600])
            pos[u] += 1600
            if pos[u] >= len(waves[u]):
                sc.close(u)
                live.discard(u)
        sc.step(0.1, sync=False)
        od.advance(sc)
    for u in range(2):
        words, weight, ok = od.result(u)
        assert (words, ok) == (want[u][0], want[u][2]) and np.float32(weight).tobytes() == np.float32(want[u][1]).tobytes(), u
        assert od.num_frames(u) == bs.num_frames(u)
    for o in (od, sc):
        o.destroy()
    for o in (dec, bs, fst, am):
        o.close()


def test_refusals_are_the_stream_entry_s(setup):
    s = setup
    with pytest.raises(pk.PkCodeError) as e:                 # order 1 makes two blocks of a three-block model
        pk.OnlineRecognizer(s["conf"], frontend=s["frontend"], deltas=pk.DeltaSpec(1, 2))
    if s["Db"] == 13:                                        # 39 / 2: the create entry's refusal
        assert e.value.code == E_INVALID and "2 blocks" in str(e.value) and "39" in str(e.value)
    else:                                                    # 120 / 2 = 60: the model file's cmvn_stats are not at 60
        assert e.value.code == E_IO and "2 delta blocks" in str(e.value) and "61" in str(e.value)
    with pytest.raises(pk.PkCodeError) as e:
        pk.OnlineRecognizer(s["conf"], frontend=s["frontend"], deltas=pk.DeltaSpec(4, 2))
    assert e.value.code == E_INVALID and "order" in str(e.value)
    with pytest.raises(pk.PkCodeError) as e:                 # a front-end of another dimension than Db
        pk.OnlineRecognizer(s["conf"], frontend=pk.FrontendSpec(num_mel_bins=80), deltas=pk.DeltaSpec())
    assert e.value.code == E_INVALID
