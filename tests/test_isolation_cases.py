"""The designed poisoned waves (tests/isolation_cases.py) without a GPU: the oracle's NaN pattern on every one of them is
the predicted one exactly, stage by stage; healthy utterances give no NaN; and where the live reference is built
(oracle/_ref/libpkref_am_ndebug.so: with assertions on a NaN reaching ApplyLog aborts the process, vector.cc:336) the
oracle equals it on the poisoned waves too, bit for bit.  test_gpu_isolation.py holds the GPU to the same predictions."""
import numpy as np
import pytest

from pocketkaldi_amd import synth
from oracle import oracle as O
from refmodel_files import write_model

import isolation_cases as C

G = synth.global_cmvn_stats()
DESIGNED = C.designed_waves()
IDS = [d[0] for d in DESIGNED]


def stages(wave, layers, prior, L, R):
    raw = O.Fbank().compute(wave)
    y = O.cmvn(G, raw)
    with np.errstate(invalid="ignore"):
        ll = O.Nnet(layers).am_compute(y, prior, L, R, 0.1)
    return raw, y, ll


def test_the_designed_layouts_and_waves():
    assert {k for _, k, _, _ in DESIGNED} == set(C.KINDS)
    for name, (_, layout, _) in C.LAYOUTS.items():
        for rot in C.ROTATIONS:
            utts = C.layout_utterances(name, rot)
            assert [C.frames_of(len(e["wave"])) for e in utts] == [T for T, _ in layout]
            assert [e["kind"] is not None for e in utts] == [bad for _, bad in layout]
        seen = [{C.layout_utterances(name, rot)[u]["kind"] for rot in C.ROTATIONS} for u, (_, bad) in enumerate(layout) if bad]
        assert all(s == set(C.KINDS) for s in seen), name          # every poisoned place sees every kind
    assert C.compact_rows(C.LAYOUT_C) >= 6144 and sum(len(e["wave"]) for e in C.layout_utterances("C", 0)) < 1.1e6
    for T in (3, 5, 130, 310, 333, 601, 887, 905):
        f0 = C.first_bad_frame(T)
        assert 0 < f0 < T and f0 % 4 and f0 % 64
        assert 160 * (f0 - 1) + 400 <= C.bad_sample(T) < 160 * f0 + 400 <= C.samples_for(T)       # frame f0 - 1 is clean
    assert sum(C.samples_for(T) for T in C.REUSE_POISON_FRAMES) == C.REUSE_CAP
    loud = C.poisoned("loud", 1, 130)[0]
    assert 2.5e4 < loud.std() < 3.5e4                                  # sigma 3e4, far outside 16-bit PCM


@pytest.mark.parametrize("name,kind,wave,pred", DESIGNED, ids=IDS)
def test_oracle_nan_pattern_is_the_predicted_one(name, kind, wave, pred):
    layers, prior, L, R = synth.model("tiny")
    raw, y, ll = stages(wave, layers, prior, L, R)
    assert raw.shape == y.shape == (pred.T, 40) and ll.shape == (pred.T, len(prior))
    C.assert_nan_rows(raw, pred.fbank, name + " fbank")
    C.assert_nan_rows(y, pred.cmvn, name + " cmvn")
    C.assert_nan_rows(ll, pred.loglik(R), name + " loglik")
    for a in (raw, y, ll):
        assert not np.isinf(a).any(), name
    if kind == "loud":
        assert not pred.fbank.any() and np.isfinite(ll).all()
        assert 10.0 < raw.min() and raw.max() < 35.0                   # (sigma 3e4: 16.9 .. 30.6 measured)


def test_oracle_nan_pattern_with_model_S_rows_of_layout_B():
    layers, prior, L, R = synth.model("S")
    for e in C.layout_utterances("B", 1):                               # nan_from at 333 frames, inf_one at 5
        if e["kind"]:
            _, _, ll = stages(e["wave"], layers, prior, L, R)
            C.assert_nan_rows(ll, e["pred"].loglik(R), "B %s" % e["kind"])


def test_healthy_utterances_have_no_nan():
    layers, prior, L, R = synth.model("tiny")
    waves = [e["wave"] for name in C.LAYOUTS for e in C.layout_utterances(name, 0) if e["kind"] is None]
    waves += [w for i in range(len(C.REUSE_LAYOUTS)) for w in C.reuse_healthy_waves(i)]
    waves += [w for s, w in enumerate(C.online_neighbour_waves("loud")[0]) if s != C.ONLINE_POISONED_SLOT]
    waves += [C.online_reuse_waves()[1], C.online_big_step_wave(), C.online_long_wave()]
    assert len(waves) > 30
    for w in waves:
        for a in stages(w, layers, prior, L, R):
            assert np.isfinite(a).all()


@pytest.mark.skipif(not O.have_ref_am(), reason="oracle/_ref/libpkref_am.so not built (needs the reference tree once)")
def test_oracle_equals_the_live_reference_on_the_poisoned_waves(tmp_path):
    layers, prior, L, R = synth.model("tiny")
    am = O.RefAm(write_model(tmp_path, layers, prior, L, R), ndebug=True)
    for name, kind, wave, pred in DESIGNED:
        raw, y, ll = stages(wave, layers, prior, L, R)
        ref_raw = O.ref_fbank(wave, ndebug=True)
        assert C.same_bits(raw, ref_raw), name + " fbank"
        ref_y = O.ref_cmvn(G, ref_raw, ndebug=True)
        assert C.same_bits(y, ref_y), name + " cmvn"
        assert C.same_bits(ll, am.decodable(ref_y, 0.1)), name + " loglik"
        C.assert_nan_rows(ref_raw, pred.fbank, name + " reference fbank")
        C.assert_nan_rows(ref_y, pred.cmvn, name + " reference cmvn")
