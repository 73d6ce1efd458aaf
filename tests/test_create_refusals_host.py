"""CPU-only: the refusals of the twelve create entries and the eight load entries that are said without a device
(tests/create_refusal_cases.py), row by row what the library said before its create paths were folded into one request
and one check order (tests/golden/create_refusals.json).  The rows that differ are the two
accepted meetings of two faults that a model without a device can reach, written out below; every other row, every
single fault among them, is the golden file's."""
import json

import pytest

import create_refusal_cases as RC

E_INVALID, E_STATE = -1, -4
F16_REFUSED = [E_INVALID, "the online scorer runs f32 models only (the f16 modes' calibration and range verdict are per batch)"]
NOT_FINALIZED = [E_STATE, "model not finalized"]
WAS = {"f32": NOT_FINALIZED, "f16": F16_REFUSED}            # what these rows said: the model's refusal
FRONTEND_WORDS = {
    "bins129": "front-end spec: num_mel_bins 129 is outside 3 .. 128",
    "ceps24of23": "front-end spec: num_ceps 24 is outside 1 .. num_mel_bins = 23",
    "band": "front-end spec: high_freq resolves to 4000 Hz: it must be above low_freq = 4000 and at most 8000",
}
# (entry, case id) -> (what the golden file holds, what the library says now)
ACCEPTED = {}
for _model, _was in WAS.items():
    # 1. pk_mi355_features_stream_create_stats: null statistics are named before the model is looked at
    ACCEPTED[("pk_mi355_features_stream_create_stats", "model=%s,stats=null" % _model)] = (_was, [E_INVALID, "null argument"])
    # 2. pk_mi355_deltas_stream_create, pk_mi355_transform_stream_create: a bad front-end spec is named before the model
    #    is looked at, as pk_mi355_frontend_stream_create names it (a null deltas spec is no fault of the transform entry)
    for _bad, _words in FRONTEND_WORDS.items():
        for _entry, _between in (("pk_mi355_deltas_stream_create", ""), ("pk_mi355_transform_stream_create", ""),
                                 ("pk_mi355_transform_stream_create", "deltas=null,")):
            ACCEPTED[(_entry, "model=%s,%sfrontend=%s" % (_model, _between, _bad))] = (_was, [E_INVALID, _words])


@pytest.fixture(scope="module")
def golden():
    with open(RC.GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_every_case_and_the_accepted_rows_as_they_were(golden):
    assert sorted(golden) == sorted(RC.ENTRIES)
    for entry in RC.ENTRIES:
        assert list(golden[entry]) == [cid for cid, _, _ in RC.cases(entry)], entry
    assert len(ACCEPTED) == 2 * (1 + 3 * 3)
    for (entry, cid), (was, _) in ACCEPTED.items():
        assert golden[entry][cid] == was, (entry, cid)


def test_every_fault_alone_is_a_row():
    """Each of the entry's faults has a row of its own under every model (a load entry: under none), and so has every
    pair of faults that are not on the same argument."""
    for entry in RC.ENTRIES:
        fs, ids = RC.faults(entry), {cid for cid, _, _ in RC.cases(entry)}
        for model in (RC.MODELS if entry in RC.CREATE else ("-",)):
            assert "model=%s" % model in ids
            for i, f in enumerate(fs):
                assert "model=%s,%s=%s" % ((model,) + f) in ids
                for g in fs[i + 1:]:
                    assert (f[0] == g[0]) != ("model=%s,%s=%s,%s=%s" % ((model,) + f + g) in ids)


@pytest.mark.parametrize("entry", sorted(RC.ENTRIES))
def test_refusals_are_the_golden_rows(entry, golden):
    differing = []
    for cid, model, chosen in RC.cases(entry):
        got = list(RC.run(entry, model, chosen))
        print(entry, cid, got)
        want = ACCEPTED[(entry, cid)][1] if (entry, cid) in ACCEPTED else golden[entry][cid]
        if got != want:
            differing.append((cid, got, want))
    assert not differing, differing[:10]
