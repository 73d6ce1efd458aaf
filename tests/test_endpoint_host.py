"""The host half of endpointing through the C ABI (the library loads without a GPU): pk_mi355_endpoint_eval against a
table, pk_mi355_endpoint_default_rules, and the argument errors that are found before the device is touched."""
import ctypes as C

import numpy as np
import pytest

import pocketkaldi_amd as pk

INF = float("inf")
E_INVALID = -1
DEFAULT = [(0, 500, INF, 0), (1, 50, 2.0, 0), (1, 100, 8.0, 0), (1, 200, INF, 0), (0, 0, INF, 2000)]


def rules_of(table):
    arr = (pk.pk_mi355_endpoint_rule_t * max(len(table), 1))()
    for i, (must, trail, cost, length) in enumerate(table):
        arr[i].must_contain_nonsilence, arr[i].min_trailing_silence_frames = must, trail
        arr[i].max_relative_cost, arr[i].min_utterance_frames = cost, length
    return arr


def ev(table, frames, trailing, cost):
    return pk.lib().pk_mi355_endpoint_eval(rules_of(table), len(table), frames, trailing, cost)


def up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def test_default_rules():
    arr = (pk.pk_mi355_endpoint_rule_t * 5)()
    assert pk.lib().pk_mi355_endpoint_default_rules(arr, 5) == 5
    got = [(r.must_contain_nonsilence, r.min_trailing_silence_frames, r.max_relative_cost, r.min_utterance_frames) for r in arr]
    assert got == DEFAULT
    assert pk.lib().pk_mi355_endpoint_default_rules(None, 0) == 5
    two = (pk.pk_mi355_endpoint_rule_t * 5)()
    assert pk.lib().pk_mi355_endpoint_default_rules(two, 2) == 5
    assert two[1].min_trailing_silence_frames == 50 and two[2].min_trailing_silence_frames == 0       # two written
    assert pk.endpoint_default_rules() == [pk.EndpointRule(False, 5.0, INF, 0.0), pk.EndpointRule(True, 0.5, 2.0, 0.0),
                                           pk.EndpointRule(True, 1.0, 8.0, 0.0), pk.EndpointRule(True, 2.0, INF, 0.0),
                                           pk.EndpointRule(False, 0.0, INF, 20.0)]


# (frames, trailing, relative cost) -> rule, on the default rules: each rule alone, and just missing
TABLE = [
    ((500, 500, INF), 1),            # rule 1: silence only, 5 s of it
    ((499, 499, INF), 0),            # one frame short (and no speech: rules 2 - 4 stay quiet)
    ((1999, 199, INF), 0),           # speech, but no final token, not yet 200 frames of silence
    ((60, 50, 2.0), 2),              # rule 2: speech, 50 frames, cost 2.0
    ((60, 49, 2.0), 0),              # one frame short
    ((60, 50, up(2.0)), 0),          # the next float above 2.0 (rule 3 needs 100 frames)
    ((50, 50, 2.0), 0),              # the utterance is all silence
    ((51, 50, 2.0), 2),              # one frame of speech
    ((120, 100, 8.0), 3),            # rule 3
    ((120, 99, 8.0), 0),
    ((120, 100, up(8.0)), 0),
    ((120, 100, up(2.0)), 3),        # past rule 2's cost only
    ((300, 200, INF), 4),            # rule 4: +inf against max = +inf fires
    ((300, 199, INF), 0),
    ((300, 199, up(8.0)), 0),
    ((200, 200, 0.0), 0),            # all silence: rules 2 - 4 quiet, rule 1 needs 500
    ((2000, 0, INF), 5),             # rule 5
    ((1999, 0, INF), 0),
    ((2000, 500, 0.0), 1),           # order: the first of several
    ((2000, 300, 0.0), 2),
    ((2000, 300, 5.0), 3),
    ((2000, 300, 9.0), 4),
    ((2000, 10, 0.0), 5),
    ((0, 0, 0.0), 0),                # nothing fires at frames == 0 ...
]


@pytest.mark.parametrize("case, want", TABLE)
def test_eval_table(case, want):
    assert ev(DEFAULT, *case) == want
    assert pk.endpoint_eval(pk.endpoint_default_rules(), *case) == want


def test_eval_edges():
    assert ev([(0, 0, INF, 0)], 0, 0, 0.0) == 0                       # ... whatever the rule
    assert ev([(0, 0, INF, 0)], 1, 0, 0.0) == 1
    assert ev([(1, 100, 8.0, 0)], 300, 200, INF) == 0                 # +inf against 8.0
    assert ev([(1, 100, INF, 0)], 300, 200, INF) == 1
    assert ev([(0, 0, INF, 0)], 5, 0, float("nan")) == 0              # a NaN cost is below nothing
    assert ev([], 100, 100, 0.0) == 0                                 # num_rules = 0
    assert pk.lib().pk_mi355_endpoint_eval(None, 3, 100, 100, 0.0) == 0
    assert ev([(0, 5, INF, 0), (0, 5, INF, 0)], 9, 5, 0.0) == 1       # the first of two equal rules
    assert ev([(0, 6, INF, 0), (0, 5, INF, 0)], 9, 5, 0.0) == 2
    assert pk.endpoint_eval([], 10, 10, 0.0) == 0
    assert pk.endpoint_eval([pk.EndpointRule(True, 0.07, 1.5, 0.0)], 9, 7, 1.5) == 1          # int(round(s * 100))
    assert pk.endpoint_eval([pk.EndpointRule(True, 0.07, 1.5, 0.0)], 9, 6, 1.5) == 0


def test_argument_errors_before_the_device():
    L = pk.lib()
    rules = rules_of(DEFAULT)
    sil = (C.c_int32 * 1)(0)
    assert L.pk_mi355_online_decoder_set_endpointing(None, sil, 1, rules, 5) == E_INVALID
    assert "null online decoder" in L.pk_mi355_last_error().decode()
    assert L.pk_mi355_online_decoder_endpoint(None, 0, None) == E_INVALID
    assert L.pk_mi355_online_decoder_finish(None, None, 0, 1) == E_INVALID
