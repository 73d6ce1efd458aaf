"""Every refusal of the twelve scorer create entries and the eight recognizer load entries that is reachable without a
device: the model null, f32 or f16 and never finalized; every pointer an entry takes null; one bad
field per spec kind, a few fields each, as the host tests of the single entries choose them; for the load entries a model
file that does not exist and the three bad capacities.  A case is a model (a load entry: none) and none, one or two of
the entry's faults on the same call, two never on the same argument.

    python tests/create_refusal_cases.py

writes tests/golden/create_refusals.json, entry -> case id -> [code, text], from the library it finds.  The committed
file was written by the library as it stood before the create paths were folded into one;
tests/test_create_refusals_host.py holds the library to it row by row."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import pocketkaldi_amd as pk

import frontend_any_cases as FA
import transform_cases as TC

GOLDEN = os.path.join(HERE, "golden", "create_refusals.json")
MISSING = b"no-such-dir/missing.conf"                   # (relative: the text that names it is the same everywhere)
MODELS = {"null": None, "f32": 0, "f16": 1}             # no model; PK_MI355_PRECISION_F32, _F16X3, created and never finalized
f32p = C.POINTER(C.c_float)

_M = TC.matrix(13, 3, 3, 40, True)
_NONFINITE = _M.copy()
_NONFINITE[2, 5] = np.inf
# the good specs fit one another (a 13-dim front-end, a 13-dim transform input); no model here is finalized, so nothing
# compares them with a model
GOOD = {"frontend": FA.SPECS[9], "deltas": pk.DeltaSpec(2, 2), "transform": pk.TransformSpec(_M, 3, 3)}
BAD = {
    "frontend": {"bins129": FA.S(bins=129), "ceps24of23": FA.S("mfcc", 23, 24), "band": FA.S(low=4000.0, high=4000.0)},
    "deltas": {"order4": pk.DeltaSpec(4, 2), "window0": pk.DeltaSpec(2, 0)},
    "transform": {"left17": pk.TransformSpec(_M, 17, 0, in_dim=13), "cols": pk.TransformSpec(_M, 3, 3, in_dim=12),
                  "nomatrix": pk.TransformSpec(None, 1, 0, in_dim=13), "nonfinite": pk.TransformSpec(_NONFINITE, 3, 3)},
}
CAPACITIES = {"units": (2, 0), "cap": (1600, 0), "trace": (0, -1)}          # argument -> (good, bad)

# entry -> its arguments in order.  "stats41": a pointer alone; "stats": a pointer and its length.
CREATE = {}
for _kind in ("batch", "stream"):
    CREATE.update({
        "pk_mi355_%s_create" % _kind: ("am", "stats41", "units", "cap"),
        "pk_mi355_features_%s_create" % _kind: ("am", "stats41", "units", "cap"),
        "pk_mi355_features_%s_create_stats" % _kind: ("am", "stats", "units", "cap"),
        "pk_mi355_frontend_%s_create" % _kind: ("am", "frontend", "stats", "units", "cap"),
        "pk_mi355_deltas_%s_create" % _kind: ("am", "deltas", "frontend", "stats", "units", "cap"),
        "pk_mi355_transform_%s_create" % _kind: ("am", "transform", "deltas", "frontend", "stats", "units", "cap"),
    })
LOAD = {}
for _live, _head in ((False, ("precision",)), (True, ())):
    _name = "pk_mi355_%s" + ("online_recognizer_load" if _live else "recognizer_load")
    _tail = _head + ("units", "cap", "trace")
    LOAD.update({
        _name % "": ("path",) + _tail,
        _name % "frontend_": ("path", "frontend") + _tail,
        _name % "deltas_": ("path", "frontend", "deltas") + _tail,
        _name % "transform_": ("path", "frontend", "deltas", "transform") + _tail,
    })
ENTRIES = dict(CREATE, **LOAD)
assert len(CREATE) == 12 and len(LOAD) == 8


def faults(entry):
    """[(argument, what)]: what is "null", the name of a bad spec, or "bad" for a capacity."""
    out = []
    for arg in ENTRIES[entry]:
        if arg in ("stats41", "stats", "path"):
            out.append((arg, "null"))
        elif arg in BAD:
            out += [(arg, "null")] + [(arg, name) for name in BAD[arg]]
        elif arg in CAPACITIES and entry in LOAD:
            out.append((arg, "bad"))
    return out


def cases(entry):
    """[(case id, model, faults)] in a fixed order: every model (a load entry: "-") x none, one or two faults."""
    fs = faults(entry)
    sets = [()] + [(f,) for f in fs] + [p for p in itertools.combinations(fs, 2) if p[0][0] != p[1][0]]
    out = []
    for model in (MODELS if entry in CREATE else ("-",)):
        for chosen in sets:
            out.append(("model=%s" % model + "".join(",%s=%s" % f for f in chosen), model, chosen))
    return out


def run(entry, model, chosen):
    """The call with the chosen faults -> (code, text); the entry must refuse it."""
    L = pk.lib()
    chosen = dict(chosen)
    keep, args = [], []
    am = None
    if model in ("f32", "f16"):
        am = L.pk_mi355_am_create()
        assert am and L.pk_mi355_am_set_precision(am, MODELS[model]) == 0
    try:
        for arg in ENTRIES[entry]:
            what = chosen.get(arg)
            if arg == "am":
                args.append(am)
            elif arg == "path":
                args.append(None if what else MISSING)
            elif arg == "precision":
                args.append(0)
            elif arg in ("stats41", "stats"):
                g = np.zeros(41 if arg == "stats41" else 14, np.float32)
                keep.append(g)
                args.append(None if what else g.ctypes.data_as(f32p))
                if arg == "stats":
                    args.append(0 if what else g.size)
            elif arg in GOOD:
                spec = None if what == "null" else (BAD[arg][what] if what else GOOD[arg]).struct()
                keep.append(spec)
                args.append(None if spec is None else C.byref(spec))
            else:
                args.append(CAPACITIES[arg][1 if what else 0])
        handle = getattr(L, entry)(*args)
        assert not handle, (entry, model, chosen)
        return L.pk_mi355_last_error_code(), L.pk_mi355_last_error().decode()
    finally:
        if am:
            L.pk_mi355_am_destroy(am)


def table():
    return {entry: {cid: list(run(entry, model, chosen)) for cid, model, chosen in cases(entry)} for entry in sorted(ENTRIES)}


if __name__ == "__main__":
    rows = table()
    with open(GOLDEN, "w") as f:            # one row a line
        f.write("{\n" + ",\n".join(' %s: {\n%s\n }' % (json.dumps(entry), ",\n".join("  %s: %s" % (json.dumps(cid), json.dumps(row)) for cid, row in got.items()))
                                   for entry, got in rows.items()) + "\n}\n")
    print("%s: %d entries, %d rows" % (GOLDEN, len(rows), sum(len(got) for got in rows.values())))
