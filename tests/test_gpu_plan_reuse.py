"""One features batch walked through every cell of the batch plan ("The two plans"): source raw or
normalised x mode none, utterance, speaker, online CMVN, sliding, in two different orders, speaker records handed over
where the mode takes them.  After every cell fetch_cmvn and the log-likelihood rows equal, bit for bit, those of a
fresh object that was scored in that one cell only: the shared raw, normalised and delta rows make every call a
function of its own inputs, whatever mode and source the call before it ran in.  (The fresh objects are anchored to
the host rules by test_gpu_norm, test_gpu_online_cmvn, test_gpu_deltas and test_gpu_cmvn_any.)
Two shapes, a 16-pdf linear + softmax model with L = R = 2 each: D = 40 without deltas (sliding: the fused CmvnKernel)
and Db = 8 with deltas of order 1, D = 16 (sliding: the chain); utterances of 1, 5 and 70 frames (70 crosses a 64-frame
tile)."""
import numpy as np
import pytest

import pocketkaldi_amd as pk

import cmvn_any_cases as CA
import norm_cases as NC
from test_cpp_ark_features import weight
from test_gpu_cmvn_any import fetch_rows

pytestmark = pytest.mark.gpu

L, R, N = 2, 2, 16
FRAMES = [1, 5, 70]
MODES = ["none", "utterance", "speaker", "online", "sliding"]
CELLS = [(source, mode) for source in ("raw", "normalized") for mode in MODES]
ORDERS = [CELLS, CELLS[::-1][1::2] + CELLS[::2] + CELLS[::-1][0::2] + CELLS[1::2]]     # every cell twice in the second one
SHAPES = {"D40": (40, None), "Db8-deltas": (8, (1, 2))}


class Shape:
    def __init__(self, Db, deltas):
        self.Db, self.spec = Db, pk.DeltaSpec(*deltas) if deltas else None
        D = self.D = self.spec.dim(Db) if deltas else Db
        K = D * (L + R + 1)
        self.am = pk.AcousticModel([("linear", weight(np.arange(N * K)).reshape(N, K), weight(1000003 + np.arange(N))), ("softmax",)],
                                   np.full(N, 1.0 / N, np.float32), L, R)
        self.g = CA.stats_for(Db)
        self.raw = [NC.features(T, Db, 40 + u) for u, T in enumerate(FRAMES)]
        self.normalized = [NC.features(T, D, 60 + u) for u, T in enumerate(FRAMES)]
        rec = [NC.accumulate(x) for x in self.raw]
        self.spk = [r + rec[2] for r in rec]
        self.want = {cell: self.run(self.scorer(), cell) for cell in CELLS}      # computed once, left unchanged

    def scorer(self):
        return pk.FeatureScorer(self.am, len(FRAMES), sum(FRAMES), global_stats=self.g, deltas=self.spec)

    def run(self, fs, cell):
        source, mode = cell
        fs.set_norm(pk.OnlineCmvnSpec(8, 600, 0, True) if mode == "online" else pk.NormSpec(mode, True, mode in ("utterance", "speaker")))
        if mode in ("speaker", "online"):
            fs.set_speaker_stats(self.spk)
        fs.set_features(self.raw if source == "raw" else self.normalized, source)
        fs.score(0.1)
        return [fs.fetch_cmvn(u) for u in range(len(FRAMES))], fetch_rows(fs)


_shapes = {}


def shape(name):
    if name not in _shapes:
        _shapes[name] = Shape(*SHAPES[name])
    return _shapes[name]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_cell_on_one_batch_equals_a_fresh_object(name, order):
    s = shape(name)
    assert len(ORDERS[1]) == 2 * len(CELLS) and set(ORDERS[1]) == set(CELLS) and ORDERS[1][:len(CELLS)] != CELLS
    fs = s.scorer()
    assert (fs.base_dim(), fs.feat_dim()) == (s.Db, s.D)
    for step, cell in enumerate(ORDERS[order]):
        rows, ll = s.run(fs, cell)
        want_rows, want_ll = s.want[cell]
        for u, T in enumerate(FRAMES):
            assert rows[u].shape == (T, s.D) and ll[u].shape == (T, N)
            assert NC.bits_equal(rows[u], want_rows[u]), "%s step %d %s utterance %d: fetch_cmvn differs from the fresh object's" % (name, step, cell, u)
            assert NC.bits_equal(ll[u], want_ll[u]), "%s step %d %s utterance %d: log-likelihoods differ from the fresh object's" % (name, step, cell, u)
    # the cells are different computations: the comparison above is not one of equal constants
    for mode in MODES[1:]:
        assert not NC.bits_equal(s.want[("raw", mode)][0][2], s.want[("raw", "none")][0][2]), mode
    assert all(NC.bits_equal(s.want[("normalized", mode)][1][2], s.want[("normalized", "none")][1][2]) for mode in MODES)
    fs.close()
