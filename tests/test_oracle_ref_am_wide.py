"""The oracle against the REAL reference acoustic path at wide feature dimensions, bit for bit (the checks and nets of
tests/test_oracle_ref_am.py, whose pin stops at D = 40): spliced inputs of more than one 512-chunk of k, odd
dimensions, contexts wider than the utterance.  tests/test_gpu_splice_wide.py holds the GPU to the oracle at these
widths; this holds the oracle to the reference's own code, both flavours.  CPU only; skipped where oracle/_ref was
never built."""
import numpy as np
import pytest

from oracle import oracle as O

from test_oracle_ref_am import check_am, small_net

pytestmark = pytest.mark.skipif(not O.have_ref_am(), reason="oracle/_ref/libpkref_am.so not built (needs the reference tree once)")

SHAPES = [(80, 5, 5), (130, 5, 5), (65, 4, 3), (43, 6, 5), (128, 1, 2), (130, 70, 3), (33, 7, 7)]
FRAMES = [1, 3, 47, 160]


@pytest.mark.parametrize("D,L,R", SHAPES)
def test_decodable_wide_feature_dims(D, L, R, tmp_path):
    rng = np.random.default_rng([0x41DE, D, L, R])
    layers, prior = small_net(rng, D, L, R)
    for i, T in enumerate(FRAMES):                          # T = 1 and T < L + R among them (splice edge replication)
        sub = tmp_path / str(i)
        sub.mkdir()
        check_am(sub, layers, prior, L, R, rng.standard_normal((T, D)).astype(np.float32))
