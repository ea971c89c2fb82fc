"""The inputs of tests/recon_stages.py:bs_lane_cases through recon_chain_kernel: one ReconSession, a chain per case, every padded
plane of every picture against the oracle, bit for bit.  They cover what tests/recon_directed.py:bs_thresholds does not hold of the
boundary strengths: the 8x8 transform inside the macroblock, intra on either side, a macroblock without neighbours, slice borders
under deblock_idc 2, a concealed neighbour, counts on one side of an edge, P8x8REF0 and SKIP.  tests/test_recon_bs_lanes.py shows
(CPU) that each case's edge is, or is not, filtered."""
import pytest

import recon_directed as D
import recon_stages as S
from test_recon_directed_gpu import _check, _oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_wave_override(monkeypatch):
    monkeypatch.delenv("LH264_WAVES", raising=False)


def test_bs_lanes():
    import losslessh264_amd as lh
    cases = S.bs_lane_cases()
    assert len(cases) == 77
    for c in cases:
        D.check_refs_defined(c.frames)
    sess = lh.ReconSession([c.frames for c in cases])
    sess.run(); sess.synchronize()
    assert sess.n_chains == len(cases)
    for i, c in enumerate(cases):
        _check(sess, i, c.frames, _oracle("bs_lanes " + c.name, c.oracle_frames), "bs_lanes " + c.name)
