"""The inputs of tests/recon_stages.py:mc_stage_cases through recon_chain_kernel: one ReconSession, a chain per case, every padded
plane of every picture against the oracle, bit for bit.  Mixed fraction classes inside one wave are the point: the luma motion
compensation runs by stages that the lanes share (mc_luma_rows).  tests/test_recon_mc_stages.py shows (CPU) what the inputs hold."""
import pytest

import recon_stages as S
from test_recon_directed_gpu import _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return S.mc_stage_cases()


@pytest.fixture(autouse=True)
def _no_wave_override(monkeypatch):
    monkeypatch.delenv("LH264_WAVES", raising=False)


@pytest.mark.parametrize("kind", ["a", "b", "c", "d", "e"])
def test_mc_stages(cases, kind):
    """a: the four classes over the four 8x8 partitions; b: every ordered pair of positions in P16x8; c: all 16 positions in sixteen
    4x4 partitions; d: a under weighted prediction; e: fy == 0 everywhere with mixed fx (one row fetched)"""
    sel = [(c.name, c.frames) for c in cases if c.kind == kind]
    assert len(sel) == {"a": 512, "b": 512, "c": 8, "d": 512, "e": 48}[kind]
    _run(sel)
