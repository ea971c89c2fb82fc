"""The directed pictures of tests/deblock_directed.py through recon_chain_kernel (ReconSession): one session a family, one chain a
picture, every padded plane of every picture against the oracle, bit for bit.  tests/test_deblock_directed.py shows (CPU) which
thresholds, table entries, QP lookups, short cuts and orders of filtering the pictures reach.  The order and slice families run again
with 1, 2 and 3 waves, four replicas each."""
import pytest

import deblock_directed as DD
import test_recon_directed_gpu as R          # _run / _check: the comparison and its report, shared

pytestmark = pytest.mark.gpu

_families = {}


def _named(family):
    if not _families:
        _families.update(DD.families())
    return [(s.name, s.frames()) for s in _families[family]]


@pytest.fixture(autouse=True)
def _no_wave_override(monkeypatch):
    monkeypatch.delenv("LH264_WAVES", raising=False)


@pytest.mark.parametrize("family", ["ABCD", "E", "F", "G", "H", "I", "J"])
def test_family(family):
    """A-D: every gate, clip and choice of filter_edge at and one short of its threshold; E: every entry of the alpha, beta and tc0
    tables under the inner, left and top lookup; F: the three QPs apart; G: the stale tc0; H: the scalar short cuts and mixed
    strengths; I: lines that read what earlier filters wrote; J: slices"""
    R._run(_named(family))


@pytest.mark.parametrize("waves", [1, 2, 3])
@pytest.mark.parametrize("family", ["I", "J"])
def test_order_and_slices_by_wave_count(family, waves, monkeypatch):
    """the carry between macroblocks and rows (lfY / lfC, fTop / fCur, wait_row_above) with rows shared out over 1, 2 and 3 waves"""
    monkeypatch.setenv("LH264_WAVES", str(waves))
    R._run(_named(family), replicate=4)
