"""The directed intra pictures of tests/intra_directed.py through recon_chain_kernel (ReconSession): one session a family, one chain a
picture, every padded plane of every picture against the oracle, bit for bit.  tests/test_intra_directed.py shows (CPU) which
cells the pictures reach, that the oracle equals an independent model on them, and that the model's wrong variants differ there.
The I4x4, I8x8 and position families run once more on one wave, where the top edge of every macroblock row comes through the line
slots, four replicas each."""
import pytest

import intra_directed as ID
import test_recon_directed_gpu as R          # _run / _check: the comparison and its report, shared

pytestmark = pytest.mark.gpu


def _named(family):
    return [(c.name, c.frames()) for c in ID.families()[family]]


@pytest.fixture(autouse=True)
def _no_wave_override(monkeypatch):
    monkeypatch.delenv("LH264_WAVES", raising=False)


@pytest.mark.parametrize("family", ["i4", "i8", "i16c", "pos", "res", "filtered"])
def test_family(family):
    """i4: every (mode, block) and the *_TOP modes beside real top-right samples; i8: every (mode, block, top-left, top-right) of the
    edge filter; i16c: I16x16 and chroma, plane predictors at +-9180 / +-2550 and at both clips, chroma DC sums that all differ; pos:
    column 0, the last column, row 0, the first macroblock of a slice mid-row, below a slice boundary; res: prediction + residual
    beyond both ends of 8 bits in all four phases; filtered: everything without residual under the strongest in-loop filter"""
    R._run(_named(family))


@pytest.mark.parametrize("family", ["i4", "i8", "pos"])
def test_family_on_one_wave(family, monkeypatch):
    monkeypatch.setenv("LH264_WAVES", "1")
    R._run(_named(family), replicate=4)
