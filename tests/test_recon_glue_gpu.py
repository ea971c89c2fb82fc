"""The glue of the reconstruct kernel's macroblock loop through recon_chain_kernel (ReconSession): the inputs of
tests/recon_glue_cases.py, every padded plane of every picture against the oracle, bit for bit.  They aim at the predicates and
addresses of the moves between the tile, the carry, the row buffers and the picture (a left neighbour, a row above, the last column,
the last row), at the job flags, at a macroblock no slice covers and at the single / triple threshold lookup of the in-loop filter.
tests/test_recon_glue.py shows (CPU) that the inputs reach what they claim."""
import numpy as np
import pytest

import oracle_lib as O
import recon_glue_cases as G
import recon_directed as D

pytestmark = pytest.mark.gpu

_oracle_cache = {}


def _oracle(key, frames, flags=0):
    """the chain through the oracle with the job's flags, once per input (the pictures are compared, never written)"""
    if key not in _oracle_cache:
        pics, out = {}, []
        for f in frames:
            dst = O.HostPic(f.mb_w, f.mb_h)
            O.recon_frame(f.mbs, f.coeffs, f.slices, dst, [pics[r] for r in f.ref_ids], flags)
            pics[f.id] = dst
            out.append(dst)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def _check(sess, chain, frames, want, label):
    for i, f in enumerate(frames):
        got = sess.picture(chain, i, padded=True)
        for p in range(3):
            ref = want[i].padded_plane(p)
            if not np.array_equal(got[p], ref):
                ys, xs = np.nonzero(got[p] != ref)
                bs, pad = (8, 16) if p else (16, 32)
                x, y = int(xs[0]) - pad, int(ys[0]) - pad
                raise AssertionError("%s: chain %d picture %d plane %d: %d samples differ, first at (%d,%d) (macroblock %d,%d) got %d want %d"
                                     % (label, chain, i, p, len(ys), x, y, x // bs, y // bs, got[p][ys[0], xs[0]], ref[ys[0], xs[0]]))


def _run(named, flags=0, replicate=2):
    """named: [(label, frames)] -> one session, one chain each (x replicate, so that the chain base is not 0), all compared"""
    import losslessh264_amd as lh
    for _, frames in named:
        D.check_refs_defined(frames)
    sess = lh.ReconSession([fr for _, fr in named], flags=flags, replicate=replicate)
    sess.run(); sess.synchronize()
    for c in range(sess.n_chains):
        label, frames = named[c % len(named)]
        _check(sess, c, frames, _oracle((label, flags), frames, flags), label)


@pytest.fixture(autouse=True)
def _no_wave_override(monkeypatch):
    monkeypatch.delenv("LH264_WAVES", raising=False)


@pytest.mark.parametrize("mb_w,mb_h", G.SHAPES)
def test_picture_shapes(mb_w, mb_h):
    """one macroblock sees every combination of a left neighbour, a row above, the last column and the last row"""
    _run([("shape %dx%d" % (mb_w, mb_h), G.chain(mb_w, mb_h))])


@pytest.mark.parametrize("mb_w,mb_h", G.SLICED)
@pytest.mark.parametrize("idc", [2, 1])
def test_slices_and_filter_modes(mb_w, mb_h, idc):
    """idc 2: neighbours across the slice edge take no part in the filter; idc 1: no filter at all"""
    _run([("sliced %dx%d idc %d" % (mb_w, mb_h, idc), G.chain(mb_w, mb_h, n_slices=2, idc=idc))])


@pytest.mark.parametrize("flags", [O.NO_EXPAND, O.NO_DEBLOCK, O.NO_EXPAND | O.NO_DEBLOCK])
def test_job_flags(flags):
    """without the padding only intra pictures are defined (a vector may reach into it)"""
    frames = G.intra_chain(3, 3) if flags & O.NO_EXPAND else G.chain(3, 3)
    _run([("flags %d" % flags, frames)], flags=flags)


@pytest.mark.parametrize("place", list(G.uncovered_places()))
def test_uncovered_macroblock(place):
    """the pass-through loads of a macroblock no slice covers, and its neighbours' filters across it"""
    _run([("uncovered " + place, G.uncovered(G.uncovered_places()[place]))])


@pytest.mark.parametrize("name", G.QP_PATTERNS)
def test_qp_patterns(name):
    """one threshold lookup where the three QPs of every line agree, three where any differs; the Cb / Cr quirk of an intra macroblock"""
    _run([("qp " + name, G.qp_pattern(name))])
