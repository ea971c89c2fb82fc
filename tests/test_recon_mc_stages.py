"""The inputs of tests/recon_stages.py:mc_stage_cases reach what they claim: shown with the oracle alone (CPU).  The device runs of the
same inputs are in tests/test_recon_mc_stages_gpu.py."""
import itertools

import numpy as np
import pytest

import oracle_lib as O
import recon_directed as D
import recon_stages as S


@pytest.fixture(scope="module")
def cases():
    return S.mc_stage_cases()


def _oracle(frames):
    pics, out = {}, []
    for f in frames:
        dst = O.HostPic(f.mb_w, f.mb_h)
        O.recon_frame(f.mbs, f.coeffs, f.slices, dst, [pics[r] for r in f.ref_ids], 0)
        pics[f.id] = dst
        out.append(dst)
    return out


def _cls(frac):
    return [n for n, fr in S.CLASSES if frac in fr][0]


def test_every_input_is_defined_and_unclamped(cases):
    assert len({c.name for c in cases}) == len(cases)
    lo, hx, hy = D.clamp_bounds(1, 1)
    for c in cases:
        D.check_refs_defined(c.frames)
        ref, f = c.frames
        assert (f.mb_w, f.mb_h) == (1, 1) and (ref.mbs["mb_type"] == S.IPCM).all() and f.slices["deblock_idc"][0] == 1
        for (ox, oy, w, h, mvx, mvy) in c.parts:
            assert lo < 4 * ox + mvx < hx and lo < 4 * oy + mvy < hy
            for by, bx in itertools.product(range(oy >> 2, (oy + h) >> 2), range(ox >> 2, (ox + w) >> 2)):
                assert tuple(f.mbs[0]["mv"][by * 4 + bx]) == (mvx, mvy)


def test_a_and_d_hold_every_assignment_of_the_classes(cases):
    """256 assignments of (full-pel, fy == 0, fx == 0, both) to the four 8x8 partitions on each content, plain (a) and weighted (d);
    over the cases each class meets all of its fractions in each quadrant position it can take"""
    for kind in "ad":
        for content in S.MC_CONTENTS:
            sel = [c for c in cases if c.kind == kind and c.name.endswith(content)]
            assert len(sel) == 256
            assert {tuple(_cls(fr) for fr in c.fractions()) for c in sel} == set(itertools.product([n for n, _ in S.CLASSES], repeat=4))
            assert {fr for c in sel for fr in c.fractions()} == set(S.POSITIONS)
            for c in sel:
                assert int(c.frames[1].mbs[0]["mb_type"]) == S.P8x8 and len(c.parts) == 4
                assert bool(c.frames[1].slices[0]["weighted_pred"]) == (kind == "d")
            assert sum(int(c.frames[1].mbs[0]["cbp"]) != 0 for c in sel) >= 32      # some with a residual (the unpacked path)
    wp = [c.frames[1].slices[0] for c in cases if c.kind == "d"]
    assert {(int(s["luma_log2_denom"]), int(s["chroma_log2_denom"])) for s in wp} == set(D.WP_DENOMS)
    assert {int(s["luma_weight"][0]) for s in wp} >= set(D.WP_EXTREMES) and {int(s["luma_offset"][0]) for s in wp} >= set(D.WP_EXTREMES)


def test_b_holds_every_ordered_pair_of_positions(cases):
    for content in S.MC_CONTENTS:
        sel = [c for c in cases if c.kind == "b" and c.name.endswith(content)]
        assert {tuple(c.fractions()) for c in sel} == set(itertools.product(S.POSITIONS, repeat=2)) and len(sel) == 256
        pairs = {tuple(c.fractions()) for c in sel}
        assert ((1, 3), (1, 0)) in pairs and ((2, 0), (3, 3)) in pairs          # stage H on row 3 beside row 2
        assert ((1, 1), (2, 2)) in pairs and ((3, 3), (1, 2)) in pairs          # e / r beside j / i
        assert ((0, 0), (2, 2)) in pairs and ((3, 1), (0, 0)) in pairs          # full-pel beside both fractions


def test_c_and_e(cases):
    for content in S.MC_CONTENTS:
        sel = [c for c in cases if c.kind == "c" and c.name.endswith(content)]
        assert len(sel) == 4 and all(sorted(c.fractions()) == sorted(S.POSITIONS) for c in sel)
        assert len({tuple(c.fractions()) for c in sel}) == 4
        sel = [c for c in cases if c.kind == "e" and c.name.endswith(content)]
        assert len(sel) == 24
        for c in sel:
            assert all(fy == 0 for _, fy in c.fractions()) and len({fx for fx, _ in c.fractions()}) >= 2       # one row fetched, mixed fx
        assert any({fx for fx, _ in c.fractions()} == {0, 1, 2, 3} for c in sel)


def test_contents_reach_both_clips_of_the_centre_position(cases):
    """from the oracle's reference picture: over the partitions at (2, 2), (j + 512) >> 10 goes above 255 and below 0 on each content,
    and the vertical sums reach the ends of int16's use (+10,710 / -2,550) on the tap-extreme content"""
    for content in S.MC_CONTENTS:
        hi, lo, n = -1 << 30, 1 << 30, 0
        for c in cases:
            if not c.name.endswith(content) or (2, 2) not in c.fractions():
                continue
            for j in S.centre_sums(_oracle(c.frames[:1])[0].padded_plane(0), c):
                hi, lo, n = max(hi, (int(j.max()) + 512) >> 10), min(lo, (int(j.min()) + 512) >> 10), n + 1
        assert n >= 50 and hi > 255 and lo < 0, (content, n, hi, lo)
    c = [c for c in cases if c.name.endswith("tap_extreme")][0]
    pic = _oracle(c.frames[:1])[0].padded_plane(0).astype(np.int64)
    vs = sum(S.TAPS[i] * pic[i:i + pic.shape[0] - 5, :] for i in range(6))
    assert vs.max() == 10710 and vs.min() == -2550


def test_the_oracle_runs_every_case(cases):
    for c in cases:
        _oracle(c.frames)
