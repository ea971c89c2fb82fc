"""Directed inputs for the two places where the reconstruct kernel works by lanes that differ inside one macroblock (no GPU here):
the luma motion compensation, which runs by stages (H, V, X, J of mc_luma_rows) that every lane needing them shares, and the boundary
strengths, which lanes compute from 4x4 blocks and their left / upper block.  The helpers are those of tests/recon_directed.py.
tests/test_recon_mc_stages.py and tests/test_recon_bs_lanes.py prove with the oracle alone that every input reaches what it claims;
tests/test_recon_mc_stages_gpu.py and tests/test_recon_bs_lanes_gpu.py run them through the kernel."""
import copy
import itertools

import numpy as np

import recon_directed as D
from synth import I16, IPCM, P16, P8x8, P8x8R0, SKIP    # noqa: F401 (the tests read them from here)

CONCEAL = 0x400            # LH264_MB_CONCEAL
TAPS = np.array([1, -5, 20, 20, -5, 1])

# ---- motion compensation by stages -----------------------------------------------------------------------------------------------------
# the four classes of a quarter-sample position (fx, fy): which stages a strip of that position needs
CLASSES = (("full", [(0, 0)]),
           ("h", [(1, 0), (2, 0), (3, 0)]),                                        # stage H alone
           ("v", [(0, 1), (0, 2), (0, 3)]),                                        # stage V alone
           ("hv", [(fx, fy) for fy in (1, 2, 3) for fx in (1, 2, 3)]))             # H + V + X, and J where fx == 2 or fy == 2
POSITIONS = [(fx, fy) for fy in range(4) for fx in range(4)]
MC_CONTENTS = ("tap_extreme", "binary")


class McCase:
    """frames: [PCM reference, P picture of one macroblock]; parts: (ox, oy, w, h, mvx, mvy) of its partitions; kind: 'a'..'e'"""

    def __init__(self, name, kind, frames, parts):
        self.name, self.kind, self.frames, self.parts = name, kind, frames, parts

    def fractions(self):
        return [(p[4] & 3, p[5] & 3) for p in self.parts]


def _weights(f, rng, k):
    sl = f.slices[0]
    sl["weighted_pred"] = 1
    sl["luma_log2_denom"], sl["chroma_log2_denom"] = D.WP_DENOMS[k % 9]
    sl["luma_weight"], sl["luma_offset"] = D._wp_values(rng), D._wp_values(rng)
    sl["chroma_weight"] = np.stack([D._wp_values(rng), D._wp_values(rng)], axis=1)
    sl["chroma_offset"] = np.stack([D._wp_values(rng), D._wp_values(rng)], axis=1)


def _mc_case(rng, name, kind, content, shape, fracs, weighted=None, residual=False):
    """one macroblock of `shape` whose partition i lies at the fraction fracs[i], with a random integer displacement of up to 10
    samples (inside the 32 samples of padding: nothing is clamped)"""
    parts = []
    for (ox, oy, w, h), (fx, fy) in zip(D.SHAPES[shape][2], fracs):
        ix, iy = (int(v) for v in rng.integers(-10, 11, 2))
        parts.append((ox, oy, w, h, 4 * ix + fx, 4 * iy + fy))
    ref = D.pcm_content(rng, 1, 1, content)
    f = D.new_frame(1, 1, 1, [0], idc=1)
    D.set_inter(f.mbs[0], shape, [(p[4], p[5]) for p in parts])
    if residual:
        D.set_residual(f.mbs[0], f.coeffs[0], rng)
    if weighted is not None:
        _weights(f, rng, weighted)
    return McCase("%s %s %s" % (kind, name, content), kind, [ref, f], parts)


def mc_stage_cases(seed=11):
    """-> list of McCase.
    a: P8x8 of four 8x8 partitions, every assignment of the four classes to the four quadrants (256), each class walking through
       its fractions from case to case; every fourth case carries a residual
    b: P16x8 with every ordered pair of the 16 positions (256): fy == 3 (stage H on row 3) beside fy == 0 (row 2), e g p r beside
       the positions that need j, full-pel beside both fractions
    c: sixteen 4x4 partitions with all 16 positions at once (the identity and three permutations)
    d: a again under explicit weighted prediction
    e: every partition fy == 0 with all four fx in one macroblock: the one-row fetch
    each on both contents."""
    rng = np.random.default_rng(seed)
    out = []
    for content in MC_CONTENTS:
        for kind in ("a", "d"):
            used = [0, 0, 0, 0]
            for i, assign in enumerate(itertools.product(range(4), repeat=4)):
                fracs = []
                for c in assign:
                    fracs.append(CLASSES[c][1][used[c] % len(CLASSES[c][1])])
                    used[c] += 1
                name = "8x8 " + "/".join(CLASSES[c][0] for c in assign)
                out.append(_mc_case(rng, name, kind, content, "8x8", fracs, weighted=i if kind == "d" else None, residual=i % 4 == 3))
        for p0, p1 in itertools.product(POSITIONS, repeat=2):
            out.append(_mc_case(rng, "16x8 %d%d+%d%d" % (p0 + p1), "b", content, "16x8", [p0, p1]))
        for k in range(4):
            perm = list(range(16)) if k == 0 else list(rng.permutation(16))
            out.append(_mc_case(rng, "4x4 all16 perm%d" % k, "c", content, "4x4", [POSITIONS[j] for j in perm], residual=k == 3))
        for shape in ("16x8", "8x16", "8x8", "8x4", "4x8", "4x4"):
            n = len(D.SHAPES[shape][2])
            for rot in range(4):
                fracs = [((j + rot) % 4 if n >= 4 else (2 * j + rot) % 4, 0) for j in range(n)]
                out.append(_mc_case(rng, "%s fy0 rot%d" % (shape, rot), "e", content, shape, fracs))
    return out


def centre_sums(ref_plane, case):
    """the unshifted centre values j (tap over the vertical sums) of every sample of the case's partitions at position (2, 2), from
    the padded luma plane of its reference"""
    pic = ref_plane.astype(np.int64)
    out = []
    for (ox, oy, w, h, mvx, mvy) in case.parts:
        if (mvx & 3, mvy & 3) != (2, 2):
            continue
        x0, y0 = ox + (mvx >> 2) + D.PAD, oy + (mvy >> 2) + D.PAD
        win = pic[y0 - 2:y0 + h + 3, x0 - 2:x0 + w + 3]
        vs = sum(TAPS[i] * win[i:i + h, :] for i in range(6))
        out.append(sum(TAPS[i] * vs[:, i:i + w] for i in range(6)))
    return out


# ---- boundary strengths on block lanes -------------------------------------------------------------------------------------------------
C = 4                      # macroblock (1, 1) of 3x3
INNER_LINES = (2, 3, 4, 5, 10, 11, 12, 13)      # lines of an edge that no crossing edge's bS < 4 filter reaches (it changes 2 samples a side)


class BsLaneCase:
    """frames: what the kernel gets; oracle_frames: an input the oracle reconstructs to the same pictures (the oracle does not know
    LH264_MB_CONCEAL) - the same list otherwise; claims: [((mb x, mb y, dir, edge, lines 0..15), filtered)]"""

    def __init__(self, name, frames, claims, oracle_frames=None):
        self.name, self.frames, self.claims = name, frames, claims
        self.oracle_frames = frames if oracle_frames is None else oracle_frames


def edge_lines(plane, edge):
    """the luma samples p0 | q0 on both sides of an edge, on the given lines (rows of a vertical edge, columns of a horizontal one)"""
    x, y, d, e, lines = edge
    if d == 0:
        return np.stack([plane[16 * y + i, 16 * x + 4 * e - 1:16 * x + 4 * e + 1] for i in lines])
    return np.stack([plane[16 * y + 4 * e - 1:16 * y + 4 * e + 1, 16 * x + i] for i in lines])


def seg_lines(*segs):
    return tuple(4 * s + i for s in segs for i in range(4))


ALL_LINES = seg_lines(0, 1, 2, 3)


def _base(rng, idc=0, bounds=None):
    """[PCM of smooth content, P picture of 3x3 P16x16 macroblocks with zero vectors and no residual] -> frames, P picture.
    bounds: first macroblocks of the slices"""
    frames = [D.pcm_content(rng, 3, 3, "smooth", 0)]
    f = D.new_frame(1, 3, 3, [0], idc=idc, n_slices=1 if bounds is None else len(bounds), qp=D.BS_QP)
    if bounds is not None:
        ends = list(bounds[1:]) + [9]
        for s, (a, b) in enumerate(zip(bounds, ends)):
            f.slices[s]["first_mb"], f.slices[s]["n_mbs"] = a, b - a
            f.mbs["slice_id"][a:b] = s
    for k in range(9):
        D.set_inter(f.mbs[k], "16x16", [(0, 0)])
    frames.append(f)
    return frames, f


def _count(f, k, bx, by):
    """one coefficient in the 4x4 block (bx, by) of macroblock k, with the cbp bit and the nonzero count that go with it"""
    t8 = int(f.mbs[k]["flags"]) & 1
    zb = (bx & 1) | (by & 1) << 1 | (bx >> 1) << 2 | (by >> 1) << 3
    f.coeffs[k][(zb >> 2) * 64 if t8 else zb * 16] = 1         # a DC: an offset on the block, the filters' conditions keep holding
    f.mbs[k]["cbp"] |= 1 << (zb >> 2)
    f.mbs[k]["nzc"][by * 4 + bx] = 1


def _pcm(frames, k):
    """macroblock k of the P picture becomes I_PCM with the samples the reference picture has there: smooth, with steps at the block
    boundaries (its record keeps the picture's QP, so its edges are filtered)"""
    f = frames[-1]
    m = f.mbs[k]
    m["mb_type"], m["flags"], m["nzc"], m["chroma_mode"], m["cbp"], m["sub_type"], m["ref_idx"], m["mv"] = IPCM, 2, 16, 6, 0, 0, 0, 0
    f.coeffs[k] = frames[0].coeffs[k]


def _nb(d):
    return C - 1 if d == 0 else C - 3


def bs_lane_cases(seed=12):
    """-> list of BsLaneCase, the case macroblock at (1, 1) of 3x3 unless the name says otherwise"""
    rng = np.random.default_rng(seed)
    out = []
    diffs = [((3, 0), False), ((4, 0), True), ((0, -3), False), ((0, -4), True)]
    # inner edge 2 under the 8x8 transform: vectors 3 / 4 apart, and a count in only one of the two 8x8 blocks
    for d in (0, 1):
        for v, filt in diffs:
            frames, f = _base(rng)
            D.set_inter(f.mbs[C], "8x8", D._split("8x8", d, 2, (0, 0), v))
            f.mbs[C]["flags"] = 1
            out.append(BsLaneCase("t8 edge2 dir%d vectors %d,%d" % (d, v[0], v[1]), frames, [((1, 1, d, 2, ALL_LINES), filt)]))
        for side in (0, 1):                                    # the 8x8 block before / behind the edge, first half of the edge; its
            frames, f = _base(rng)                             # count sits in the 4x4 block that does not touch the edge
            f.mbs[C]["mb_type"], f.mbs[C]["sub_type"], f.mbs[C]["flags"] = P8x8, D.SUB_8x8, 1
            b = 3 * side
            _count(f, C, b if d == 0 else 0, 0 if d == 0 else b)
            out.append(BsLaneCase("t8 edge2 dir%d count %s" % (d, "behind" if side else "before"), frames,
                                  [((1, 1, d, 2, (2, 3, 4, 5)), True), ((1, 1, d, 2, (10, 11, 12, 13)), False)]))
    # edges 1 and 3 under the 8x8 transform: vectors and counts that filter them without the flag, and must not with it
    for d in (0, 1):
        for what in ("vectors", "counts"):
            for t8 in (1, 0):
                frames, f = _base(rng)
                m = f.mbs[C]
                if what == "vectors":                          # each column (dir 0) / row (dir 1) of blocks 4 further
                    D.set_inter(m, "4x4", [((ox if d == 0 else oy), 0) for (ox, oy, _, _) in D.SHAPES["4x4"][2]])
                else:
                    m["mb_type"], m["sub_type"] = P8x8, D.SUB_8x8
                m["flags"] = t8
                if what == "counts":                           # blocks (0, 1) and (2, 1) [dir 0]: edges 1 and 3, lines 4..7
                    for b in (0, 2):
                        _count(f, C, b if d == 0 else 1, 1 if d == 0 else b)
                lines = INNER_LINES if what == "vectors" else (4, 5)
                out.append(BsLaneCase("%s edges 1 3 dir%d %s" % ("t8" if t8 else "no t8", d, what), frames,
                                      [((1, 1, d, 1, lines), not t8), ((1, 1, d, 3, lines), not t8)]))
    # intra at (1, 1): 3 inside, 4 at its edges
    frames, f = _base(rng)
    _pcm(frames, C)
    out.append(BsLaneCase("intra pcm", frames, [((1, 1, d, e, INNER_LINES), True) for d in (0, 1) for e in (0, 1, 2, 3)]))
    frames, f = _base(rng)
    f.mbs[C]["mv"], f.mbs[C]["sub_type"] = 0, 0
    D.directed_intra(f.mbs[C], 2, 1, 3)
    f.coeffs[C][:256] = np.where(np.arange(256) % 16 == 0, rng.integers(-2, 3, 256), 0)           # a DC for every block: steps
    f.mbs[C]["cbp"] = 0
    D.set_nzc(f.mbs[C], f.coeffs[C])
    out.append(BsLaneCase("intra 16x16", frames, [((1, 1, d, e, INNER_LINES), True) for d in (0, 1) for e in (0, 1, 2, 3)]))
    # inter at (1, 1) beside an intra neighbour: 4 (every vector is zero: without the neighbour nothing is filtered)
    for d in (0, 1):
        for intra in (True, False):
            frames, f = _base(rng)
            if intra:
                _pcm(frames, _nb(d))
            out.append(BsLaneCase("intra neighbour dir%d %s" % (d, "pcm" if intra else "control"), frames, [((1, 1, d, 0, INNER_LINES), intra)]))
    # the case macroblock at (0, 0): no neighbours; its inner edges as everywhere
    for d in (0, 1):
        for v, filt in diffs[:2]:
            frames, f = _base(rng)
            D.set_inter(f.mbs[0], "4x4", D._split("4x4", d, 2, (0, 0), v))
            for s in range(4):                                 # counts along its left and top edge: strengths only beside a neighbour
                _count(f, 0, 0, s)
                _count(f, 0, s, 0)
            out.append(BsLaneCase("corner dir%d %d" % (d, v[0]), frames, [((0, 0, d, 2, (6, 7, 8, 9, 10, 11)), filt)]))
    # deblock_idc 2: no filter across a slice border.  Slices are runs in raster order: a border above (1, 1) alone, or left and above
    for name, bounds, left, top in (("top border", [0, 3], True, False), ("left and top border", [0, 4], False, False), ("no border", None, True, True)):
        frames, f = _base(rng, idc=2, bounds=bounds)
        D.set_inter(f.mbs[C], "16x16", [(4, 0)])
        out.append(BsLaneCase("idc2 " + name, frames, [((1, 1, 0, 0, INNER_LINES), left), ((1, 1, 1, 0, INNER_LINES), top)]))
    # a concealed neighbour (a slice of its own that is not filtered, as the front end emits it): the edge towards it is not filtered.
    # The oracle, which does not know the flag, gets the plain type and deblock_idc 2 in the other slices: the same pictures, because
    # nothing but the concealed macroblock's vector differs from its surroundings.
    for d in (0, 1):
        k = _nb(d)
        frames, f = _base(rng, bounds=[0, k, k + 1])
        D.set_inter(f.mbs[k], "16x16", [(4, 0)])
        f.slices[1]["deblock_idc"] = 1
        g = copy.deepcopy(f)
        f.mbs[k]["mb_type"] = P16 | CONCEAL
        g.slices["deblock_idc"] = (2, 1, 2)
        out.append(BsLaneCase("concealed neighbour dir%d" % d, frames, [((1, 1, d, 0, INNER_LINES), False)], oracle_frames=[frames[0], g]))
        frames, f = _base(rng)
        D.set_inter(f.mbs[k], "16x16", [(4, 0)])
        out.append(BsLaneCase("concealed neighbour dir%d control" % d, frames, [((1, 1, d, 0, INNER_LINES), True)]))
    # a nonzero count on one side of the macroblock edge only, one segment at a time
    for d in (0, 1):
        for side in ("current", "neighbour"):
            for s in range(4):
                frames, f = _base(rng)
                if side == "current":
                    _count(f, C, 0 if d == 0 else s, s if d == 0 else 0)
                else:
                    _count(f, _nb(d), 3 if d == 0 else s, s if d == 0 else 3)
                far = [t for t in range(4) if abs(t - s) >= 2]
                out.append(BsLaneCase("count %s dir%d segment %d" % (side, d, s), frames,
                                      [((1, 1, d, 0, seg_lines(s)), True), ((1, 1, d, 0, seg_lines(*far)), False)]))
    # P8x8REF0
    for d in (0, 1):
        for v, filt in diffs:
            frames, f = _base(rng)
            D.set_inter(f.mbs[C], "8x8", D._split("8x8", d, 2, (0, 0), v))
            f.mbs[C]["mb_type"] = P8x8R0
            out.append(BsLaneCase("P8x8REF0 dir%d vectors %d,%d" % (d, v[0], v[1]), frames, [((1, 1, d, 2, ALL_LINES), filt)]))
    # SKIP beside P16x16 at the macroblock edge, either way round
    for d in (0, 1):
        for v, filt in diffs:
            for skip_is in ("current", "neighbour"):
                frames, f = _base(rng)
                D.set_inter(f.mbs[C], "16x16", [v])
                f.mbs[C if skip_is == "current" else _nb(d)]["mb_type"] = SKIP
                out.append(BsLaneCase("SKIP %s dir%d vectors %d,%d" % (skip_is, d, v[0], v[1]), frames, [((1, 1, d, 0, INNER_LINES), filt)]))
    return out
