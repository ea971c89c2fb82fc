"""Directed inputs of the reconstruct kernel's intra prediction (no GPU here): small pictures of I_PCM macroblocks under deblock_idc 1,
whose samples are therefore given exactly, with intra macroblocks under test at places where all their neighbours are I_PCM.  The
families: every I4x4 (mode, block), the *_TOP modes where real top-right samples exist, every I8x8 (mode, block, top-left, top-right),
I16x16 and chroma with plane predictors at the ends of their arithmetic and chroma DC sums that all differ, macroblocks at the
picture's and the slices' edges, coded residual that drives prediction + residual beyond both ends of 8 bits, and everything without
residual once more under a strong in-loop filter.  cells() says which coverage cells a case reaches, all_cell_names() which are
demanded; tests/test_intra_directed.py holds the cases against tests/intra_model.py and the oracle (CPU),
tests/test_intra_directed_gpu.py runs them through the kernel."""
import copy

import numpy as np

import intra_model as M
import recon_directed as D
from intra_model import AVAIL_L, AVAIL_T, AVAIL_TL, AVAIL_TR
from synth import I4, I8, I16, IPCM

MB_W, MB_H = 7, 6
SITES = [(x, y) for y in (1, 3, 5) for x in (1, 3, 5)]         # odd (x, y), a right-hand neighbour included: all eight neighbours I_PCM
TYPE_NAME = {I4: "i4", I8: "i8", I16: "i16"}
TOP_MODES = (M.DDL_TOP, M.VL_TOP)


# ---- which modes respect availability ---------------------------------------------------------------------------------------------------
def z_of(bx, by):
    return (bx & 1) | ((by & 1) << 1) | ((bx >> 1) << 2) | ((by >> 1) << 3)


def _bits(avail):
    return tuple(bool(avail & b) for b in (AVAIL_T, AVAIL_TL, AVAIL_L, AVAIL_TR))


def i4_block_avail(avail, bx, by):
    """(top, left, top-left, top-right) of 4x4 block (bx, by); inside the macroblock the top-right block is available where it
    precedes the block in z-order (6.4.11.4)"""
    t, tl, l, tr = _bits(avail)
    a_tr = (t if bx < 3 else tr) if by == 0 else (bx < 3 and z_of(bx + 1, by - 1) < z_of(bx, by))
    return t if by == 0 else True, l if bx == 0 else True, tl if (bx == 0 and by == 0) else t if by == 0 else l if bx == 0 else True, a_tr


def i8_block_avail(avail, i8):
    t, tl, l, tr = _bits(avail)
    ftl, ftr = M.i8_flags(avail)
    return t if i8 < 2 else True, l if (i8 & 1) == 0 else True, ftl[i8], ftr[i8]


def nxn_valid(mode, a_t, a_l, a_tl, a_tr, strict_top):
    """a mode is valid where it reads available samples only.  strict_top (I8x8, whose records carry the flag): a *_TOP mode goes
    with an unavailable top-right block, as the parser pairs them"""
    if mode == M.DC_128:
        return True
    if mode in (M.V, M.DC_T):
        return a_t
    if mode in (M.H, M.HU, M.DC_L):
        return a_l
    if mode == M.DC:
        return a_t and a_l
    if mode in (M.DDR, M.VR, M.HD):
        return a_t and a_l and a_tl
    if mode in (M.DDL, M.VL):
        return a_t and a_tr
    return a_t and not (strict_top and a_tr)


def i4_valid(avail):
    """raster block -> its valid modes"""
    return [[m for m in range(14) if nxn_valid(m, *i4_block_avail(avail, b & 3, b >> 2), False)] for b in range(16)]


def i8_valid(avail):
    return [[m for m in range(14) if nxn_valid(m, *i8_block_avail(avail, i8), True)] for i8 in range(4)]


def i16_valid(avail):
    t, tl, l, _ = _bits(avail)
    return [m for m, ok in ((M.I16_V, t), (M.I16_H, l), (M.I16_DC, t and l), (M.I16_P, t and l and tl), (M.I16_DC_L, l), (M.I16_DC_T, t), (M.I16_DC_128, True)) if ok]


def chroma_valid(avail):
    t, tl, l, _ = _bits(avail)
    return [m for m, ok in ((M.C_DC, t and l), (M.C_H, l), (M.C_V, t), (M.C_P, t and l and tl), (M.C_DC_L, l), (M.C_DC_T, t), (M.C_DC_128, True)) if ok]


def physical_avail(f, k):
    """what 6.4.9 gives in a picture of raster slices: a neighbour is available where it exists and lies in the same slice"""
    x, y, sid = k % f.mb_w, k // f.mb_w, f.mbs["slice_id"]
    a = 0
    if y > 0 and sid[k - f.mb_w] == sid[k]:
        a |= AVAIL_T
    if x > 0 and y > 0 and sid[k - f.mb_w - 1] == sid[k]:
        a |= AVAIL_TL
    if x > 0 and sid[k - 1] == sid[k]:
        a |= AVAIL_L
    if y > 0 and x + 1 < f.mb_w and sid[k - f.mb_w + 1] == sid[k]:
        a |= AVAIL_TR
    return a


# ---- content classes: (rng, height, width, unit) -> plane; unit: the macroblock's size in the plane (16 luma, 8 chroma) ----------------
def content_uniform(rng, h, w, unit):
    return rng.integers(0, 256, (h, w)).astype(np.uint8)


def content_binary(rng, h, w, unit):
    return rng.choice(np.array([0, 255], dtype=np.uint8), (h, w))


def content_steep(sx, sy):
    """the steepest ramp a plane predictor can see: the row above a macroblock at odd (x, y) is 0 left of its middle and 255 right of
    it (sx > 0; the reverse for sx < 0), the column left of it likewise in y: |H| = |V| = 9180 in luma where the signs agree (the
    corner sample belongs to both)"""
    def fn(rng, h, w, unit):
        y, x = np.mgrid[0:h, 0:w]
        per = 2 * unit
        gx = np.where((x % per) >= 3 * unit // 2, 255, 0)
        gy = np.where((y % per) >= 3 * unit // 2, 255, 0)
        a = rng.integers(0, 256, (h, w))
        a = np.where((x % per) == unit - 1, gy if sy > 0 else 255 - gy, a)
        a = np.where((y % per) == unit - 1, gx if sx > 0 else 255 - gx, a)
        return a.astype(np.uint8)
    return fn


def content_gentle(rng, h, w, unit):
    """slopes of +-1/4 .. 2 a sample, a pair a tile of two macroblocks, with a little noise: small H and V of both signs, no clip"""
    y, x = np.mgrid[0:h, 0:w]
    per = 2 * unit
    ty, tx = y // per, x // per
    shape = (h // per + 1, w // per + 1)
    sx = (rng.choice([-1, 1], shape) * rng.integers(1, 9, shape) / (4.0 * unit / 8))[ty, tx]
    sy = (rng.choice([-1, 1], shape) * rng.integers(1, 9, shape) / (4.0 * unit / 8))[ty, tx]
    base = rng.integers(80, 176, shape)[ty, tx]
    return np.clip(np.rint(base + sx * ((x % per) - unit) + sy * ((y % per) - unit)) + rng.integers(-2, 3, (h, w)), 0, 255).astype(np.uint8)


def content_distinct(rng, h, w, unit):
    """a level per 4x4 block, 16 different ones in a pattern of period 16, and noise below their distance: the four sums of chroma DC
    differ from each other, and (other levels a plane) Cb's from Cr's"""
    y, x = np.mgrid[0:h, 0:w]
    lv = rng.permutation(np.arange(6, 246, 12))[:16]
    return (lv[((x // 4) % 4) + 4 * ((y // 4) % 4)] + rng.integers(0, 6, (h, w))).astype(np.uint8)


def content_ties(rng, h, w, unit):
    """two neighbouring values: sums on every residue of the roundings"""
    y, x = np.mgrid[0:h, 0:w]
    base = rng.integers(0, 255, (h // 8 + 1, w // 8 + 1))[y // 8, x // 8]
    return (base + rng.integers(0, 2, (h, w))).astype(np.uint8)


CLASSES = {"uniform": content_uniform, "binary": content_binary, "steep++": content_steep(1, 1), "steep+-": content_steep(1, -1),
           "steep-+": content_steep(-1, 1), "steep--": content_steep(-1, -1), "gentle": content_gentle, "distinct": content_distinct}
RAMPS = ("steep++", "steep+-", "steep-+", "steep--", "gentle")


def make_planes(rng, content, mb_w, mb_h, avoid128=False):
    fn = CLASSES[content] if isinstance(content, str) else content
    planes = [fn(rng, mb_h * 16, mb_w * 16, 16), fn(rng, mb_h * 8, mb_w * 8, 8), fn(rng, mb_h * 8, mb_w * 8, 8)]
    if avoid128:
        planes = [np.where(p == 128, 127, p).astype(np.uint8) for p in planes]
    return planes


def edge_vectors(rng, cls, n):
    """the neighbours of one n x n block in content class cls -> (p[-1..2n-1, -1], p[-1, 0..n-1]); for the oracle's pin against the
    reference's kernels (tests/test_oracle_vs_ref.py)"""
    if cls == "ties":
        plane = content_ties(rng, 4 * n, 4 * n, n)
    else:
        plane = CLASSES[cls](rng, 4 * n, 4 * n, n)
    return plane[n - 1, n - 1:3 * n].copy(), plane[n:2 * n, n - 1].copy()


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """one picture: I_PCM macroblocks carrying `planes`, with the macroblocks under test (sites: (x, y, avail, place)) put over them"""

    def __init__(self, name, family, planes, mb_w=MB_W, mb_h=MB_H, starts=(0,)):
        self.name, self.family, self.planes, self.mb_w, self.mb_h = name, family, planes, mb_w, mb_h
        self.f = D.pcm_picture(mb_w, mb_h, *planes)
        n = mb_w * mb_h
        bounds = list(starts) + [n]
        sl = np.zeros(len(starts), dtype=self.f.slices.dtype)
        sl[:] = self.f.slices[0]
        for s in range(len(starts)):
            sl[s]["first_mb"], sl[s]["n_mbs"] = bounds[s], bounds[s + 1] - bounds[s]
            self.f.mbs["slice_id"][bounds[s]:bounds[s + 1]] = s
        self.f.slices = sl
        self.sites = []
        self.residual = False
        self.zero_residual_unfiltered = True
        self._cache = {}

    def frames(self):
        return [self.f]

    def put(self, x, y, typ, modes, chroma, avail, place=""):
        """modes: 16 (I4x4, raster blocks), 4 (I8x8, z-order) or 1 (I16x16)"""
        k = y * self.mb_w + x
        m = self.f.mbs[k]
        assert int(m["mb_type"]) == IPCM
        self.f.coeffs[k] = 0
        m["mb_type"], m["flags"], m["nzc"], m["cbp"], m["qp_y"], m["qp_c"] = typ, 1 if typ == I8 else 0, 0, 0, 26, 26
        mode = np.zeros(16, dtype=np.int8)
        if typ == I4:
            mode[:] = modes
        elif typ == I8:
            mode[[0, 2, 8, 10]] = modes
        else:
            mode[0] = modes[0]
        m["intra_mode"], m["chroma_mode"], m["intra_avail"] = mode, chroma, avail if typ == I8 else 0
        self.sites.append((x, y, avail, place))

    def record(self, x, y):
        return self.f.mbs[y * self.mb_w + x]

    # -- the oracle and the model on this case (kept: the pictures are compared, never written) --
    def oracle(self, flags=0):
        import oracle_lib as O
        if flags not in self._cache:
            dst = O.HostPic(self.mb_w, self.mb_h)
            O.recon_frame(self.f.mbs, self.f.coeffs, self.f.slices, dst, [], flags)
            self._cache[flags] = dst
        return self._cache[flags]

    def residual_of(self, x, y):
        """the residual of macroblock (x, y) as the oracle's transforms give it: the record alone in a picture, every mode DC_128 ->
        reconstruction - 128, exact where that stays inside 1..254 (asserted)"""
        import oracle_lib as O
        if ("res", x, y) in self._cache:
            return self._cache[("res", x, y)]
        k = y * self.mb_w + x
        f = D.new_frame(0, 1, 1, (), idc=1)
        f.mbs[0] = self.f.mbs[k]
        f.mbs[0]["slice_id"] = 0
        f.mbs[0]["intra_mode"] = M.I16_DC_128 if int(f.mbs[0]["mb_type"]) == I16 else M.DC_128
        f.mbs[0]["chroma_mode"] = M.C_DC_128
        f.coeffs[0] = self.f.coeffs[k]
        dst = O.HostPic(1, 1)
        O.recon_frame(f.mbs, f.coeffs, f.slices, dst, [], O.NO_EXPAND)
        out = [dst.plane(p).astype(np.int64) for p in range(3)]
        assert all(o.min() >= 1 and o.max() <= 254 for o in out), "%s (%d,%d): a residual beyond +-127 is not measured exactly" % (self.name, x, y)
        self._cache[("res", x, y)] = [o - 128 for o in out]
        return self._cache[("res", x, y)]

    def model(self, variant=None, preds=None):
        """the picture as the model predicts it: the given planes with every macroblock under test replaced.  preds: a dict that
        receives (x, y) -> the three prediction arrays"""
        if variant is None and preds is None and "model" in self._cache:
            return self._cache["model"]
        out = [p.copy() for p in self.planes]
        for (x, y, _, _) in self.sites:
            pr = None
            if preds is not None:
                pr = preds[(x, y)] = [np.zeros((16, 16), np.int64), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.int64)]
            got = M.predict_mb(self.planes, x, y, self.record(x, y), variant, self.residual_of(x, y) if self.residual else None, pr)
            for p, bs in enumerate((16, 8, 8)):
                out[p][bs * y:bs * y + bs, bs * x:bs * x + bs] = got[p]
        if variant is None and preds is None:
            self._cache["model"] = out
        return out


def _rot(lst, i):
    return lst[i % len(lst)]


def build_i4(seed=11):
    """every valid (mode, block) with all neighbours: macroblock j gives block b the ((j + 3 b) mod n)-th of its n valid modes, 18
    macroblocks a content class"""
    lists = i4_valid(15)
    cases = []
    for ci, cname in enumerate(CLASSES):
        rng = np.random.default_rng(seed * 1000 + ci)
        for pic in range(2):
            c = Case("i4 %s %d" % (cname, pic), "i4", make_planes(rng, cname, MB_W, MB_H))
            for si, (x, y) in enumerate(SITES):
                j = pic * len(SITES) + si
                c.put(x, y, I4, [_rot(lists[b], j + (3 + ci) * b) for b in range(16)], j % 7, 15)
            cases.append(c)
    return cases


def i8_plan():
    """[(avail, four modes)]: greedily, every valid (mode, block, top-left, top-right) over all 16 settings of intra_avail"""
    covered, plan = set(), []
    for avail in range(16):
        lists = i8_valid(avail)
        ftl, ftr = M.i8_flags(avail)
        while True:
            pick, new = [], False
            for i8 in range(4):
                todo = [m for m in lists[i8] if (m, i8, ftl[i8], ftr[i8]) not in covered]
                pick.append(todo[0] if todo else _rot(lists[i8], len(plan)))
                new = new or bool(todo)
            if not new:
                break
            covered |= {(pick[i8], i8, ftl[i8], ftr[i8]) for i8 in range(4)}
            plan.append((avail, pick))
    return plan


def build_i8(seed=12):
    plan = i8_plan()
    cases = []
    for ci, cname in enumerate(CLASSES):
        rng = np.random.default_rng(seed * 1000 + ci)
        for p0 in range(0, len(plan), len(SITES)):
            c = Case("i8 %s %d" % (cname, p0 // len(SITES)), "i8", make_planes(rng, cname, MB_W, MB_H))
            for si, (avail, pick) in enumerate(plan[p0:p0 + len(SITES)]):
                c.put(*SITES[si], I8, pick, _rot(chroma_valid(avail), p0 + si), avail)
            cases.append(c)
    return cases


def build_i16c(seed=13):
    """the seven I16x16 and the seven chroma modes; on the ramps every other macroblock predicts both by plane"""
    cases = []
    for ci, cname in enumerate(CLASSES):
        rng = np.random.default_rng(seed * 1000 + ci)
        for pic in range(2):
            c = Case("i16c %s %d" % (cname, pic), "i16c", make_planes(rng, cname, MB_W, MB_H))
            for si, (x, y) in enumerate(SITES):
                j = pic * len(SITES) + si
                plane = cname in RAMPS and j % 2 == 0
                c.put(x, y, I16, [M.I16_P if plane else j % 7], M.C_P if plane else (3 * j + 1) % 7, 15)
            cases.append(c)
    return cases


# the picture of the position family: 8 x 6, slices from (0,0), (3,2) and (0,4); site -> place
POS_W, POS_H = 8, 6
POS_STARTS = (0, 2 * POS_W + 3, 4 * POS_W)
POS_SITES = {(3, 0): "row0", (5, 0): "row0", (0, 1): "col0", (7, 1): "lastcol", (3, 2): "slice_first", (1, 3): "below_slice",
             (4, 4): "below_slice", (6, 4): "below_slice"}
PLACES = ("col0", "lastcol", "row0", "slice_first", "below_slice")
POS_ROT = 8


def build_pos(seed=14):
    """macroblocks in column 0, in the last column, in row 0, first of a slice that starts mid-row and directly below a slice
    boundary, each type at each site, the modes that stay valid there in turn.  No sample is 128: where a neighbour that exists is not
    available, nothing that could stand for it equals it by construction"""
    cases = []
    used = {}

    def fresh(key, lst, i):
        """the first mode of lst that this place and type have not had yet, else the i-th in turn"""
        todo = [m for m in lst if m not in used.setdefault(key, set())]
        m = todo[0] if todo else _rot(lst, i)
        used[key].add(m)
        return m
    for r in range(POS_ROT):
        for shift in range(3):
            cname = ("uniform", "distinct", "binary")[(r + shift) % 3]
            rng = np.random.default_rng(seed * 1000 + r * 3 + shift)
            c = Case("pos %d/%d %s" % (r, shift, cname), "pos", make_planes(rng, cname, POS_W, POS_H, avoid128=True), POS_W, POS_H, POS_STARTS)
            for s, ((x, y), place) in enumerate(POS_SITES.items()):
                avail = physical_avail(c.f, y * POS_W + x)
                typ = (I4, I8, I16)[(s + shift) % 3]
                if typ == I4:
                    lists = i4_valid(avail)
                    modes = [fresh((place, typ), lists[b], r + 3 * b) for b in range(16)]
                elif typ == I8:
                    lists = i8_valid(avail)
                    modes = [fresh((place, typ), lists[i8], r + 3 * i8) for i8 in range(4)]
                else:
                    modes = [fresh((place, typ), i16_valid(avail), r)]
                c.put(x, y, typ, modes, fresh((place, "c"), chroma_valid(avail), r + shift), avail, place)
            cases.append(c)
    return cases


def pos_avail():
    """place -> the availabilities its sites have"""
    c = Case("", "pos", make_planes(np.random.default_rng(0), "uniform", POS_W, POS_H), POS_W, POS_H, POS_STARTS)
    out = {}
    for (x, y), place in POS_SITES.items():
        out.setdefault(place, set()).add(physical_avail(c.f, y * POS_W + x))
    return out


def _ac_pair(rng, lo, hi):
    return int(rng.choice([-1, 1])) * int(rng.integers(lo, hi)), int(rng.choice([-1, 1])) * int(rng.integers(lo // 2, hi // 2))


def build_res(seed=15):
    """coded residual in every block of every plane (two AC coefficients a block, both signs, below +-127 a sample) over dark
    neighbours (0..24) and over bright ones (231..255): prediction + residual leaves 8 bits at both ends, in I4x4 and I8x8 also from
    samples that earlier blocks reconstructed"""
    lists4, lists8 = i4_valid(15), i8_valid(15)
    cases = []
    for name, lo in (("dark", 0), ("bright", 231)):
        rng = np.random.default_rng(seed * 1000 + lo)
        fn = lambda g, h, w, unit: g.integers(lo, lo + 25, (h, w)).astype(np.uint8)
        c = Case("res %s" % name, "res", make_planes(rng, fn, MB_W, MB_H))
        c.residual, c.zero_residual_unfiltered = True, False
        for si, (x, y) in enumerate(SITES):
            typ = (I4, I8, I16)[si % 3]
            j = si // 3
            if typ == I4:
                modes = [_rot(lists4[b], 5 * j + 3 * b + (lo > 0)) for b in range(16)]
                if j == 0:           # one macroblock whose blocks read left, top, top-left and top-right inside the macroblock
                    modes = [M.DC, M.H, M.HU, M.H, M.V, M.DDR, M.DDL, M.VR, M.VL, M.HD, M.DDL, M.DC, M.V, M.DDR, M.VL, M.HD]
            elif typ == I8:
                modes = [_rot(lists8[i8], 4 * j + 3 * i8 + (lo > 0)) for i8 in range(4)]
            else:
                modes = [(M.I16_DC, M.I16_P, M.I16_V)[j]]
            c.put(x, y, typ, modes, (M.C_DC, M.C_P, M.C_H)[j], 15)
            k = y * MB_W + x
            m, co = c.f.mbs[k], c.f.coeffs[k]
            if typ == I8:
                for b8 in range(4):
                    co[b8 * 64 + 1], co[b8 * 64 + 8] = _ac_pair(rng, 1500, 2500)
            else:
                for zb in range(16):
                    co[zb * 16 + 1], co[zb * 16 + 4] = _ac_pair(rng, 2000, 4000)
            for b in range(8):
                co[256 + b * 16 + 1], co[256 + b * 16 + 4] = _ac_pair(rng, 2000, 4000)
            m["cbp"] = 15 | (2 << 4)
            D.set_nzc(m, co)
        cases.append(c)
    return cases


FILTER_QP = 51


def filtered(case):
    """the same records under deblock_idc 0 with the filter as strong as it gets (QP 51, offsets +12: alpha 255, beta 18)"""
    c = copy.copy(case)
    c.f = copy.copy(case.f)
    c.f.mbs, c.f.slices = case.f.mbs.copy(), case.f.slices.copy()
    c.f.slices["deblock_idc"], c.f.slices["alpha_c0_offset"], c.f.slices["beta_offset"] = 0, 12, 12
    c.f.mbs["qp_y"], c.f.mbs["qp_c"] = FILTER_QP, FILTER_QP
    c.name, c.family, c.source_family, c.zero_residual_unfiltered, c._cache = case.name + " filtered", "filtered", case.family, False, {}
    return c


_families = {}


def families():
    """family -> [Case]"""
    if not _families:
        _families.update({"i4": build_i4(), "i8": build_i8(), "i16c": build_i16c(), "pos": build_pos(), "res": build_res()})
        _families["filtered"] = [filtered(c) for fam in ("i4", "i8", "i16c", "pos") for c in _families[fam]]
    return _families


# ---- coverage cells -----------------------------------------------------------------------------------------------------------------------
PLANE_CELLS = ("Hpos", "Hneg", "Vpos", "Vneg", "Hfrac", "Vfrac", "clip0", "clip255")


def all_cell_names():
    names = ["i4/%s/%d%d" % (M.MODE_NAMES[m], b & 3, b >> 2) for b, lst in enumerate(i4_valid(15)) for m in lst]
    names += ["i4top/%s/%d%d" % (M.MODE_NAMES[m], bx, by) for m in TOP_MODES for by in range(4) for bx in range(4) if bx < 3 or by == 0]
    i8 = set()
    for avail in range(16):
        ftl, ftr = M.i8_flags(avail)
        i8 |= {(m, b, ftl[b], ftr[b]) for b, lst in enumerate(i8_valid(avail)) for m in lst}
    names += ["i8/%s/%d/%d%d" % (M.MODE_NAMES[m], b, tl, tr) for (m, b, tl, tr) in sorted(i8)]
    names += ["i16/%d" % m for m in range(7)] + ["i16p/" + n for n in PLANE_CELLS]
    names += ["c/%s/%d" % (p, m) for p in ("cb", "cr") for m in range(7)] + ["cp/" + n for n in PLANE_CELLS]
    names += ["cdc/%d/q%d" % (m, q) for m in (M.C_DC, M.C_DC_L, M.C_DC_T) for q in range(4)]
    for place, avails in sorted(pos_avail().items()):
        for a in sorted(avails):
            names += ["pos/%s/i4/%s" % (place, M.MODE_NAMES[m]) for m in sorted({m for lst in i4_valid(a) for m in lst})]
            names += ["pos/%s/i8/%s" % (place, M.MODE_NAMES[m]) for m in sorted({m for lst in i8_valid(a) for m in lst})]
            names += ["pos/%s/i16/%d" % (place, m) for m in i16_valid(a)] + ["pos/%s/c/%d" % (place, m) for m in chroma_valid(a)]
    names += ["res/%s/%s" % (ph, e) for ph in ("i4", "i8", "i16", "c") for e in ("lo", "hi")]
    names += ["i4res/" + n for n in ("L", "T", "TL", "TR", "all_blocks")]
    names += ["filt/" + fam for fam in ("i4", "i8", "i16c", "pos")]
    return sorted(set(names))


def _plane_cells(prefix, plane, x0, y0, n, hit):
    hh, vv, b, c, raw = M.plane_terms(plane, x0, y0, n)
    k = 5 if n == 16 else 34
    for name, ok in (("Hpos", hh > 0), ("Hneg", hh < 0), ("Vpos", vv > 0), ("Vneg", vv < 0), ("Hfrac", k * hh + 32 < 0 and (k * hh + 32) % 64 != 0),
                     ("Vfrac", k * vv + 32 < 0 and (k * vv + 32) % 64 != 0), ("clip0", raw.min() < 0), ("clip255", raw.max() > 255)):
        if ok:
            hit[prefix + name] = hit.get(prefix + name, 0) + 1


def _neighbours(plane, x0, y0, n, right):
    """the samples an n x n macroblock can read: the row above it from its top-left corner to `right` samples beyond it, the column left"""
    h, w = plane.shape
    row = plane[y0 - 1, max(x0 - 1, 0):min(x0 + n + right, w)] if y0 > 0 else plane[0, :0]
    col = plane[y0:y0 + n, x0 - 1] if x0 > 0 else plane[:0, 0]
    return np.concatenate([row, col])


def cells(case):
    """cell name -> how often the case reaches it"""
    hit = {}

    def add(n):
        hit[n] = hit.get(n, 0) + 1
    fam = case.family
    if fam == "filtered":
        import oracle_lib as O
        fin, pre = case.oracle(0), case.oracle(O.NO_DEBLOCK)
        for (x, y, _, _) in case.sites:
            for p, bs in enumerate((16, 8, 8)):
                if not np.array_equal(_neighbours(fin.plane(p), bs * x, bs * y, bs, bs // 2), _neighbours(pre.plane(p), bs * x, bs * y, bs, bs // 2)):
                    add("filt/" + case.source_family)
                    break
        return hit
    preds = {}
    final = case.model(preds=preds) if case.residual else case.model()
    for (x, y, avail, place) in case.sites:
        m = case.record(x, y)
        typ, mode, cm = int(m["mb_type"]), [int(v) for v in m["intra_mode"]], int(m["chroma_mode"])
        x0, y0 = 16 * x, 16 * y
        if fam == "pos":
            used = set(mode) if typ == I4 else {mode[0], mode[2], mode[8], mode[10]} if typ == I8 else {mode[0]}
            for md in used:
                add("pos/%s/%s/%s" % (place, TYPE_NAME[typ], md if typ == I16 else M.MODE_NAMES[md]))
            add("pos/%s/c/%d" % (place, cm))
            continue
        if fam == "res":
            res = case.residual_of(x, y)
            got = case.oracle(0)
            for ph, p, bs in ((TYPE_NAME[typ], 0, 16), ("c", 1, 8), ("c", 2, 8)):
                want = preds[(x, y)][p] + res[p]
                out = got.plane(p)[bs * y:bs * y + bs, bs * x:bs * x + bs]
                if ((want < 0) & (out == 0)).any():
                    add("res/%s/lo" % ph)
                if ((want > 255) & (out == 255)).any():
                    add("res/%s/hi" % ph)
            if typ == I4:
                nz = [bool(res[0][4 * (b >> 2):4 * (b >> 2) + 4, 4 * (b & 3):4 * (b & 3) + 4].any()) for b in range(16)]
                if all(nz):
                    add("i4res/all_blocks")
                    for b in range(16):
                        bx, by, md = b & 3, b >> 2, mode[b]
                        corner = md in (M.DDR, M.VR, M.HD)
                        if bx > 0 and (corner or md in (M.H, M.HU, M.DC, M.DC_L)):
                            add("i4res/L")
                        if by > 0 and (corner or md in (M.V, M.DC, M.DC_T, M.DDL, M.VL, M.DDL_TOP, M.VL_TOP)):
                            add("i4res/T")
                        if bx > 0 and by > 0 and corner:
                            add("i4res/TL")
                        if by > 0 and md in (M.DDL, M.VL):
                            add("i4res/TR")
            continue
        if typ == I4:
            for b in range(16):
                bx, by, md = b & 3, b >> 2, mode[b]
                add("i4/%s/%d%d" % (M.MODE_NAMES[md], bx, by))
                if md in TOP_MODES and (bx < 3 or by == 0):
                    row = final[0][y0 + 4 * by - 1]
                    if (row[x0 + 4 * bx + 4:x0 + 4 * bx + 8] != row[x0 + 4 * bx + 3]).any():
                        add("i4top/%s/%d%d" % (M.MODE_NAMES[md], bx, by))
        elif typ == I8:
            ftl, ftr = M.i8_flags(avail)
            for i8 in range(4):
                add("i8/%s/%d/%d%d" % (M.MODE_NAMES[mode[((i8 >> 1) << 3) + ((i8 & 1) << 1)]], i8, ftl[i8], ftr[i8]))
        else:
            add("i16/%d" % mode[0])
            if mode[0] == M.I16_P:
                _plane_cells("i16p/", case.planes[0], x0, y0, 16, hit)
        cb, cr = final[1][8 * y:8 * y + 8, 8 * x:8 * x + 8], final[2][8 * y:8 * y + 8, 8 * x:8 * x + 8]
        if cm == M.C_DC_128 or not np.array_equal(cb, cr):
            add("c/cb/%d" % cm)
            add("c/cr/%d" % cm)
        if cm == M.C_P:
            _plane_cells("cp/", case.planes[1], 8 * x, 8 * y, 8, hit)
            _plane_cells("cp/", case.planes[2], 8 * x, 8 * y, 8, hit)
        if cm in (M.C_DC, M.C_DC_L, M.C_DC_T):
            su = M.chroma_dc_sums(M._at(M._padded(case.planes[1]), 8 * x, 8 * y))
            sv = M.chroma_dc_sums(M._at(M._padded(case.planes[2]), 8 * x, 8 * y))
            if len(set(su)) == 4 and len(set(sv)) == 4 and all(a != b for a, b in zip(su, sv)):
                for q in range(4):
                    qy, qx = 4 * (q >> 1), 4 * (q & 1)
                    if cb[qy, qx] != cr[qy, qx]:
                        add("cdc/%d/q%d" % (cm, q))
    return hit


# ---- what each wrong variant of the model must be told apart on ------------------------------------------------------------------------
_L4, _L8, _L16, _C = ("i4", "luma"), ("i8", "luma"), ("i16c", "luma"), ("i16c", "chroma")
VARIANT_PARTS = {"a": (_L4, _L8), "b": (_L8,), "c": (_L8,), "d": (_L8,), "e": (_L8,), "f": (_L4, _L8, _L16, _C), "g": (_L16, _C), "h": (_L16, _C),
                 "i": (_L16, _C), "j": (_C,), "k": (_C,), "l": (_L4,)}
