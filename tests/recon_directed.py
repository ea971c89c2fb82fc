"""Directed inputs of the reconstruct kernel (no GPU here): records built on purpose for the mechanisms the seeded random streams of
tests/synth.py reach only by chance - the motion-compensation arithmetic at its ends, the clamp of the vectors, the 64-macroblock
masks that decide which unfiltered lines a row publishes, the wave count and its LDS fallback, value ranges the generator never
draws, the boundary-strength thresholds and the wait for a reference picture still in flight.  Record layout and type constants
are those of tests/synth.py; tests/test_recon_directed.py proves with the oracle alone that every builder reaches what it claims,
tests/test_recon_directed_gpu.py runs them through the kernel."""
import numpy as np

import synth
from refdump import MB_DTYPE, SLICE_DTYPE
from synth import I4, I16, I8, P16, P16x8, P8x16, P8x8, SKIP, IPCM, SynFrame

PAD = 32
SUB_8x8, SUB_8x4, SUB_4x8, SUB_4x4 = 1, 2, 4, 8
# shape -> (mb_type, sub_type, partitions (ox, oy, w, h) in decoding order)
SHAPES = {
    "16x16": (P16, 0, [(0, 0, 16, 16)]),
    "16x8": (P16x8, 0, [(0, 0, 16, 8), (0, 8, 16, 8)]),
    "8x16": (P8x16, 0, [(0, 0, 8, 16), (8, 0, 8, 16)]),
    "8x8": (P8x8, SUB_8x8, [(qx, qy, 8, 8) for qy in (0, 8) for qx in (0, 8)]),
    "8x4": (P8x8, SUB_8x4, [(qx, qy + j, 8, 4) for qy in (0, 8) for qx in (0, 8) for j in (0, 4)]),
    "4x8": (P8x8, SUB_4x8, [(qx + j, qy, 4, 8) for qy in (0, 8) for qx in (0, 8) for j in (0, 4)]),
    "4x4": (P8x8, SUB_4x4, [(qx + jx, qy + jy, 4, 4) for qy in (0, 8) for qx in (0, 8) for jy in (0, 4) for jx in (0, 4)]),
}


# ---- frames and records ---------------------------------------------------------------------------------------------------------------
def new_frame(fid, mb_w, mb_h, ref_ids=(), idc=0, n_slices=1, qp=26):
    """an empty picture: a P slice (an I slice without references) over zeroed records"""
    f = SynFrame()
    f.id, f.mb_w, f.mb_h, f.ref_ids = fid, mb_w, mb_h, list(ref_ids)
    n = mb_w * mb_h
    bounds = np.linspace(0, n, n_slices + 1).astype(int)
    f.slices = np.zeros(n_slices, dtype=SLICE_DTYPE)
    f.mbs = np.zeros(n, dtype=MB_DTYPE)
    for s in range(n_slices):
        sl = f.slices[s]
        sl["first_mb"], sl["n_mbs"] = bounds[s], bounds[s + 1] - bounds[s]
        sl["slice_type"] = 0 if f.ref_ids else 2
        sl["deblock_idc"] = idc
        sl["n_refs"] = max(len(f.ref_ids), 1)
        sl["luma_dc_weight"] = 16
        sl["ref_slot"][:] = -1
        sl["ref_slot"][:len(f.ref_ids)] = np.arange(len(f.ref_ids))
        f.mbs["slice_id"][bounds[s]:bounds[s + 1]] = s
    f.mbs["qp_y"] = qp
    f.mbs["qp_c"] = qp
    f.coeffs = np.zeros((n, 384), dtype=np.int16)
    f.covered = np.ones(n, dtype=np.uint8)
    return f


def set_inter(m, shape, vecs, ref=0):
    """macroblock record m becomes `shape` with one vector per partition (decoding order), every 4x4 block of a partition carrying it"""
    typ, sub, parts = SHAPES[shape]
    m["mb_type"], m["sub_type"], m["ref_idx"] = typ, sub, ref
    mv = np.zeros((16, 2), dtype=np.int16)
    for (ox, oy, w, h), v in zip(parts, vecs):
        for by in range(oy >> 2, (oy + h) >> 2):
            mv[by * 4 + (ox >> 2):by * 4 + ((ox + w) >> 2)] = v
    m["mv"] = mv


def set_nzc(m, c):
    """nonzero counts of record m from its coefficients c (raster layout; the DC of I16x16 and of chroma excluded), as synth does"""
    typ, t8 = int(m["mb_type"]), int(m["flags"]) & 1
    nz = np.zeros(24, dtype=np.uint8)
    if typ == IPCM:
        nz[:] = 16
    else:
        for zb in range(16):
            bx, by = (zb & 1) | ((zb >> 2) & 1) << 1, ((zb >> 1) & 1) | ((zb >> 3) & 1) << 1
            blk = c[(zb >> 2) * 64:(zb >> 2) * 64 + 64] if t8 else c[zb * 16:zb * 16 + 16]
            nz[by * 4 + bx] = min(np.count_nonzero(blk[1:] if (typ == I16 and not t8) else blk), 16)
        for j, k in enumerate([16, 17, 20, 21, 18, 19, 22, 23]):
            nz[k] = np.count_nonzero(c[256 + j * 16 + 1:256 + j * 16 + 16])
    m["nzc"] = nz


def set_residual(m, c, rng, amp=600, density=0.08):
    """random coefficients consistent with a random cbp (what a parser leaves behind), and their counts"""
    typ = int(m["mb_type"])
    t8 = int(m["flags"]) & 1
    cbp_l, cbp_c = int(rng.integers(0, 16)), int(rng.integers(0, 3))
    if typ == I16:
        cbp_l = int(rng.choice([0, 15]))
    c[:] = np.where(rng.random(384) < density, rng.integers(-amp, amp + 1, 384), 0)
    for b8 in range(4):
        if not (cbp_l >> b8) & 1:
            blk = c[b8 * 64:(b8 + 1) * 64]
            dc = blk[::16].copy()
            blk[:] = 0
            if typ == I16 and not t8:
                blk[::16] = dc
    if cbp_c == 0:
        c[256:] = 0
    elif cbp_c == 1:
        dc = c[256::16].copy()
        c[256:] = 0
        c[256::16] = dc
    m["cbp"] = cbp_l | (cbp_c << 4)
    set_nzc(m, c)


def random_inter(m, c, rng, nref=1, span=40, amp=600, density=0.08):
    shape = str(rng.choice(list(SHAPES)))
    set_inter(m, shape, rng.integers(-span, span + 1, (16, 2)))
    r = rng.integers(0, nref, 4)
    typ = int(m["mb_type"])
    m["ref_idx"] = r[0] if typ == P16 else (r[0], r[0], r[1], r[1]) if typ == P16x8 else (r[0], r[1], r[0], r[1]) if typ == P8x16 else r
    m["flags"] = 0
    set_residual(m, c, rng, amp, density)


# ---- content ---------------------------------------------------------------------------------------------------------------------------
TAP6 = np.array([255, 0, 255, 255, 0, 255], dtype=np.uint8)      # 1 -5 20 20 -5 1 over it: 10,710; over its complement: -2,550


def content_uniform(rng, h, w):
    return rng.integers(0, 256, (h, w)).astype(np.uint8)


def content_binary(rng, h, w):
    return rng.choice(np.array([0, 255], dtype=np.uint8), (h, w))


def content_tap_extreme(rng, h, w):
    """four vertical bands: rows of period 6 (255 0 255 255 0 255), their complement, columns of that period, their complement"""
    y, x = np.mgrid[0:h, 0:w]
    band = (x * 4) // w
    a, b = TAP6[y % 6], TAP6[x % 6]
    return np.where(band == 0, a, np.where(band == 1, 255 - a, np.where(band == 2, b, 255 - b))).astype(np.uint8)


def content_smooth_steps(rng, h, w):
    """smooth content with small steps at the 4-sample boundaries: the deblocking filters' conditions hold and their deltas are not 0"""
    y, x = np.mgrid[0:h, 0:w]
    base = int(rng.integers(60, 180))
    return np.clip(base + rng.integers(-3, 4, (h, w)) + 6 * ((x // 4) % 3) + 6 * ((y // 4) % 3), 0, 255).astype(np.uint8)


CONTENT = {"uniform": content_uniform, "binary": content_binary, "tap_extreme": content_tap_extreme, "smooth": content_smooth_steps}


def pcm_picture(mb_w, mb_h, y, u, v, fid=0):
    """an all-IPCM intra picture, not filtered (deblock_idc 1): its reconstruction IS the given planes"""
    f = new_frame(fid, mb_w, mb_h, (), idc=1, qp=0)
    f.mbs["mb_type"], f.mbs["flags"], f.mbs["nzc"], f.mbs["chroma_mode"] = IPCM, 2, 16, 6
    y, u, v = (np.asarray(p, dtype=np.uint8) for p in (y, u, v))
    assert y.shape == (mb_h * 16, mb_w * 16) and u.shape == v.shape == (mb_h * 8, mb_w * 8)
    f.coeffs[:, :256] = y.reshape(mb_h, 16, mb_w, 16).transpose(0, 2, 1, 3).reshape(-1, 256)
    f.coeffs[:, 256:320] = u.reshape(mb_h, 8, mb_w, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    f.coeffs[:, 320:] = v.reshape(mb_h, 8, mb_w, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    return f


def pcm_content(rng, mb_w, mb_h, content, fid=0):
    fn = CONTENT[content]
    return pcm_picture(mb_w, mb_h, fn(rng, mb_h * 16, mb_w * 16), fn(rng, mb_h * 8, mb_w * 8), fn(rng, mb_h * 8, mb_w * 8), fid)


# ---- motion compensation --------------------------------------------------------------------------------------------------------------
GRID_W, GRID_H = 64, 16


def grid_vectors(x, y, shape, mixed=False):
    """the vectors of macroblock (x, y) of the grid, one per partition of `shape`"""
    n = len(SHAPES[shape][2])
    return [(x - 32 + (5 * i if mixed else 0), y - 8 + (3 * i if mixed else 0)) for i in range(n)]


def mc_grid(shape, content, mixed=False, seed=1):
    """[PCM reference, P picture]: zero residual, not filtered; macroblock (x, y) of the 64x16 picture carries mvx = x - 32 and
    mvy = y - 8 in every partition of `shape`: all 16 luma and 64 chroma fractions, both signs, every byte alignment of the fetches.
    mixed: partition i of a macroblock adds (5i, 3i), so one wave holds strips of different fractions."""
    rng = np.random.default_rng(seed)
    ref = pcm_content(rng, GRID_W, GRID_H, content)
    f = new_frame(1, GRID_W, GRID_H, [0], idc=1)
    for k in range(GRID_W * GRID_H):
        set_inter(f.mbs[k], shape, grid_vectors(k % GRID_W, k // GRID_W, shape, mixed))
    return [ref, f]


def clamp_bounds(mb_w, mb_h):
    """BaseMC's bounds of the absolute quarter-sample position (rec_mb.cpp:251-252): (lo, hi_x, hi_y)"""
    return (-PAD + 2) * 4, (mb_w * 16 + PAD - 19) * 4, (mb_h * 16 + PAD - 19) * 4


def border_targets(mb_w, mb_h):
    """(name, absolute x, absolute y) in quarter samples; None: an ordinary position.  On each bound, from 3 inside it to 1 beyond."""
    lo, hx, hy = clamp_bounds(mb_w, mb_h)
    out = []
    for d in range(-3, 2):
        out += [("x_lo%+d" % d, lo - d, None), ("x_hi%+d" % d, hx + d, None), ("y_lo%+d" % d, None, lo - d), ("y_hi%+d" % d, None, hy + d),
                ("tl%+d" % d, lo - d, lo - d), ("tr%+d" % d, hx + d, lo - d), ("bl%+d" % d, lo - d, hy + d), ("br%+d" % d, hx + d, hy + d)]
    return out


def mc_border(mb_w, mb_h, seed=2):
    """-> (frames, cases): a PCM picture of random content (so the padding is not uniform) and P pictures over it whose macroblocks
    each take one target of border_targets as 16x16 or as sixteen 4x4 partitions that all land on the same absolute position;
    cases[i] = (frame index, macroblock, name, shape)"""
    rng = np.random.default_rng(seed)
    frames = [pcm_content(rng, mb_w, mb_h, "uniform")]
    todo = [(t, shape) for shape in ("16x16", "4x4") for t in border_targets(mb_w, mb_h)]
    n = mb_w * mb_h
    cases = []
    for i0 in range(0, len(todo), n):
        f = new_frame(len(frames), mb_w, mb_h, [0], idc=1)
        for k, ((name, ax, ay), shape) in enumerate(todo[i0:i0 + n]):
            x, y = k % mb_w, k // mb_w
            vecs = []
            fill = rng.integers(-9, 10, 2)
            for (ox, oy, _, _) in SHAPES[shape][2]:
                vx = ax - 4 * (16 * x + ox) if ax is not None else fill[0]
                vy = ay - 4 * (16 * y + oy) if ay is not None else fill[1]
                vecs.append((vx, vy))
            set_inter(f.mbs[k], shape, vecs)
            cases.append((len(frames), k, name, shape))
        for k in range(len(todo[i0:i0 + n]), n):
            set_inter(f.mbs[k], "16x16", [(0, 0)])
        frames.append(f)
    return frames, cases


# ---- the 64-macroblock masks of a row -------------------------------------------------------------------------------------------------
def mask_columns(mb_w):
    return sorted(c for c in set([0, 1, 61, 62, 63, 64, 65, 66] + list(range(125, 131)) + [mb_w - 2, mb_w - 1]) if 0 <= c < mb_w)


def directed_intra(m, kind, x, mb_w):
    """an intra macroblock of a row > 0 that reads the unfiltered bottom rows of (x-1, x, x+1) above and the left neighbour's right
    column, as far as they exist.  kind 0: I4x4 (block 0 diagonal-down-right: top-left; block (3,0) diagonal-down-left: top-right),
    1: I8x8 (the same through the reference-sample filter), 2: I16x16 plane, 3: chroma plane."""
    left, tr = x > 0, x + 1 < mb_w
    m["flags"], m["cbp"], m["nzc"], m["intra_avail"] = 0, 0, 0, 0
    m["intra_mode"] = 0
    m["chroma_mode"] = 0 if left else 2                        # DC / vertical
    if kind == 0:
        m["mb_type"] = I4
        mode = np.full(16, 2 if left else 0, dtype=np.int8)    # DC / vertical
        mode[[4, 8, 12]] = 1 if left else 0                    # left column: horizontal
        mode[0] = 4 if left else 7                             # DDR (top-left) / VL (top + top-right)
        mode[3] = 3 if tr else 12                              # DDL with / without top-right
        m["intra_mode"] = mode
    elif kind == 1:
        m["mb_type"], m["flags"] = I8, 1
        m["intra_avail"] = 1 | (2 if left else 0) | (4 if left else 0) | (8 if tr else 0)
        mode = np.zeros(16, dtype=np.int8)
        mode[0] = 4 if left else 7                             # 8x8 block 0
        mode[2] = 3 if tr else 12                              # block 1
        mode[8] = 1 if left else 0                             # block 2
        mode[10] = 2                                           # block 3
        m["intra_mode"] = mode
    elif kind == 2:
        m["mb_type"] = I16
        m["intra_mode"][0] = 3 if left else 0                  # plane / vertical
    else:
        m["mb_type"] = I16
        m["intra_mode"][0] = 2 if left else 0                  # DC / vertical
        m["chroma_mode"] = 3 if left else 2                    # plane / vertical


def _mask_placements(mb_w):
    """pictures x rows 1, 2 -> columns, so that every column of mask_columns carries an isolated macroblock in row 1 of some picture
    and in row 2 of some picture: at least 4 columns between two of a row, rows 1 and 2 at least 2 columns apart"""
    cols = mask_columns(mb_w)
    pend = {1: list(cols), 2: list(reversed(cols))}
    out = []
    while pend[1] or pend[2]:
        put = {1: [], 2: []}
        for r in (1, 2):
            for c in list(pend[r]):
                if all(abs(c - o) >= 5 for o in put[r]) and all(abs(c - o) >= 2 for o in put[3 - r]):
                    put[r].append(c)
                    pend[r].remove(c)
        out.append(put)
    return out


def row_masks(mb_w, complement=False, seed=3):
    """[PCM picture, P pictures of 3 rows]: every macroblock inter (random shapes, vectors, residuals) except isolated directed intra
    macroblocks in rows 1 and 2 at the columns where the kernel's 64-bit row masks have their special cases.  complement: every
    macroblock intra (random, from synth) except isolated inter macroblocks at the same places."""
    rng = np.random.default_rng(seed * 1000 + mb_w + (500 if complement else 0))
    frames = [pcm_content(rng, mb_w, 3, "uniform")]
    kind = 0
    for put in _mask_placements(mb_w):
        fid = len(frames)
        if complement:
            f = synth.make_stream(int(rng.integers(1 << 30)), mb_w, 3, 1, p_frames=False, t8=True)[0]
            f.id, f.ref_ids = fid, [fid - 1]
            f.slices["slice_type"], f.slices["ref_slot"][0, 0] = 0, 0
        else:
            f = new_frame(fid, mb_w, 3, [fid - 1])
            for k in range(3 * mb_w):
                random_inter(f.mbs[k], f.coeffs[k], rng)
        f.placed = put
        for r in (1, 2):
            for c in put[r]:
                k = r * mb_w + c
                if complement:
                    f.mbs[k]["intra_mode"], f.mbs[k]["intra_avail"], f.mbs[k]["chroma_mode"] = 0, 0, 0
                    random_inter(f.mbs[k], f.coeffs[k], rng)
                else:
                    f.coeffs[k] = 0
                    f.mbs[k]["mv"], f.mbs[k]["ref_idx"], f.mbs[k]["sub_type"] = 0, 0, 0
                    directed_intra(f.mbs[k], kind & 3, c, mb_w)
                    kind += 1
        frames.append(f)
    return frames


MASK_WIDTHS = (63, 64, 65, 66, 127, 128, 129, 130)


# ---- wave counts ----------------------------------------------------------------------------------------------------------------------
def wave_thresholds(rows=9):
    """from the product (lh264_debug_recon_geometry): {waves: the last width that still runs on that many}, for pictures of `rows` rows"""
    from losslessh264_amd import _lib
    last = {}
    for nw in (8, 4, 2, 1):
        lo, hi = 1, 4096                       # the wave count does not grow with the width: bisect the last width with >= nw waves
        while lo < hi:
            mid = (lo + hi + 1) // 2
            rc, w, _ = _lib.recon_geometry(mid, rows)
            if rc == 0 and w >= nw:
                lo = mid
            else:
                hi = mid - 1
        last[nw] = lo
    return last


def wave_edge_widths(rows=9):
    """[(width, waves the launch must choose)]: both sides of every fallback, the last width of one wave, and a 4K picture"""
    t = wave_thresholds(rows)
    from losslessh264_amd import _lib
    return [(t[8], 8), (t[8] + 1, 4), (t[4], 4), (t[4] + 1, 2), (t[2], 2), (t[2] + 1, 1), (t[1], 1), (240, _lib.recon_geometry(240, rows)[1])]


def wave_edges(width, rows=9):
    """random I + P records of synth at one of the widths of wave_edge_widths: 9 rows, so 8 waves are wanted"""
    return synth.make_stream(seed=7000 + width, mb_w=width, mb_h=rows, n_frames=2)


# ---- ranges the generator never draws -------------------------------------------------------------------------------------------------
DC_WEIGHTS = (1, 6, 15, 17, 64, 255, 0)          # 0: what the parser emits without a scaling list; it means 16
DC_QPS = tuple(range(12)) + (51,)


def dc_amp_bound(qp, weight):
    """the largest |level| of the 16 luma DCs that keeps f * qmul of WelsLumaDcDequantIdct inside int32 (|f| <= 16 |level|; the
    reference adds 2 before its shift)"""
    import oracle_lib as O
    qmul = O.lib().orc_luma_dc_qmul(qp, weight if weight else 16)
    return min(32767, ((1 << 31) - 3) // (16 * max(qmul, 1)))


def ranges_dc_weight(seed=4):
    """one intra picture, one slice per scaling-list weight, two rows a slice: I16x16 at QP 0..11 and 51; the upper row carries DCs
    of the full amplitude in the four Hadamard sign patterns that put 16 |level| into one output, the lower row random ones"""
    rng = np.random.default_rng(seed)
    w, nsl = len(DC_QPS), len(DC_WEIGHTS)
    f = new_frame(0, w, 2 * nsl, (), idc=0, n_slices=nsl)
    f.slices["luma_dc_weight"] = DC_WEIGHTS
    f.slices["alpha_c0_offset"] = f.slices["beta_offset"] = 12
    blk_x, blk_y = [0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3], [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3]     # z-order -> raster
    had = [(1, 1, 1, 1), (1, 1, -1, -1), (1, -1, -1, 1), (1, -1, 1, -1)]
    for k in range(len(f.mbs)):
        x, y = k % w, k // w
        m, c = f.mbs[k], f.coeffs[k]
        qp, wt = DC_QPS[x], DC_WEIGHTS[y // 2]
        m["mb_type"], m["qp_y"], m["qp_c"] = I16, qp, qp
        m["intra_mode"][0] = (1 if x else 6) if y % 2 == 0 else (2 if x else 0)     # first row of a slice: no macroblock above
        m["chroma_mode"] = (1 if x else 6) if y % 2 == 0 else (0 if x else 2)
        amp = dc_amp_bound(qp, wt)
        if y % 2 == 0:
            sgn = -1 if (x + y // 2) & 1 else 1
            for zb in range(16):
                c[zb * 16] = sgn * amp * had[x & 3][blk_x[zb]] * had[(x >> 2) & 3][blk_y[zb]]
        else:
            c[0:256:16] = rng.integers(-amp, amp + 1, 16)
            c[:256] += np.where((rng.random(256) < 0.1) & (np.arange(256) % 16 != 0), rng.integers(-300, 301, 256), 0).astype(np.int16)
        m["cbp"] = 15 if np.count_nonzero(np.delete(c[:256].reshape(16, 16), 0, axis=1)) else 0
        set_nzc(m, c)
    return [f]


def ranges_low_qp(seed=5):
    """every macroblock type of synth at qp_y 0..9 (filter offsets of +12 keep the loop filter awake from QP 4 on)"""
    rng = np.random.default_rng(seed)
    frames = synth.make_stream(seed=9100 + seed, mb_w=8, mb_h=6, n_frames=3, t8=True, pcm=True, n_slices=2)
    for f in frames:
        f.mbs["qp_y"] = rng.integers(0, 10, len(f.mbs))
        f.mbs["qp_c"] = rng.integers(0, 10, (len(f.mbs), 2))
        f.slices["alpha_c0_offset"] = f.slices["beta_offset"] = 12
    return frames


def ranges_t8_saturating(density, seed=6):
    """8x8 transform (intra and inter) with coefficients up to +-32767: the int16 stores between its two passes wrap"""
    return synth.make_stream(seed=9200 + seed + int(density * 10), mb_w=6, mb_h=4, n_frames=2, t8=True, amp=32767, density=density)


WP_EXTREMES = (-128, -1, 0, 1, 127)
WP_DENOMS = [(a, b) for a in (0, 1, 7) for b in (0, 1, 7)]


def _wp_values(rng):
    """16 distinct values of -128..127, the five extremes among them, in random order"""
    rest = [v for v in rng.permutation(np.arange(-128, 128)) if v not in WP_EXTREMES][:11]
    return rng.permutation(np.array(list(WP_EXTREMES) + rest))


def ranges_refs16(weighted=False, seed=7, mb_w=4, mb_h=3):
    """a chain of 17 pictures in which the reference lists grow to 16 entries, ref_slot is a permutation and picture 16 uses every
    ref_idx 0..15; then picture 17, where two indices name one picture, and picture 18, where ref_slot[k] = -1 for used k > 0 (the
    partition predicts from list entry 0; ref_slot[0] >= 0 always).  weighted: every P slice weights explicitly, denominators from
    {0, 1, 7}, weights and offsets from -128..127 with the extremes, distinct per ref_idx."""
    rng = np.random.default_rng(seed + (50 if weighted else 0))
    n = mb_w * mb_h
    frames = [synth.make_stream(seed=9300 + seed, mb_w=mb_w, mb_h=mb_h, n_frames=1, p_frames=False)[0]]
    for fi in range(1, 19):
        nref = min(fi, 16)
        f = new_frame(fi, mb_w, mb_h, [fi - 1 - k for k in range(nref)])
        sl = f.slices[0]
        sl["ref_slot"][:nref] = rng.permutation(nref)
        use = np.arange(n * 4) % nref                           # every index the list has, in turn
        if fi == 17:
            sl["ref_slot"][5] = sl["ref_slot"][3]
            use = np.where(np.arange(n * 4) % 2 == 0, 3, 5)
        if fi == 18:
            sl["ref_slot"][[2, 7, 15]] = -1
            use = np.array([2, 7, 15, 0, 1, 7, 2, 15])[np.arange(n * 4) % 8]
        for k in range(n):
            m = f.mbs[k]
            random_inter(m, f.coeffs[k], rng, span=24)
            set_inter(m, "8x8" if k % 3 else "4x4", m["mv"][[0, 2, 8, 10] if k % 3 else [0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15]],
                      ref=use[4 * k:4 * k + 4])
        if weighted:
            sl["weighted_pred"] = 1
            sl["luma_log2_denom"], sl["chroma_log2_denom"] = WP_DENOMS[(fi - 1) % 9]
            sl["luma_weight"], sl["luma_offset"] = _wp_values(rng), _wp_values(rng)
            sl["chroma_weight"] = np.stack([_wp_values(rng), _wp_values(rng)], axis=1)
            sl["chroma_offset"] = np.stack([_wp_values(rng), _wp_values(rng)], axis=1)
        frames.append(f)
    return frames


def ranges():
    """name -> frames"""
    return {"dc_weight": ranges_dc_weight(), "low_qp": ranges_low_qp(), "t8_density0.5": ranges_t8_saturating(0.5),
            "t8_density1.0": ranges_t8_saturating(1.0), "refs16": ranges_refs16(False), "refs16_weighted": ranges_refs16(True)}


def check_refs_defined(frames):
    """the rule of include/lh264.h: no inter macroblock in a slice without ref_slot[0], none in a picture without references"""
    for f in frames:
        inter = (f.mbs["mb_type"] & 0x1F8) != 0
        if inter.any():
            assert len(f.ref_ids) > 0, "picture %d: inter macroblocks without a reference picture" % f.id
            bad = inter & (f.slices["ref_slot"][f.mbs["slice_id"], 0] < 0)
            assert not bad.any(), "picture %d: inter macroblock %d in a slice whose ref_slot[0] < 0" % (f.id, int(np.nonzero(bad)[0][0]))


# ---- boundary strengths ---------------------------------------------------------------------------------------------------------------
BS_QP = 40


class BsCase:
    """frames: [PCM, (PCM,) P]; edge: (macroblock x, y, dir (0: vertical edge), edge 0..3, segments) of the P picture's edge the case is
    about; filtered: whether the reference filters it (boundary strength > 0)"""

    def __init__(self, name, frames, edge, filtered):
        self.name, self.frames, self.edge, self.filtered = name, frames, edge, filtered


def _bs_base(rng, two_refs=False, same_picture=False):
    frames = [pcm_content(rng, 3, 3, "smooth", 0)]
    if two_refs:
        frames.append(pcm_content(rng, 3, 3, "smooth", 1))
    f = new_frame(len(frames), 3, 3, [0, 1] if two_refs else [0], idc=0, qp=BS_QP)
    if same_picture:
        f.slices["ref_slot"][0, :2] = 0
    for k in range(9):
        set_inter(f.mbs[k], "16x16", [(0, 0)])
    frames.append(f)
    return frames, f


def _split(shape, dir_, e, va, vb):
    """vectors of `shape`: va for the partitions before edge e (left of a vertical edge, above a horizontal one), vb from it on"""
    return [vb if (ox if dir_ == 0 else oy) >= 4 * e else va for (ox, oy, _, _) in SHAPES[shape][2]]


def bs_thresholds(seed=8):
    """-> list of BsCase.  Pairs `name/3` and `name/4`: two adjacent partitions whose vectors differ by exactly 3 (not filtered) or
    exactly 4 (filtered) quarter samples in one axis; then reference indices, the 8x8-transform remaps, P16x16 and SKIP."""
    rng = np.random.default_rng(seed)
    cases = []
    C = 4          # the macroblock the cases are about: (1, 1) of 3x3
    internal = [("4x4", d, e) for d in (0, 1) for e in (1, 2, 3)] + [("8x8", 0, 2), ("8x8", 1, 2), ("16x8", 1, 2), ("8x16", 0, 2)]
    for axis in (0, 1):
        for diff in (3, 4):
            v = (diff, 0) if axis == 0 else (0, diff)
            sign = -1 if rng.random() < 0.5 else 1
            v = (sign * v[0], sign * v[1])
            for shape, d, e in internal:
                frames, f = _bs_base(rng)
                set_inter(f.mbs[C], shape, _split(shape, d, e, (0, 0), v))
                cases.append(BsCase("internal %s dir%d edge%d %s/%d" % (shape, d, e, "xy"[axis], diff), frames, (1, 1, d, e, (0, 1, 2, 3)), diff == 4))
            for d in (0, 1):                                   # the macroblock's left / top edge
                frames, f = _bs_base(rng)
                set_inter(f.mbs[C], "16x16", [v])
                set_inter(f.mbs[C + 1], "16x16", [v]); set_inter(f.mbs[C + 3], "16x16", [v])
                cases.append(BsCase("mb edge dir%d %s/%d" % (d, "xy"[axis], diff), frames, (1, 1, d, 0, (0, 1, 2, 3)), diff == 4))
            # the 8x8-transform remap of the vectors at a macroblock edge (deblocking.cpp:273-352): a side with the flag is read at the
            # first 4x4 block of its 8x8 block.  Those blocks carry the pair under test; the other blocks along the edge carry the
            # opposite decision (3 where the pair differs by 4, 4 where it differs by 3).
            other = tuple(c * (7 - diff) // diff for c in v)
            for d in (0, 1):
                for t8c, t8n in ((1, 0), (0, 1), (1, 1)):
                    frames, f = _bs_base(rng)
                    cur, nb = f.mbs[C], f.mbs[C - 1 if d == 0 else C - 3]
                    mvc, mvn = np.zeros((16, 2), np.int16), np.zeros((16, 2), np.int16)
                    for seg in range(4):
                        bc, bn = (seg * 4, seg * 4 + 3) if d == 0 else (seg, 12 + seg)
                        rc = ((seg >> 1) * 8 if d == 0 else (seg >> 1) * 2) if t8c else bc
                        rn = ((seg >> 1) * 8 + 2 if d == 0 else 8 + (seg >> 1) * 2) if t8n else bn
                        if bc != rc:
                            mvc[bc] = other
                        if bn != rn:
                            mvn[bn] = tuple(a - b for a, b in zip(v, other))
                        mvc[rc] = v
                    for m, mv, t8 in ((cur, mvc, t8c), (nb, mvn, t8n)):
                        m["mb_type"], m["sub_type"], m["flags"], m["mv"] = P8x8, SUB_4x4, t8, mv
                    cases.append(BsCase("t8 cur%d nb%d dir%d %s/%d" % (t8c, t8n, d, "xy"[axis], diff), frames, (1, 1, d, 0, (0, 1, 2, 3)), diff == 4))
    for d in (0, 1):
        for same in (False, True):
            # equal vectors, different reference indices: the reference compares the INDICES (deblocking.cpp:58-63), so the edge is
            # filtered even where both indices name one picture
            frames, f = _bs_base(rng, two_refs=True, same_picture=same)
            shape = "8x16" if d == 0 else "16x8"
            set_inter(f.mbs[C], shape, [(0, 0), (0, 0)])
            f.mbs[C]["ref_idx"] = (0, 1, 0, 1) if d == 0 else (0, 0, 1, 1)
            cases.append(BsCase("ref_idx internal dir%d %s" % (d, "one picture" if same else "two pictures"), frames, (1, 1, d, 2, (0, 1, 2, 3)), True))
            frames, f = _bs_base(rng, two_refs=True, same_picture=same)
            f.mbs[C]["ref_idx"] = 1
            cases.append(BsCase("ref_idx mb edge dir%d %s" % (d, "one picture" if same else "two pictures"), frames, (1, 1, d, 0, (0, 1, 2, 3)), True))
        # the 8x8-transform remap of the nonzero counts: the neighbour's only count sits in a 4x4 block of the edge's 8x8 block that
        # does not touch the edge
        for have in (True, False):
            frames, f = _bs_base(rng)
            nb = f.mbs[C - 1 if d == 0 else C - 3]
            nb["flags"] = 1
            if have:
                blk8 = 1 if d == 0 else 2                      # top-right / bottom-left 8x8 block of the neighbour: segments 0, 1
                f.coeffs[C - 1 if d == 0 else C - 3][blk8 * 64 + 9] = 40
                nb["cbp"] = 1 << blk8
                nb["nzc"][2 if d == 0 else 8] = 1
            cases.append(BsCase("t8 nz remap dir%d %s" % (d, "coefficient" if have else "none"), frames, (1, 1, d, 0, (0, 1)), have))
    for typ, name in ((P16, "P16x16"), (SKIP, "SKIP")):        # vectors inside are not compared (mv_too false / skipped)
        for d in (0, 1):
            frames, f = _bs_base(rng)
            m = f.mbs[C]
            set_inter(m, "4x4", _split("4x4", d, 2, (0, 0), (4, 4)))
            m["mb_type"], m["sub_type"] = typ, 0
            # (segments 1, 2: the outer ones are also touched by the filtered macroblock edges that cross this one)
            cases.append(BsCase("%s internal dir%d" % (name, d), frames, (1, 1, d, 2, (1, 2)), False))
    return cases


def edge_samples(plane, edge):
    """the luma samples p0 | q0 on both sides of an edge's segments"""
    x, y, d, e, segs = edge
    out = []
    for s in segs:
        if d == 0:
            out.append(plane[16 * y + 4 * s:16 * y + 4 * s + 4, 16 * x + 4 * e - 1:16 * x + 4 * e + 1])
        else:
            out.append(plane[16 * y + 4 * e - 1:16 * y + 4 * e + 1, 16 * x + 4 * s:16 * x + 4 * s + 4])
    return np.stack(out)


# ---- a reference picture still in flight ----------------------------------------------------------------------------------------------
def in_flight_rows(f, fi):
    """per macroblock of P picture fi of in_flight: (integer row Y of the reference its first sample comes from, fraction)"""
    lo, _, hy = clamp_bounds(f.mb_w, f.mb_h)
    out = []
    for k in range(len(f.mbs)):
        fy = min(max(4 * 16 * (k // f.mb_w) + int(f.mbs[k]["mv"][0][1]), lo), hy)
        out.append((fy >> 2, fy & 3))
    return out


def in_flight(mb_w, mb_h, seed=9):
    """6 pictures, each P picture predicted from the one before it - the picture the kernel may still be writing.  Odd pictures point
    as far down as the clamp allows (bound - 0..3: zero and nonzero fractions).  Even pictures point where the last reference row a
    macroblock needs crosses a macroblock-row boundary: for a 16x16 block from row Y that is Y + 18 under a vertical fraction, Y + 15
    without one, and Y + 16 where the chroma term decides (no luma fraction, Y odd) - each on 16k + 15 for some macroblocks and
    beyond it for others."""
    rng = np.random.default_rng(seed * 100 + mb_h)
    frames = [synth.make_stream(seed=9400 + mb_h, mb_w=mb_w, mb_h=mb_h, n_frames=1, p_frames=False)[0]]
    _, _, hy = clamp_bounds(mb_w, mb_h)
    for fi in range(1, 6):
        f = new_frame(fi, mb_w, mb_h, [fi - 1])
        for k in range(mb_w * mb_h):
            x, y = k % mb_w, k // mb_w
            if fi & 1:
                ay = hy - int(rng.integers(0, 4))
            else:
                kk = min(y + 1 + int(rng.integers(0, 2)), mb_h - 1)
                rel, frac = [(-3, 1), (-2, 2), (-3, 3), (-2, 1), (0, 0), (1, 0), (-1, 0), (0, 0)][int(rng.integers(0, 8))]
                ay = 4 * (16 * kk + rel) + frac
            vx = int(rng.integers(-20, 21))
            shape = "16x16" if (x + y + fi) % 3 else "4x4"
            random_inter(f.mbs[k], f.coeffs[k], rng)
            set_inter(f.mbs[k], shape, [(vx, ay - 4 * (16 * y + oy)) for (_, oy, _, _) in SHAPES[shape][2]])
        frames.append(f)
    return frames
