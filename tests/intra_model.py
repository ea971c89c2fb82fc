"""An independent model of H.264 intra prediction (no GPU, no C): the predictors of Intra4x4 (8.3.1.2), Intra8x8 with its reference-sample
filter (8.3.2.2), Intra16x16 (8.3.3) and chroma (8.3.4) stated from the standard's formulas in plain Python integers, written from
neither the kernel nor oracle/oracle_recon.c.  predict_mb predicts one macroblock from a picture's unfiltered samples; the I4x4 and
I8x8 blocks run in z-order and each reads what the blocks before it wrote.  It is defined for records whose modes respect
availability (modes numbered as include/lh264.h numbers them) and, without `residual`, for zero residual, where the reconstruction
IS the prediction.

`variant` selects a deliberately WRONG alternative (VARIANTS): what a kernel could plausibly compute instead.  tests/test_intra_directed.py
demands that the directed inputs of tests/intra_directed.py tell every one of them from the true model - that is what makes the GPU
comparison able to fail."""
import numpy as np

V, H, DC, DDL, DDR, VR, HD, VL, HU, DC_L, DC_T, DC_128, DDL_TOP, VL_TOP = range(14)
I16_V, I16_H, I16_DC, I16_P, I16_DC_L, I16_DC_T, I16_DC_128 = range(7)
C_DC, C_H, C_V, C_P, C_DC_L, C_DC_T, C_DC_128 = range(7)
MODE_NAMES = ["V", "H", "DC", "DDL", "DDR", "VR", "HD", "VL", "HU", "DC_L", "DC_T", "DC_128", "DDL_TOP", "VL_TOP"]
AVAIL_T, AVAIL_TL, AVAIL_L, AVAIL_TR = 1, 2, 4, 8
I4, I16, I8 = 1, 2, 4

VARIANTS = {
    "a": "*_TOP modes read the real top-right samples and do not replicate (I4, I8)",
    "b": "I8 low-pass: the top-left flag inverted for T'0 and L'0",
    "c": "I8 low-pass: T'7 with the top-right flag inverted",
    "d": "I8 low-pass: T'15 filtered like an inner sample",
    "e": "I8 low-pass skipped altogether",
    "f": "DC, DC_L and DC_T always sum both sides (I4, I8, I16, chroma)",
    "g": "plane prediction without the final clip",
    "h": "plane b and c with a division that truncates towards zero (luma, chroma)",
    "i": "plane H and V exchanged",
    "j": "chroma DC: the top-right and bottom-left quadrants use both sums",
    "k": "Cb and Cr sums exchanged",
    "l": "an I4 block of diagonal t reads its neighbours as they stood before diagonal t-1 was written",
}
MARGIN = 32
Z_X = [0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3]      # z-order index -> 4x4 block column / row (6.4.3)
Z_Y = [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3]


def clip1(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _padded(plane):
    """an int plane with a margin of 128s, so that a (wrong) variant may read beyond the picture"""
    return np.pad(np.asarray(plane, dtype=np.int64), MARGIN, mode="constant", constant_values=128)


def _at(P, x0, y0):
    return lambda x, y: int(P[y0 + y + MARGIN, x0 + x + MARGIN])


# ---- the directional predictors shared by 4x4 and 8x8 (8.3.1.2.4-9, 8.3.2.2.5-10); p(x, y): the (filtered) neighbours ---------------
def _directional(p, n, mode):
    out = np.zeros((n, n), dtype=np.int64)
    corner = lambda: (p(0, -1) + 2 * p(-1, -1) + p(-1, 0) + 2) >> 2
    for y in range(n):
        for x in range(n):
            if mode == DDL:
                if x == n - 1 and y == n - 1:
                    v = (p(2 * n - 2, -1) + 3 * p(2 * n - 1, -1) + 2) >> 2
                else:
                    v = (p(x + y, -1) + 2 * p(x + y + 1, -1) + p(x + y + 2, -1) + 2) >> 2
            elif mode == DDR:
                if x > y:
                    v = (p(x - y - 2, -1) + 2 * p(x - y - 1, -1) + p(x - y, -1) + 2) >> 2
                elif x < y:
                    v = (p(-1, y - x - 2) + 2 * p(-1, y - x - 1) + p(-1, y - x) + 2) >> 2
                else:
                    v = corner()
            elif mode == VR:
                z, i = 2 * x - y, x - (y >> 1)
                if z >= 0 and z % 2 == 0:
                    v = (p(i - 1, -1) + p(i, -1) + 1) >> 1
                elif z >= 0:
                    v = (p(i - 2, -1) + 2 * p(i - 1, -1) + p(i, -1) + 2) >> 2
                elif z == -1:
                    v = corner()
                else:
                    v = (p(-1, y - 2 * x - 1) + 2 * p(-1, y - 2 * x - 2) + p(-1, y - 2 * x - 3) + 2) >> 2
            elif mode == HD:
                z, i = 2 * y - x, y - (x >> 1)
                if z >= 0 and z % 2 == 0:
                    v = (p(-1, i - 1) + p(-1, i) + 1) >> 1
                elif z >= 0:
                    v = (p(-1, i - 2) + 2 * p(-1, i - 1) + p(-1, i) + 2) >> 2
                elif z == -1:
                    v = corner()
                else:
                    v = (p(x - 2 * y - 1, -1) + 2 * p(x - 2 * y - 2, -1) + p(x - 2 * y - 3, -1) + 2) >> 2
            elif mode == VL:
                i = x + (y >> 1)
                if y % 2 == 0:
                    v = (p(i, -1) + p(i + 1, -1) + 1) >> 1
                else:
                    v = (p(i, -1) + 2 * p(i + 1, -1) + p(i + 2, -1) + 2) >> 2
            elif mode == HU:
                z, i = x + 2 * y, y + (x >> 1)
                if z > 2 * n - 3:
                    v = p(-1, n - 1)
                elif z == 2 * n - 3:
                    v = (p(-1, n - 2) + 3 * p(-1, n - 1) + 2) >> 2
                elif z % 2 == 0:
                    v = (p(-1, i) + p(-1, i + 1) + 1) >> 1
                else:
                    v = (p(-1, i) + 2 * p(-1, i + 1) + p(-1, i + 2) + 2) >> 2
            else:
                raise ValueError("mode %d" % mode)
            out[y, x] = v
    return out


def _nxn(p, n, mode, variant):
    """V, H and the DC family on the neighbours p; everything else is directional"""
    if variant == "f" and mode in (DC_L, DC_T):
        mode = DC
    lg = {4: 2, 8: 3}[n]
    if mode == V:
        return np.array([[p(x, -1) for x in range(n)]] * n, dtype=np.int64)
    if mode == H:
        return np.array([[p(-1, y)] * n for y in range(n)], dtype=np.int64)
    if mode == DC_128:
        return np.full((n, n), 128, dtype=np.int64)
    top, left = sum(p(x, -1) for x in range(n)), sum(p(-1, y) for y in range(n))
    if mode == DC:
        return np.full((n, n), (top + left + n) >> (lg + 1), dtype=np.int64)
    if mode == DC_L:
        return np.full((n, n), (left + (n >> 1)) >> lg, dtype=np.int64)
    if mode == DC_T:
        return np.full((n, n), (top + (n >> 1)) >> lg, dtype=np.int64)
    return _directional(p, n, mode)


def pred4(P, x0, y0, mode, variant=None):
    """the 4x4 block at (x0, y0) of the padded plane P.  DDL_TOP / VL_TOP: the samples p[4..7, -1] are not available and
    p[3, -1] stands for them (8.3.1.2)"""
    g = _at(P, x0, y0)
    p = g
    if mode in (DDL_TOP, VL_TOP):
        if variant != "a":
            p = lambda x, y: g(3, -1) if (y == -1 and x > 3) else g(x, y)
        mode = DDL if mode == DDL_TOP else VL
    return _nxn(p, 4, mode, variant)


def pred8(P, x0, y0, mode, tl, tr, variant=None):
    """the 8x8 block at (x0, y0): the reference-sample filter of 8.3.2.2.1 over p[-1, 7..0], p[-1, -1], p[0..15, -1], then the
    predictor.  tl / tr: whether p[-1, -1] / p[8..15, -1] are available; a *_TOP mode says that the latter are not"""
    g = _at(P, x0, y0)
    top_var = mode in (DDL_TOP, VL_TOP)
    have_tr = (variant == "a") if top_var else bool(tr)
    if top_var:
        mode = DDL if mode == DDL_TOP else VL
    t = [g(x, -1) if (x < 8 or have_tr) else g(7, -1) for x in range(16)]
    l = [g(-1, y) for y in range(8)]
    c = g(-1, -1)
    if variant == "e":
        ft, fl, fc = t, l, c
    else:
        tlf = bool(tl) != (variant == "b")
        ft = [0] * 16
        ft[0] = (c + 2 * t[0] + t[1] + 2) >> 2 if tlf else (3 * t[0] + t[1] + 2) >> 2
        for x in range(1, 15):
            ft[x] = (t[x - 1] + 2 * t[x] + t[x + 1] + 2) >> 2
        ft[15] = (t[14] + 3 * t[15] + 2) >> 2
        if variant == "c":
            t8 = g(7, -1) if have_tr else g(8, -1)
            ft[7] = (t[6] + 2 * t[7] + t8 + 2) >> 2
        if variant == "d":
            t16 = g(16, -1) if have_tr else g(7, -1)
            ft[15] = (t[14] + 2 * t[15] + t16 + 2) >> 2
        fl = [0] * 8
        fl[0] = (c + 2 * l[0] + l[1] + 2) >> 2 if tlf else (3 * l[0] + l[1] + 2) >> 2
        for y in range(1, 7):
            fl[y] = (l[y - 1] + 2 * l[y] + l[y + 1] + 2) >> 2
        fl[7] = (l[6] + 3 * l[7] + 2) >> 2
        fc = (t[0] + 2 * c + l[0] + 2) >> 2
    p = lambda x, y: fc if (x == -1 and y == -1) else ft[x] if y == -1 else fl[y]
    return _nxn(p, 8, mode, variant)


def _shift_div(n, shift, variant):
    """n >> shift: the standard's arithmetic shift (a division that rounds towards minus infinity)"""
    if variant == "h" and n < 0:
        return -((-n) >> shift)
    return n >> shift


def _plane(g, s, n, variant):
    """8.3.3.4 (n = 16) and 8.3.4.4 (n = 8, 4:2:0): s supplies the samples of the sums H and V, g those of a"""
    h = n >> 1
    hh = sum((i + 1) * (s(h + i, -1) - s(h - 2 - i, -1)) for i in range(h))
    vv = sum((i + 1) * (s(-1, h + i) - s(-1, h - 2 - i)) for i in range(h))
    if variant == "i":
        hh, vv = vv, hh
    a = 16 * (g(-1, n - 1) + g(n - 1, -1))
    k = 5 if n == 16 else 34
    b, c = _shift_div(k * hh + 32, 6, variant), _shift_div(k * vv + 32, 6, variant)
    out, raw = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    for y in range(n):
        for x in range(n):
            v = (a + b * (x - (h - 1)) + c * (y - (h - 1)) + 16) >> 5
            raw[y, x] = v
            out[y, x] = (v & 255) if variant == "g" else clip1(v)
    return out, hh, vv, b, c, raw


def pred16(P, x0, y0, mode, variant=None):
    g = _at(P, x0, y0)
    if variant == "f" and mode in (I16_DC_L, I16_DC_T):
        mode = I16_DC
    if mode == I16_V:
        return np.array([[g(x, -1) for x in range(16)]] * 16, dtype=np.int64)
    if mode == I16_H:
        return np.array([[g(-1, y)] * 16 for y in range(16)], dtype=np.int64)
    if mode == I16_P:
        return _plane(g, g, 16, variant)[0]
    if mode == I16_DC_128:
        return np.full((16, 16), 128, dtype=np.int64)
    top, left = sum(g(x, -1) for x in range(16)), sum(g(-1, y) for y in range(16))
    v = (top + left + 16) >> 5 if mode == I16_DC else (left + 8) >> 4 if mode == I16_DC_L else (top + 8) >> 4
    return np.full((16, 16), v, dtype=np.int64)


def chroma_dc_sums(s):
    """t0, t1, l0, l1: the sums over p[0..3, -1], p[4..7, -1], p[-1, 0..3], p[-1, 4..7]"""
    return (sum(s(x, -1) for x in range(4)), sum(s(x, -1) for x in range(4, 8)), sum(s(-1, y) for y in range(4)), sum(s(-1, y) for y in range(4, 8)))


def predc(P, S, x0, y0, mode, variant=None):
    """one 8x8 chroma block; S: the plane the sums (DC, plane H and V) are taken from - P itself but for variant k"""
    g, s = _at(P, x0, y0), _at(S, x0, y0)
    if variant == "f" and mode in (C_DC_L, C_DC_T):
        mode = C_DC
    if mode == C_V:
        return np.array([[g(x, -1) for x in range(8)]] * 8, dtype=np.int64)
    if mode == C_H:
        return np.array([[g(-1, y)] * 8 for y in range(8)], dtype=np.int64)
    if mode == C_P:
        return _plane(g, s, 8, variant)[0]
    out = np.full((8, 8), 128, dtype=np.int64)
    if mode == C_DC_128:
        return out
    t0, t1, l0, l1 = chroma_dc_sums(s)
    if mode == C_DC:          # 8.3.4.1-3 with both sides available
        q = [(t0 + l0 + 4) >> 3, (t1 + 2) >> 2, (l1 + 2) >> 2, (t1 + l1 + 4) >> 3]
        if variant == "j":
            q[1], q[2] = (t1 + l0 + 4) >> 3, (t0 + l1 + 4) >> 3
    elif mode == C_DC_L:      # only the left side
        q = [(l0 + 2) >> 2, (l0 + 2) >> 2, (l1 + 2) >> 2, (l1 + 2) >> 2]
    else:                     # only the top side
        q = [(t0 + 2) >> 2, (t1 + 2) >> 2, (t0 + 2) >> 2, (t1 + 2) >> 2]
    out[:4, :4], out[:4, 4:], out[4:, :4], out[4:, 4:] = q
    return out


def i8_flags(avail):
    """per 8x8 block (z-order) whether its top-left and top-right neighbours are available (6.4.11), from the macroblock's"""
    t, tl, l, tr = (bool(avail & b) for b in (AVAIL_T, AVAIL_TL, AVAIL_L, AVAIL_TR))
    return [tl, t, l, True], [t, tr, True, False]


def _put(P, x0, y0, blk, res, preds=None):
    n = blk.shape[0]
    if preds is not None:
        preds[0][y0 % 16:y0 % 16 + n, x0 % 16:x0 % 16 + n] = blk
    if res is not None:
        blk = np.clip(blk + res[y0 % 16:y0 % 16 + n, x0 % 16:x0 % 16 + n], 0, 255)
    P[y0 + MARGIN:y0 + MARGIN + n, x0 + MARGIN:x0 + MARGIN + n] = blk


def predict_mb(planes, mbx, mby, m, variant=None, residual=None, preds=None):
    """planes: (Y, U, V) of the picture, the samples around the macroblock as they are before the in-loop filter; m: its record.
    residual: None or (16x16, 8x8, 8x8) ints added to the prediction block by block, clipped to 8 bits.
    preds: None or three int arrays (16x16, 8x8, 8x8) that receive the prediction of every sample.  -> (Y 16x16, U, V 8x8)"""
    assert variant is None or variant in VARIANTS
    Y, U, Vp = (_padded(p) for p in planes)
    x0, y0 = 16 * mbx, 16 * mby
    typ = int(m["mb_type"])
    modes = [int(v) for v in m["intra_mode"]]
    ry = None if residual is None else np.asarray(residual[0], dtype=np.int64)
    if typ == I4:
        if variant == "l":
            snaps = []
            for t in range(10):
                snaps.append(Y.copy())
                src = snaps[max(t - 1, 0)]
                for zb in range(16):
                    bx, by = Z_X[zb], Z_Y[zb]
                    if bx + 2 * by == t:
                        _put(Y, x0 + 4 * bx, y0 + 4 * by, pred4(src, x0 + 4 * bx, y0 + 4 * by, modes[4 * by + bx]), ry, preds)
        else:
            for zb in range(16):
                bx, by = Z_X[zb], Z_Y[zb]
                _put(Y, x0 + 4 * bx, y0 + 4 * by, pred4(Y, x0 + 4 * bx, y0 + 4 * by, modes[4 * by + bx], variant), ry, preds)
    elif typ == I8:
        tl, tr = i8_flags(int(m["intra_avail"]))
        for i8 in range(4):
            bx, by = i8 & 1, i8 >> 1
            _put(Y, x0 + 8 * bx, y0 + 8 * by, pred8(Y, x0 + 8 * bx, y0 + 8 * by, modes[8 * by + 2 * bx], tl[i8], tr[i8], variant), ry, preds)
    elif typ == I16:
        _put(Y, x0, y0, pred16(Y, x0, y0, modes[0], variant), ry, preds)
    else:
        raise ValueError("not an intra macroblock the model predicts: type %#x" % typ)
    cm = int(m["chroma_mode"])
    cx, cy = 8 * mbx, 8 * mby
    out = [Y[y0 + MARGIN:y0 + MARGIN + 16, x0 + MARGIN:x0 + MARGIN + 16]]
    for p, (P, S) in enumerate(((U, Vp), (Vp, U))):
        blk = predc(P, S if variant == "k" else P, cx, cy, cm, variant)
        if preds is not None:
            preds[1 + p][:] = blk
        if residual is not None:
            blk = np.clip(blk + np.asarray(residual[1 + p], dtype=np.int64), 0, 255)
        out.append(blk)
    return [np.asarray(o & 255 if variant == "g" else o).astype(np.uint8) for o in out]


def plane_terms(plane, bx0, by0, n):
    """(H, V, b, c, the samples before the clip) of the plane predictor of the n x n block at (bx0, by0) of an unpadded plane"""
    g = _at(_padded(plane), bx0, by0)
    return _plane(g, g, n, None)[1:]
