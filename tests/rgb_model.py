"""The definition of RGB pictures (lh264_decode_batch_ex, include/lh264.h) in numpy, written from the definition and never from the
library: the factors are derived here with fractions.Fraction from Kr and Kb, not read from the header.

The conversion acts on the DELIVERED planes - ow x oh luma, ow/2 x oh/2 Cb and Cr, whatever sizing made them - and converts luma
sample (X, Y) with chroma sample (X >> 1, Y >> 1).  A standard is a matrix (BT.601: Kr = 299/1000, Kb = 114/1000; BT.709:
Kr = 2126/10000, Kb = 722/10000; Kg = 1 - Kr - Kb) and a range (limited: y0 = 16, sy = 255/219, sc = 255/224; full: y0 = 0,
sy = sc = 1).  With D = Cb - 128, E = Cr - 128, as real numbers
    R = sy*(Y - y0) + sc*2(1 - Kr)*E,  B = sy*(Y - y0) + sc*2(1 - Kb)*D,  G = sy*(Y - y0) - sc*(2Kb(1 - Kb)/Kg)*D - sc*(2Kr(1 - Kr)/Kg)*E.
The integer function: every factor is the exact rational times 65536 rounded half up;
    R = clip8 ((cy*(Y - y0) + crv*E + 32768) >> 16), G = clip8 ((cy*(Y - y0) - cgu*D - cgv*E + 32768) >> 16),
    B = clip8 ((cy*(Y - y0) + cbu*D + 32768) >> 16), `>>` an arithmetic shift.
Layouts: "rgb24" = oh rows of ow pixels stored R, G, B; "rgbp" = three ow x oh planes R, G, B; pictures tight one behind the other."""
import math
from fractions import Fraction as F

import numpy as np

import scale_ref

KR_KB = {"bt601": (F(299, 1000), F(114, 1000)), "bt709": (F(2126, 10000), F(722, 10000))}
# a standard in one byte, as the job tables carry it: bit 0 the matrix (0 BT.601, 1 BT.709), bit 1 the range (0 limited, 1 full)
STANDARDS = [("bt601", "limited"), ("bt709", "limited"), ("bt601", "full"), ("bt709", "full")]
LAYOUTS = {"rgb24": 1, "rgbp": 2}


def real_factors(matrix, rng):
    """-> (y0, [cy, crv, cbu, cgu, cgv]) as exact rationals"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    y0, sy, sc = (16, F(255, 219), F(255, 224)) if rng == "limited" else (0, F(1), F(1))
    return y0, [sy, sc * 2 * (1 - kr), sc * 2 * (1 - kb), sc * 2 * kb * (1 - kb) / kg, sc * 2 * kr * (1 - kr) / kg]


def factors(matrix, rng):
    """-> (y0, the five factors times 65536, rounded half up)"""
    y0, f = real_factors(matrix, rng)
    return y0, [math.floor(x * 65536 + F(1, 2)) for x in f]


def convert(Y, Cb, Cr, matrix, rng):
    """the integer function on arrays of equal shape -> (R, G, B) uint8"""
    y0, (cy, crv, cbu, cgu, cgv) = factors(matrix, rng)
    Y, D, E = np.asarray(Y).astype(np.int64) - y0, np.asarray(Cb).astype(np.int64) - 128, np.asarray(Cr).astype(np.int64) - 128
    sums = (cy * Y + crv * E + 32768, cy * Y - cgu * D - cgv * E + 32768, cy * Y + cbu * D + 32768)
    assert all(np.abs(s).max(initial=0) < 1 << 27 for s in sums)
    return tuple(np.clip(s >> 16, 0, 255).astype(np.uint8) for s in sums)


def convert_real(Y, Cb, Cr, matrix, rng):
    """the real-valued formula, rounded half up and clipped, in exact integers: every term over one common denominator"""
    y0, f = real_factors(matrix, rng)
    den = 1
    for x in f:
        den = den * x.denominator // math.gcd(den, x.denominator)
    cy, crv, cbu, cgu, cgv = [int(x * den) for x in f]
    assert all(F(n, den) == x for n, x in zip((cy, crv, cbu, cgu, cgv), f)) and 2 * 3 * 256 * max(cy, crv, cbu, cgu, cgv) + den < 1 << 62
    Y, D, E = np.asarray(Y).astype(np.int64) - y0, np.asarray(Cb).astype(np.int64) - 128, np.asarray(Cr).astype(np.int64) - 128
    out = []
    for num in (cy * Y + crv * E, cy * Y - cgu * D - cgv * E, cy * Y + cbu * D):
        out.append(np.clip((2 * num + den) // (2 * den), 0, 255).astype(np.uint8))      # floor (x + 1/2)
    return tuple(out)


def rgb_from_planes(y, u, v, layout, matrix, rng):
    """delivered planes (y: oh x ow, u and v: oh/2 x ow/2) -> the picture's RGB bytes (a flat uint8 array)"""
    oh, ow = y.shape
    assert ow % 2 == 0 and oh % 2 == 0 and u.shape == (oh // 2, ow // 2) and v.shape == u.shape
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)      # chroma sample (X >> 1, Y >> 1)
    r, g, b = convert(y, up(u), up(v), matrix, rng)
    if layout in ("rgb24", 1):
        return np.stack([r, g, b], axis=-1).reshape(-1)
    assert layout in ("rgbp", 2)
    return np.concatenate([r.reshape(-1), g.reshape(-1), b.reshape(-1)])


def rgb_packed(data, pictures, layout, standards):
    """the I420 bytes one stream delivers without colour and its picture records [(width, height, frame_num, idr, offset, bytes)] ->
    the bytes and records the call delivers with colour; standards: one (matrix, range) for all pictures, or one per picture"""
    if isinstance(standards, tuple):
        standards = [standards] * len(pictures)
    out, recs, off = [], [], 0
    for (w, h, frame_num, idr, at, n), (matrix, rng) in zip(pictures, standards):
        assert n == w * h * 3 // 2
        b = rgb_from_planes(*scale_ref.unpack(data[at:at + n], w, h, scale_ref.FMT_I420), layout, matrix, rng).tobytes()
        assert len(b) == 3 * w * h
        recs.append((w, h, frame_num, idr, off, len(b)))
        out.append(b)
        off += len(b)
    return b"".join(out), recs
