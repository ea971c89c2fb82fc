"""The definition of float RGB pictures (lh264_decode_batch_ex2, include/lh264.h) written from the definition and never from the
library: element e of a picture is a function of byte e of the same picture delivered as uint8,

    v32 = fma (float32 (c), mul[ch], add[ch])      one binary32 fused multiply-add, round to nearest even
    float32: v32     float16: v32 rounded to binary16, nearest even     bfloat16: v32 rounded to bfloat16, nearest even

with c the byte and ch its channel (0 R, 1 G, 2 B).  A (type, mul, add) is a table of 3 x 256 bit patterns.  The fused multiply-add
is computed exactly in fractions.Fraction and rounded once, by choosing between the two neighbouring binary32 values with ties to
the even mantissa - never through a float64 sum, which would round twice; the sign of an exact zero follows IEEE 754 (6.3).  binary16
comes from numpy's astype, bfloat16 from integer arithmetic on the binary32 bits."""
import math
from fractions import Fraction as F

import numpy as np

TYPES = {"float32": 1, "float16": 2, "bfloat16": 3}      # LH264_SAMPLE_*
ELEMENT_BYTES = {"float32": 4, "float16": 2, "bfloat16": 2}
SUFFIX = {"float32": ".f32", "float16": ".f16", "bfloat16": ".bf16"}


def f32(x):
    """a number as the binary32 value nearest to it (numpy's rounding of a float64; every constant of the tests is exact in float64)"""
    return np.float32(x)


def bits_of(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def round_to_binary32(x, zero_sign=0):
    """an exact rational -> the bits of the nearest binary32, ties to the even mantissa, gradual underflow, overflow to infinity;
    x == 0 gives a zero of sign zero_sign"""
    if x == 0:
        return 0x80000000 if zero_sign else 0
    sign, a = (0x80000000 if x < 0 else 0), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^(e-1) < a < 2^(e+1)
    if F(2) ** e > a:
        e -= 1
    assert F(2) ** e <= a < F(2) ** (e + 1)
    k = max(e, -126) - 23                                          # the unit of the last place: 2^k
    n = a / F(2) ** k
    q, rem = n.numerator // n.denominator, n - n.numerator // n.denominator
    if rem > F(1, 2) or (rem == F(1, 2) and (q & 1)):
        q += 1
    if q * F(2) ** k >= F(2) ** 128:
        return sign | 0x7f800000
    return sign | bits_of(math.ldexp(q, k))                        # q < 2^25: exact in float64, and a binary32 value by construction


def fma_bits(c, m, a):
    """fma (float32 (c), m, a) for an integer c >= 0 and binary32 m, a (finite) -> the bits of the binary32 result"""
    m, a = np.float32(m), np.float32(a)
    assert np.isfinite(m) and np.isfinite(a) and c >= 0
    exact = F(int(c)) * F(float(m)) + F(float(a))
    if exact != 0:
        return round_to_binary32(exact)
    # an exact zero: the sum of two zeros of one sign keeps it; every other exact zero is +0 under round to nearest
    product_zero = c == 0 or float(m) == 0.0
    product_sign = bool(np.signbit(m))                              # float32 (c) is +c
    if product_zero and float(a) == 0.0 and product_sign == bool(np.signbit(a)):
        return round_to_binary32(F(0), product_sign)
    return 0


def to_half_bits(bits32):
    """binary32 bit patterns (uint32 array) -> binary16 bit patterns, by numpy's conversion"""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(bits32, dtype=np.uint32).view(np.float32).astype(np.float16).view(np.uint16)


def to_bfloat_bits(bits32):
    """binary32 bit patterns of finite values or infinities -> bfloat16 bit patterns, nearest even in integer arithmetic"""
    b = np.asarray(bits32, dtype=np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


_tables = {}


def table32(mul, add):
    """the 3 x 256 binary32 bit patterns of fma (c, mul[ch], add[ch])"""
    key = tuple(bits_of(x) for x in list(mul) + list(add))
    if key not in _tables:
        _tables[key] = np.array([[fma_bits(c, mul[ch], add[ch]) for c in range(256)] for ch in range(3)], dtype=np.uint32)
    return _tables[key]


def table(type_name, mul, add):
    """the 3 x 256 table of a type: uint32 bit patterns for float32, uint16 for the 16-bit types"""
    t = table32(mul, add)
    return t if type_name == "float32" else to_half_bits(t) if type_name == "float16" else to_bfloat_bits(t)


def apply_picture(rgb, layout, tab):
    """one picture's uint8 RGB bytes (flat) in layout "rgb24" | "rgbp" -> its float picture's bytes (flat uint8, little-endian)"""
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1)
    assert rgb.size % 3 == 0
    ch = np.arange(rgb.size) % 3 if layout in ("rgb24", 1) else np.arange(rgb.size) // (rgb.size // 3)
    return tab[ch, rgb].astype("<u4" if tab.dtype == np.uint32 else "<u2").view(np.uint8)


def apply(data, records, layout, type_name, mul, add):
    """the bytes a stream delivers with dtype uint8 and their records [(width, height, frame_num, idr, offset, bytes)] -> the bytes
    and records the same call delivers with a float type"""
    tab, es = table(type_name, mul, add), ELEMENT_BYTES[type_name]
    out, recs, off = [], [], 0
    for (w, h, frame_num, idr, at, n) in records:
        assert n == 3 * w * h
        b = apply_picture(np.frombuffer(data, dtype=np.uint8, count=n, offset=at), layout, tab).tobytes()
        assert len(b) == n * es
        recs.append((w, h, frame_num, idr, off, len(b)))
        out.append(b)
        off += len(b)
    return b"".join(out), recs
