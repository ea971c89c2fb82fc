"""The definition of the bilinear and bicubic filters of a sized decode (lh264_decode_batch_ex6) in Python integers and numpy int64,
written from the definition in include/lh264.h and never from the library.

One plane of w x h window samples p[y][x] is delivered as ow x oh, each axis on its own, `//` floor:
  m = 2 * max (w, ow);  n (x) = |2*ow*x + ow - (2*X + 1)*w|  for x in 0 .. w - 1 only
  bilinear: r = m - n where n < m, else 0
  bicubic:  n < m: r = 3n^3 - 5n^2 m + 2m^3;  m <= n < 2m: r = -n^3 + 5n^2 m - 8n m^2 + 4m^3;  else 0
  R = sum r;  k = (2^15 * r + R) // (2R);  e = 2^14 - sum k goes to the tap with the largest r, the lowest x among equals
  H (y, X) = sum_x kx (X, x) * p[y][x];  S = sum_y ky (Y, y) * H (y, X);  sample = clip (0, 255, (S + 2^27) >> 28)
A row of weights as the library hands it out begins at the lowest x whose k is not 0 and ends at the highest.
Rectangles are tests/view_model.py's, colour tests/rgb_model.py's, the float types tests/sample_model.py's, each on the planes this
module delivers."""
import functools

import numpy as np

import rgb_model
import sample_model
import scale_ref
import view_model as VM

FILTERS = {"bilinear": 1, "bicubic": 2}


def raw(name, n, m):
    if name == "bilinear":
        return m - n if n < m else 0
    if n < m:
        return 3 * n ** 3 - 5 * n ** 2 * m + 2 * m ** 3
    if n < 2 * m:
        return -n ** 3 + 5 * n ** 2 * m - 8 * n * m ** 2 + 4 * m ** 3
    return 0


@functools.lru_cache(maxsize=None)
def rows(name, w, ow):
    """[(first, [k, ...])] per delivered coordinate: the normalised weights of an axis of w samples delivered as ow"""
    assert name in FILTERS and w >= 1 and ow >= 1
    m = 2 * max(w, ow)
    reach = (2 * m) // (2 * ow) + 2          # no x further than this from the centre has n < 2m
    out = []
    for X in range(ow):
        centre = ((2 * X + 1) * w - ow) // (2 * ow)
        lo, hi = max(0, centre - reach), min(w - 1, centre + reach + 1)
        r = [raw(name, abs(2 * ow * x + ow - (2 * X + 1) * w), m) for x in range(lo, hi + 1)]
        assert (lo == 0 or r[0] == 0) and (hi == w - 1 or r[-1] == 0)
        R = sum(r)
        assert R > 0
        k = [(2 ** 15 * v + R) // (2 * R) for v in r]          # Python's // floors toward minus infinity
        k[r.index(max(r))] += 2 ** 14 - sum(k)
        a = min(i for i, v in enumerate(k) if v)
        b = max(i for i, v in enumerate(k) if v)
        out.append((lo + a, k[a:b + 1]))
    return out


@functools.lru_cache(maxsize=None)
def matrix(name, w, ow):
    """the ow x w matrix of normalised weights (int64)"""
    K = np.zeros((ow, w), dtype=np.int64)
    for X, (first, k) in enumerate(rows(name, w, ow)):
        K[X, first:first + len(k)] = k
    return K


def unclipped(p, ow, oh, name):
    """(S + 2^27) >> 28 of every delivered sample of plane p (2-D uint8) as int64, before the clip"""
    h, w = p.shape
    H = p.astype(np.int64) @ matrix(name, w, ow).T
    assert np.abs(H).max(initial=0) < 2 ** 31
    S = matrix(name, h, oh) @ H
    return (S + (1 << 27)) >> 28


def resample_plane(p, ow, oh, name):
    return np.clip(unclipped(p, ow, oh, name), 0, 255).astype(np.uint8)


def filter_planes(y, u, v, size, name):
    """the window's planes (y: h x w, u and v: h/2 x w/2) -> the delivered planes of a W x H picture"""
    W, H = size
    h, w = y.shape
    assert w % 2 == 0 and h % 2 == 0 and u.shape == (h // 2, w // 2) and v.shape == u.shape and W % 2 == 0 and H % 2 == 0
    return resample_plane(y, W, H, name), resample_plane(u, W // 2, H // 2, name), resample_plane(v, W // 2, H // 2, name)


def placed_planes(y, u, v, place, fill, size, name):
    """the window's planes resampled to place = (x, y, w, h) of a size = (OW, OH) picture, every other sample the fill (y, cb, cr)"""
    OW, OH = size
    dx, dy, dw, dh = place
    assert not (dx | dy | dw | dh) & 1 and dw >= 2 and dh >= 2 and dx >= 0 and dy >= 0 and dx + dw <= OW and dy + dh <= OH
    out = []
    for p, f, s in zip(filter_planes(y, u, v, (dw, dh), name), fill, (1, 2, 2)):
        full = np.full((OH // s, OW // s), f, dtype=np.uint8)
        full[dy // s:(dy + dh) // s, dx // s:(dx + dw) // s] = p
        out.append(full)
    return tuple(out)


def view_planes(y, u, v, size, name, crop=None, fit="stretch", fill=VM.DEFAULT_FILL):
    """the window's planes -> the planes the call delivers under the view with the filter"""
    h, w = y.shape
    (sx, sy, sw, sh), dst = VM.rects(w, h, crop, fit, size)
    ys = y[sy:sy + sh, sx:sx + sw]
    us, vs = (c[sy // 2:(sy + sh) // 2, sx // 2:(sx + sw) // 2] for c in (u, v))
    return placed_planes(ys, us, vs, dst, fill, size, name)


def view_packed(data, pictures, fmt, size, name, crop=None, fit="stretch", fill=VM.DEFAULT_FILL):
    """the delivered bytes of one stream without a size and its picture records [(width, height, frame_num, idr, offset, bytes)] ->
    (bytes, records): what the call delivers with size, filter and view (every picture's window takes the crop)"""
    fmt = {"i420": scale_ref.FMT_I420, "nv12": scale_ref.FMT_NV12}.get(fmt, fmt)
    out, recs, off, memo = [], [], 0, {}
    for (w, h, frame_num, idr, at, n) in pictures:
        assert n == w * h * 3 // 2
        src = data[at:at + n]
        key = (w, h, src)
        if key not in memo:
            memo[key] = scale_ref.pack(*view_planes(*scale_ref.unpack(src, w, h, fmt), size, name, crop=crop, fit=fit, fill=fill), fmt)
        b = memo[key]
        assert len(b) == size[0] * size[1] * 3 // 2
        recs.append((size[0], size[1], frame_num, idr, off, len(b)))
        out.append(b)
        off += len(b)
    return b"".join(out), recs


def rgb_of(planes, layout, std):
    """RGB bytes (flat uint8) of delivered planes under standard byte std: tests/rgb_model.py unchanged"""
    return rgb_model.rgb_from_planes(*planes, layout, *rgb_model.STANDARDS[std])


def float_of(rgb, layout, type_name, mul, add):
    """... and their float picture's bytes: tests/sample_model.py unchanged"""
    return sample_model.apply_picture(rgb, layout, sample_model.table(type_name, mul, add))
