"""The definition of fitted views (lh264_decode_batch_ex3: a caller's crop, cover and letterbox) in Python integers and numpy, written
from the definition and never from the library.

A view is applied per delivered picture, before any sizing.  w x h is the picture's cropped window (even).  A caller's crop
{x, y, w, h} in window coordinates (all even, inside the window) takes the window's place in every definition.  With a size OW x OH and
w, h the window after the crop, `//` floor:
  cover:   w*OH > h*OW: sh = h, sw = max (2, 2 * ((h*OW + OH) // (2*OH)));  w*OH < h*OW: sw = w, sh = max (2, 2 * ((w*OH + OW) // (2*OW)));
           equality: the whole window.  sx = 2 * ((w - sw) // 4), sy = 2 * ((h - sh) // 4).  {sx, sy, sw, sh} is resampled to OW x OH.
  contain: w*OH > h*OW: dw = OW, dh = max (2, 2 * ((h*OW + w) // (2*w)));  w*OH < h*OW: dh = OH, dw = max (2, 2 * ((w*OH + h) // (2*h)));
           equality: the whole output.  dx = 2 * ((OW - dw) // 4), dy = 2 * ((OH - dh) // 4).  The window is resampled to dw x dh and
           lies at (dx, dy); every other luma sample is fill_y, Cb and Cr with every quantity halved and fill_cb, fill_cr.
The resampling is tests/resize_ref.py's, the scale_log2 means tests/scale_ref.py's, RGB tests/rgb_model.py's and the float types
tests/sample_model.py's, each on the planes this module delivers."""
import numpy as np

import resize_ref
import rgb_model
import sample_model
import scale_ref

FIT = {"stretch": 0, "cover": 1, "contain": 2}
DEFAULT_FILL = (16, 128, 128)


def crop_fits(crop, w, h):
    x, y, cw, ch = crop
    return x >= 0 and y >= 0 and cw >= 2 and ch >= 2 and not (x | y | cw | ch) & 1 and x + cw <= w and y + ch <= h


def rects(w, h, crop, fit, size):
    """-> (src, dst), each (x, y, w, h): the source rectangle in window coordinates, the destination rectangle in the delivered picture
    (without a size: the source's own size at (0, 0))"""
    assert fit in FIT and (size is not None or fit == "stretch")
    cx, cy, cw, ch = crop if crop is not None else (0, 0, w, h)
    assert crop_fits((cx, cy, cw, ch), w, h)
    if size is None:
        return (cx, cy, cw, ch), (0, 0, cw, ch)
    OW, OH = size
    sx, sy, sw, sh = 0, 0, cw, ch
    dx, dy, dw, dh = 0, 0, OW, OH
    if fit == "cover" and cw * OH != ch * OW:
        if cw * OH > ch * OW:
            sw = max(2, 2 * ((ch * OW + OH) // (2 * OH)))
        else:
            sh = max(2, 2 * ((cw * OH + OW) // (2 * OW)))
        sx, sy = 2 * ((cw - sw) // 4), 2 * ((ch - sh) // 4)
    if fit == "contain" and cw * OH != ch * OW:
        if cw * OH > ch * OW:
            dh = max(2, 2 * ((ch * OW + cw) // (2 * cw)))
        else:
            dw = max(2, 2 * ((cw * OH + ch) // (2 * ch)))
        dx, dy = 2 * ((OW - dw) // 4), 2 * ((OH - dh) // 4)
    return (cx + sx, cy + sy, sw, sh), (dx, dy, dw, dh)


def placed_planes(y, u, v, place, fill, size):
    """the window's planes resampled to place = (x, y, w, h) of a size = (OW, OH) picture, every other sample the fill (y, cb, cr)"""
    OW, OH = size
    dx, dy, dw, dh = place
    assert not (dx | dy | dw | dh) & 1 and dw >= 2 and dh >= 2 and dx >= 0 and dy >= 0 and dx + dw <= OW and dy + dh <= OH
    ry, ru, rv = resize_ref.resize_planes(y, u, v, (dw, dh))
    out = []
    for p, f, s in ((ry, fill[0], 1), (ru, fill[1], 2), (rv, fill[2], 2)):
        full = np.full((OH // s, OW // s), f, dtype=np.uint8)
        full[dy // s:(dy + dh) // s, dx // s:(dx + dw) // s] = p
        out.append(full)
    return tuple(out)


def view_planes(y, u, v, crop=None, fit="stretch", fill=DEFAULT_FILL, size=None, scale=0):
    """the window's planes (y: h x w, u and v: h/2 x w/2) -> the planes the call delivers under the view"""
    h, w = y.shape
    (sx, sy, sw, sh), dst = rects(w, h, crop, fit, size)
    ys = y[sy:sy + sh, sx:sx + sw]
    us, vs = (c[sy // 2:(sy + sh) // 2, sx // 2:(sx + sw) // 2] for c in (u, v))
    if size is None:
        return scale_ref.scale_planes(ys, us, vs, scale) if scale else (ys, us, vs)
    assert scale == 0
    return placed_planes(ys, us, vs, dst, fill, size)


def view_packed(data, pictures, fmt, crop=None, fit="stretch", fill=DEFAULT_FILL, size=None, scale=0):
    """the delivered bytes of one stream without a view and without a size and its picture records [(width, height, frame_num, idr,
    offset, bytes)] -> (bytes, records, views, stop): what the call delivers under the view - the pictures in front of the first one
    the crop does not fit - the (src, dst) of each, and the number of the picture that stops the stream (None: none does)"""
    fmt = {"i420": scale_ref.FMT_I420, "nv12": scale_ref.FMT_NV12}.get(fmt, fmt)
    out, recs, views, off, memo = [], [], [], 0, {}
    for k, (w, h, frame_num, idr, at, n) in enumerate(pictures):
        assert n == w * h * 3 // 2
        if crop is not None and not crop_fits(crop, w, h):
            return b"".join(out), recs, views, k
        src = data[at:at + n]
        key = (w, h, src)
        if key not in memo:
            p = view_planes(*scale_ref.unpack(src, w, h, fmt), crop=crop, fit=fit, fill=fill, size=size, scale=scale)
            memo[key] = (scale_ref.pack(*p, fmt), p[0].shape[1], p[0].shape[0])
        b, ow, oh = memo[key]
        assert len(b) == ow * oh * 3 // 2
        recs.append((ow, oh, frame_num, idr, off, len(b)))
        src_rect, dst_rect = rects(w, h, crop, fit, size)
        views.append((src_rect, dst_rect if size is not None else (0, 0, ow, oh)))      # (without a size: what is delivered, at its scale)
        out.append(b)
        off += len(b)
    return b"".join(out), recs, views, None


def rgb_of(planes, layout, matrix, rng):
    """RGB bytes (flat uint8) of delivered planes: tests/rgb_model.py unchanged, bars included"""
    return rgb_model.rgb_from_planes(*planes, layout, matrix, rng)


def float_of(rgb, layout, type_name, mul, add):
    """... and their float picture's bytes: tests/sample_model.py unchanged"""
    return sample_model.apply_picture(rgb, layout, sample_model.table(type_name, mul, add))
