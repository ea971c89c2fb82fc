"""The definition of reduced-size pictures (lh264_decode_batch, scale_log2 = s in {1, 2, 3}) in numpy, written from the definition
and never from the library:

B = 1 << s.  For a picture whose cropped window is w x h (both even), cw = w / 2 and ch = h / 2.  Delivered chroma size:
ocw = ceil (cw / B), och = ceil (ch / B); delivered luma size: ow = 2 * ocw, oh = 2 * och.  Delivered luma sample (X, Y) =
(sum + (1 << (2*s - 1))) >> (2*s), sum over the B x B window samples at x = min (X*B + i, w - 1), y = min (Y*B + j, h - 1),
0 <= i, j < B.  Cb and Cr: the same rule on their cw x ch planes.  Planes are averaged independently.  Packing as at scale 0 with
ow, oh in place of w, h: I420 = Y, Cb, Cr; NV12 = Y, then Cb / Cr interleaved; pictures tight one behind the other."""
import numpy as np

FMT_I420, FMT_NV12 = 0, 1


def scaled_size(w, h, s):
    """delivered luma (ow, oh) of a w x h window"""
    if s == 0:
        return w, h
    B = 1 << s
    return 2 * -(-(w // 2) // B), 2 * -(-(h // 2) // B)


def _scale_plane(p, pw, ph, s):
    """p: the window's samples (2-D uint8) -> pw x ph means, coordinates clamped to the window"""
    B = 1 << s
    h, w = p.shape
    ys = np.minimum(np.arange(ph * B), h - 1)
    xs = np.minimum(np.arange(pw * B), w - 1)
    big = p[np.ix_(ys, xs)].astype(np.uint32)
    sums = big.reshape(ph, B, pw, B).sum(axis=(1, 3))
    return ((sums + (1 << (2 * s - 1))) >> (2 * s)).astype(np.uint8)


def scale_planes(y, u, v, s):
    """the window's planes (y: h x w, u and v: h/2 x w/2) -> the delivered planes"""
    if s == 0:
        return y.copy(), u.copy(), v.copy()
    h, w = y.shape
    assert w % 2 == 0 and h % 2 == 0 and u.shape == (h // 2, w // 2) and v.shape == u.shape and s in (1, 2, 3)
    ow, oh = scaled_size(w, h, s)
    return _scale_plane(y, ow, oh, s), _scale_plane(u, ow // 2, oh // 2, s), _scale_plane(v, ow // 2, oh // 2, s)


def unpack(data, w, h, fmt):
    """one packed picture -> (y, u, v)"""
    a = np.frombuffer(data, dtype=np.uint8)
    assert a.size == w * h * 3 // 2
    y = a[:w * h].reshape(h, w)
    c = a[w * h:]
    if fmt == FMT_I420:
        return y, c[:c.size // 2].reshape(h // 2, w // 2), c[c.size // 2:].reshape(h // 2, w // 2)
    c = c.reshape(h // 2, w // 2, 2)
    return y, c[:, :, 0], c[:, :, 1]


def pack(y, u, v, fmt):
    if fmt == FMT_I420:
        return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).tobytes()
    return np.concatenate([y.reshape(-1), np.stack([u, v], axis=-1).reshape(-1)]).tobytes()


def scale_packed(data, pictures, fmt, s):
    """scale-0 delivered bytes of one stream and its picture records [(width, height, frame_num, idr, offset, bytes)] -> the bytes
    and records the call delivers at scale s.  fmt: 0 / "i420" or 1 / "nv12" """
    fmt = {"i420": FMT_I420, "nv12": FMT_NV12}.get(fmt, fmt)
    out, recs, off = [], [], 0
    for (w, h, frame_num, idr, at, n) in pictures:
        assert n == w * h * 3 // 2
        y, u, v = scale_planes(*unpack(data[at:at + n], w, h, fmt), s)
        b = pack(y, u, v, fmt)
        recs.append((y.shape[1], y.shape[0], frame_num, idr, off, len(b)))
        out.append(b)
        off += len(b)
    return b"".join(out), recs
