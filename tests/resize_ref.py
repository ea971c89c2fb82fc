"""The definition of pictures of one given size (lh264_decode_batch, out_width x out_height) in numpy with explicit weight matrices,
written from the definition and never from the library:

The target is OW x OH, both even, 2..4096.  Each plane is resampled on its own: luma from the w x h cropped window to OW x OH, Cb and
Cr from w/2 x h/2 to OW/2 x OH/2.  For one plane of w x h samples p[y][x] delivered as ow x oh: the weight of source column x for
delivered column X is wx (X, x) = max (0, min ((x+1)*ow, (X+1)*w) - max (x*ow, X*w)); wy (Y, y) is the same with h and oh;
S = sum over y, x of wy (Y, y) * wx (X, x) * p[y][x], D = w*h, delivered sample = floor ((2*S + D) / (2*D)).  Packing as ever with
OW, OH in place of w, h: I420 = Y, Cb, Cr; NV12 = Y, then Cb / Cr interleaved; pictures tight one behind the other."""
import functools

import numpy as np

import scale_ref

FMT_I420, FMT_NV12 = scale_ref.FMT_I420, scale_ref.FMT_NV12


@functools.lru_cache(maxsize=None)
def weights(n, on):
    """the on x n matrix of weights of n source samples for on delivered samples (int64); every row sums to n, every column to on"""
    X = np.arange(on, dtype=np.int64)[:, None]
    x = np.arange(n, dtype=np.int64)[None, :]
    m = np.maximum(0, np.minimum((x + 1) * on, (X + 1) * n) - np.maximum(x * on, X * n))
    assert np.all(m.sum(axis=1) == n) and np.all(m.sum(axis=0) == on)
    # non-zero exactly in floor (X*n / on) .. floor (((X+1)*n - 1) / on), and `on` strictly inside that span
    lo, hi = (X * n) // on, ((X + 1) * n - 1) // on
    assert np.array_equal(m > 0, (x >= lo) & (x <= hi)) and np.all(m[(x > lo) & (x < hi)] == on)
    return m


def resize_plane(p, ow, oh):
    """p: the window's samples (2-D uint8) -> oh x ow exact area means, round half up"""
    h, w = p.shape
    # integers of at most 255 * w * h < 2^53 throughout: the float64 products and sums are exact (and the matrix product is BLAS's)
    S = (weights(h, oh).astype(np.float64) @ p.astype(np.float64) @ weights(w, ow).T.astype(np.float64)).astype(np.int64)
    D = w * h
    assert 255 * D < 1 << 53 and S.max() <= 255 * D
    return ((2 * S + D) // (2 * D)).astype(np.uint8)


def resize_planes(y, u, v, size):
    """the window's planes (y: h x w, u and v: h/2 x w/2) -> the delivered planes of a W x H picture"""
    W, H = size
    h, w = y.shape
    assert w % 2 == 0 and h % 2 == 0 and u.shape == (h // 2, w // 2) and v.shape == u.shape
    assert W % 2 == 0 and H % 2 == 0 and 2 <= W <= 4096 and 2 <= H <= 4096
    return resize_plane(y, W, H), resize_plane(u, W // 2, H // 2), resize_plane(v, W // 2, H // 2)


def resize_packed(data, pictures, fmt, size):
    """the delivered bytes of one stream without a size and its picture records [(width, height, frame_num, idr, offset, bytes)] ->
    the bytes and records the call delivers with size = (W, H).  fmt: 0 / "i420" or 1 / "nv12" """
    fmt = {"i420": FMT_I420, "nv12": FMT_NV12}.get(fmt, fmt)
    W, H = size
    out, recs, off, memo = [], [], 0, {}
    for (w, h, frame_num, idr, at, n) in pictures:
        assert n == w * h * 3 // 2
        src = data[at:at + n]
        key = (w, h, src)
        if key not in memo:                 # (a stream that repeats a picture: computed once)
            memo[key] = scale_ref.pack(*resize_planes(*scale_ref.unpack(src, w, h, fmt), (W, H)), fmt)
        b = memo[key]
        assert len(b) == W * H * 3 // 2
        recs.append((W, H, frame_num, idr, off, len(b)))
        out.append(b)
        off += len(b)
    return b"".join(out), recs
