"""Synthetic padded pictures for the reduced-size pack step (tests/test_decode_scale.py on the host, test_decode_scale_gpu.py on the
device): seeded random (or fixed) samples inside the window, everywhere else in the padded picture - and in a margin around it - the
complement of the nearest window sample, so that any read outside the window moves a mean."""
import numpy as np

import scale_ref

# (w, h, crop_x, crop_y)
WINDOWS = [(2, 2, 0, 0), (4, 2, 0, 0), (2, 4, 0, 0), (6, 10, 0, 0), (14, 6, 0, 0), (16, 16, 0, 0), (18, 14, 0, 0), (30, 34, 0, 0), (34, 18, 0, 0),
           (66, 50, 0, 0), (176, 144, 0, 0), (300, 168, 26, 60), (62, 46, 6, 2)]
GUARD = 64
MARGIN = 16          # luma samples around the padded picture that belong to the buffer (chroma: half)


def _plane(win, x0, y0, pw, ph, m):
    """win at (x0, y0) of a pw x ph plane with a margin of m samples: the window's samples, the complement of the nearest one elsewhere"""
    h, w = win.shape
    ys = np.clip(np.arange(-m, ph + m) - y0, 0, h - 1)
    xs = np.clip(np.arange(-m, pw + m) - x0, 0, w - 1)
    full = (255 - win[np.ix_(ys, xs)]).astype(np.uint8)
    full[m + y0:m + y0 + h, m + x0:m + x0 + w] = win
    return full


class Case:
    """one padded picture in one flat buffer: .buf, the offsets of the planes' pixel (0, 0), the strides, the window and its samples"""

    def __init__(self, w, h, crop_x, crop_y, seed=0, content="random", pic_w=None, pic_h=None):
        assert not (w | h | crop_x | crop_y) & 1
        self.crop = (crop_x, crop_y, w, h)
        pic_w = pic_w or ((crop_x + w + 15) & ~15) + 16
        pic_h = pic_h or ((crop_y + h + 15) & ~15) + 16
        assert pic_w >= crop_x + w and pic_h >= crop_y + h
        rng = np.random.default_rng(seed)

        def samples(hh, ww):
            if content == "random":
                return rng.integers(0, 256, (hh, ww), dtype=np.uint8)
            if content == "checker":
                return (((np.arange(hh)[:, None] + np.arange(ww)[None, :]) & 1) * 255).astype(np.uint8)
            return np.full((hh, ww), int(content), dtype=np.uint8)
        self.Y, self.U, self.V = samples(h, w), samples(h // 2, w // 2), samples(h // 2, w // 2)
        m = MARGIN
        planes = [_plane(self.Y, crop_x, crop_y, pic_w, pic_h, m), _plane(self.U, crop_x // 2, crop_y // 2, pic_w // 2, pic_h // 2, m // 2),
                  _plane(self.V, crop_x // 2, crop_y // 2, pic_w // 2, pic_h // 2, m // 2)]
        self.stride_y, self.stride_c = planes[0].shape[1], planes[1].shape[1]
        at, self.off = 0, []
        for p, mm in zip(planes, (m, m // 2, m // 2)):
            self.off.append(at + mm * p.shape[1] + mm)
            at += p.size
        self.buf = np.concatenate([p.reshape(-1) for p in planes])
        self._expect = {}

    def expect(self, s, fmt):
        """the packed picture the definition gives (computed once)"""
        if (s, fmt) not in self._expect:
            self._expect[(s, fmt)] = np.frombuffer(scale_ref.pack(*scale_ref.scale_planes(self.Y, self.U, self.V, s), fmt), dtype=np.uint8)
        return self._expect[(s, fmt)]

    def fill_job(self, j, src_ptr, dst_ptr, fmt, s):
        """j: a _lib.PackJob; src_ptr: where .buf lies (host or device); dst_ptr: the packed picture's first byte"""
        j.y, j.u, j.v = src_ptr + self.off[0], src_ptr + self.off[1], src_ptr + self.off[2]
        j.dst = dst_ptr
        j.stride_y, j.stride_c = self.stride_y, self.stride_c
        j.crop_x, j.crop_y, j.crop_w, j.crop_h = self.crop
        j.format, j.reserved = fmt, s
