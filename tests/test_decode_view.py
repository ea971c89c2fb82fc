"""Fitted views (lh264_decode_batch_ex3: a caller's crop, cover, letterbox) where no device is present: the rule of the rectangles
against tests/view_model.py; the code of the three placed kernels stepped on the host (lh264_debug_view_cpu) over synthetic padded
pictures against the model, in 0xA5 guard bytes; the layout of the view struct and the arguments of the call and of the entry points."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rgb_model
import sample_model as SM
import scale_cases as SC
import scale_ref
import view_model as VM
from test_decode_resize import WINDOWS as RESIZE_WINDOWS
from test_decode_sample import IMAGENET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")

# (w, h, crop_x, crop_y) of tests/test_decode_resize.py
WINDOWS = [w for w in RESIZE_WINDOWS if w[:2] in ((2, 2), (6, 10), (18, 14), (62, 46), (176, 144), (300, 168))]
CONTENTS = ["random", 0, 255, "checker"]
OUTPUTS = [(2, 2), (4, 2), (10, 6), (22, 18), (46, 38), (224, 224), (4096, 2)]
FILLS = [(0, 0, 0), (255, 255, 255), (16, 128, 128), (81, 90, 240)]
TYPES = ["float32", "float16", "bfloat16"]
LAYOUTS = ["rgb24", "rgbp"]
assert len(WINDOWS) == 6 and (62, 46, 6, 2) in WINDOWS and (300, 168, 26, 60) in WINDOWS


def _lib():
    import __graft_entry__ as g
    g.build()
    from losslessh264_amd import _lib as L
    return L, L.lib()


def fill_word(f):
    return f[0] | f[1] << 8 | f[2] << 16


# ---- the rectangles ---------------------------------------------------------------------------------------------------------------------
def _some_crop(w, h):
    """a crop of a w x h window that is not the window where the window has room: even, at least 2 x 2, inside"""
    x, y = 2 * (w // 8), 2 * (h // 12)
    return (x, y, w - x - 2 * (w // 6), h - y - 2 * (h // 10))


def test_the_rectangles_are_the_models():
    """lh264_view_rects against view_model.rects over every even w, h in 2..68 plus {144, 176, 288, 352, 1080, 1920, 16384}, every even
    OW, OH in 2..38 plus {224, 398, 4096}, all three fits, with and without a crop; every rectangle is even, at least 2 x 2 and inside"""
    L, lib = _lib()
    ws = list(range(2, 70, 2)) + [144, 176, 288, 352, 1080, 1920, 16384]
    os_ = list(range(2, 40, 2)) + [224, 398, 4096]
    s, d, c = L.Rect(), L.Rect(), L.Rect()
    ps, pd, pc = C.byref(s), C.byref(d), C.byref(c)
    fn, rects = lib.lh264_view_rects, VM.rects
    n = 0
    for w in ws:
        for h in ws:
            crop = _some_crop(w, h)
            assert VM.crop_fits(crop, w, h)
            c.x, c.y, c.w, c.h = crop
            for cr, ptr, (bx, by, bw, bh) in ((None, None, (0, 0, w, h)), (crop, pc, crop)):
                for name, fit in VM.FIT.items():
                    for OW in os_:
                        for OH in os_:
                            assert fn(w, h, ptr, fit, OW, OH, ps, pd) == 0
                            got = ((s.x, s.y, s.w, s.h), (d.x, d.y, d.w, d.h))
                            if got != rects(w, h, cr, name, (OW, OH)):
                                raise AssertionError((w, h, cr, name, OW, OH, got, rects(w, h, cr, name, (OW, OH))))
                            if (s.x | s.y | s.w | s.h | d.x | d.y | d.w | d.h) & 1 or s.w < 2 or s.h < 2 or d.w < 2 or d.h < 2 or s.x < bx or s.y < by or \
                               s.x + s.w > bx + bw or s.y + s.h > by + bh or d.x < 0 or d.y < 0 or d.x + d.w > OW or d.y + d.h > OH:
                                raise AssertionError((w, h, cr, name, OW, OH, got))
                            n += 1
    assert n == 41 * 41 * 2 * 3 * 22 * 22


def test_the_rectangles_by_hand():
    """the examples of the header, without a size, and what lh264_view_rects refuses"""
    L, lib = _lib()
    import losslessh264_amd as lh
    assert lh.view_rects(176, 144, None, "cover", (224, 224)) == ((16, 0, 144, 144), (0, 0, 224, 224))
    assert lh.view_rects(176, 144, None, "contain", (224, 224)) == ((0, 0, 176, 144), (0, 20, 224, 184))
    assert lh.view_rects(1920, 1080, None, "cover", (224, 224)) == ((420, 0, 1080, 1080), (0, 0, 224, 224))
    assert lh.view_rects(1920, 1080, None, "contain", (224, 224)) == ((0, 0, 1920, 1080), (0, 48, 224, 126))
    assert lh.view_rects(2, 2, None, "contain", (4096, 2)) == ((0, 0, 2, 2), (2046, 0, 2, 2))
    assert VM.rects(176, 144, None, "cover", (224, 224)) == ((16, 0, 144, 144), (0, 0, 224, 224))
    assert VM.rects(1920, 1080, None, "contain", (224, 224)) == ((0, 0, 1920, 1080), (0, 48, 224, 126))
    assert VM.rects(2, 2, None, "contain", (4096, 2)) == ((0, 0, 2, 2), (2046, 0, 2, 2))
    assert lh.view_rects(176, 144) == ((0, 0, 176, 144), (0, 0, 176, 144))
    assert lh.view_rects(176, 144, (16, 2, 100, 60)) == ((16, 2, 100, 60), (0, 0, 100, 60))
    assert lh.view_rects(176, 144, (16, 2, 100, 60), "stretch", (22, 18)) == ((16, 2, 100, 60), (0, 0, 22, 18))
    assert lh.view_rects(176, 144, (16, 2, 100, 60), "cover", (20, 20)) == ((36, 2, 60, 60), (0, 0, 20, 20))     # inside the crop
    assert lh.view_rects(176, 144, None, "cover", (176, 144)) == lh.view_rects(176, 144, None, "contain", (176, 144)) == ((0, 0, 176, 144), (0, 0, 176, 144))
    s, d = L.Rect(), L.Rect()
    bad_crops = [(0, 0, 178, 144), (2, 0, 176, 144), (0, 2, 176, 144), (1, 0, 2, 2), (0, 0, 3, 2), (-2, 0, 4, 4), (0, 0, 0, 2), (0, 0, 2, 0)]
    for crop in bad_crops:
        assert lib.lh264_view_rects(176, 144, C.byref(L.Rect(*crop)), 0, 0, 0, C.byref(s), C.byref(d)) == L.E_ARG, crop
    assert lib.lh264_view_rects(176, 144, C.byref(L.Rect(0, 0, 0, 0)), 0, 0, 0, C.byref(s), C.byref(d)) == 0 and (s.w, s.h) == (176, 144)
    for args in ((175, 144, None, 0, 0, 0), (0, 144, None, 0, 0, 0), (16386, 2, None, 0, 0, 0), (176, 144, None, 3, 224, 224), (176, 144, None, 1, 0, 0),
                 (176, 144, None, 2, 0, 0), (176, 144, None, 0, 224, 0), (176, 144, None, 0, 223, 224), (176, 144, None, 0, 4098, 2)):
        assert lib.lh264_view_rects(*args, C.byref(s), C.byref(d)) == L.E_ARG, args
    assert lib.lh264_view_rects(176, 144, None, 1, 224, 224, None, None) == 0
    for bad in (dict(fit="fill"), dict(crop=(0, 0, 178, 144)), dict(crop=(0, 0, 3, 2)), dict(fit="cover")):
        with pytest.raises(ValueError):
            lh.view_rects(176, 144, **bad)


# ---- the stepped kernel code ------------------------------------------------------------------------------------------------------------
def places(w, h, size):
    """[(place, fill)] for a w x h window in a size picture: the centred one of the definition, and rectangles that are not - the whole
    output, {2, 2, ..} and {6, 0, ..} (a 4-byte piece and an 8-pixel piece straddle the seam; the latter leaves a bar of exactly 2
    columns), the last quad alone, bars of exactly 2 rows"""
    OW, OH = size
    out = [(VM.rects(w, h, None, "contain", size)[1], FILLS[3]), ((0, 0, OW, OH), FILLS[2])]
    if OW >= 6 and OH >= 6:
        out.append(((2, 2, OW - 4, OH - 4), FILLS[0]))
        out.append(((0, 2, OW, OH - 4), FILLS[2]))
    if OW >= 10:
        out.append(((6, 0, OW - 8, OH), FILLS[1]))
    out.append(((OW - 2, OH - 2, 2, 2), FILLS[3]))
    return out


_cases = {}


def case_of(window, content):
    if (window, content) not in _cases:
        _cases[(window, content)] = SC.Case(*window, seed=17 * window[0] + window[1], content=content)
    return _cases[(window, content)]


def float_factors():
    import losslessh264_amd as lh
    return tuple(tuple(SM.f32(x) for x in t) for t in lh.normalise(*IMAGENET))


def expected(case, size, place, fill, variant, std):
    """the bytes the definition gives for one job (flat uint8): variant ("yuv", fmt) | ("rgb", layout) | ("float", layout, type)"""
    memo = case.__dict__.setdefault("_view", {})
    key = (size, place, fill)
    if key not in memo:
        memo[key] = VM.placed_planes(case.Y, case.U, case.V, place, fill, size)
    planes = memo[key]
    if variant[0] == "yuv":
        return np.frombuffer(scale_ref.pack(*planes, variant[1]), dtype=np.uint8)
    rkey = (size, place, fill, variant[1], std)
    if rkey not in memo:
        memo[rkey] = VM.rgb_of(planes, variant[1], *rgb_model.STANDARDS[std])
    if variant[0] == "rgb":
        return memo[rkey]
    mul, add = float_factors()
    return VM.float_of(memo[rkey], variant[1], variant[2], mul, add)


def plan(path, windows=None):
    """per output size the jobs of one call of a path ("yuv" | "rgb" | "float"): [(window, content, place, fill, variant, offset, std)].
    Random content goes to every place at every destination offset of the path (0..15; the multiples of 4 for floats) for the
    centred place and two offsets for the others, the flat and checker contents to the centred place and the whole output"""
    variants = {"yuv": [("yuv", 0), ("yuv", 1)], "rgb": [("rgb", l) for l in LAYOUTS], "float": [("float", l, t) for l in LAYOUTS for t in TYPES]}[path]
    all_offs, few = (range(0, 16, 4), (0, 12)) if path == "float" else (range(16), (0, 3))
    by_size = {}
    for window in windows or WINDOWS:
        for content in CONTENTS:
            for size in OUTPUTS:
                pl = places(*window[:2], size)
                for q, (place, fill) in enumerate(pl if content == "random" else pl[:2]):
                    for variant in variants:
                        for off in (all_offs if content == "random" and q == 0 else few):
                            jobs = by_size.setdefault(size, [])
                            jobs.append((window, content, place, fill, variant, off, len(jobs) & 3))
    return by_size


def element_bytes(variant):
    return SM.ELEMENT_BYTES[variant[2]] if variant[0] == "float" else 1


def job_bytes(size, variant):
    return size[0] * size[1] * 3 // 2 if variant[0] == "yuv" else size[0] * size[1] * 3 * element_bytes(variant)


def run_jobs(L, fn, size, jobs_of, src_ptr_of, dst_ptr, slot):
    """one call of a placed entry point: job q's picture at dst_ptr + q * slot + GUARD + its offset -> [(first byte, expected bytes)]"""
    n = len(jobs_of)
    jobs, pls, std = (L.PackJob * n)(), (L.PackPlace * n)(), (C.c_uint8 * n)()
    placed = []
    first = jobs_of[0][4]
    for q, (window, content, place, fill, variant, off, sd) in enumerate(jobs_of):
        assert variant[0] == first[0] and (variant[0] == "yuv" or variant[1:] == first[1:])      # one call, one kernel instance
        case = case_of(window, content)
        at = q * slot + SC.GUARD + off
        case.fill_job(jobs[q], src_ptr_of(case), dst_ptr + at, variant[1] if variant[0] == "yuv" else L.FMT_I420, 0)
        pls[q].x, pls[q].y, pls[q].w, pls[q].h = place
        pls[q].fill = fill_word(fill)
        std[q] = sd
        placed.append((at, expected(case, size, place, fill, variant, sd)))
    colour = 0 if first[0] == "yuv" else rgb_model.LAYOUTS[first[1]]
    sm = None
    if first[0] == "float":
        mul, add = float_factors()
        sm = L.DecodeSample()
        sm.struct_bytes, sm.type = 32, L.SAMPLE[first[2]]
        for k in range(3):
            sm.mul[k], sm.add[k] = float(mul[k]), float(add[k])
    assert fn(jobs, pls, n, size[0], size[1], colour, std, C.byref(sm) if sm is not None else None) == 0
    return placed


def groups(jobs_of):
    """the jobs of one size by kernel instance: a call takes one colour and one sample type"""
    out = {}
    for j in jobs_of:
        out.setdefault(j[4] if j[4][0] != "yuv" else ("yuv",), []).append(j)
    return out.values()


def check(got, placed, what):
    mask = np.ones(got.size, dtype=bool)
    for at, exp in placed:
        assert np.array_equal(got[at:at + exp.size], exp), (what, at, np.flatnonzero(got[at:at + exp.size] != exp)[:8])
        mask[at:at + exp.size] = False
    assert np.all(got[mask] == 0xa5), what


def _step(path, window):
    L, lib = _lib()
    for size, jobs_of in sorted(plan(path, [window]).items()):
        for grp in groups(jobs_of):
            slot = (SC.GUARD + 16 + job_bytes(size, grp[0][4]) + SC.GUARD + 15) & ~15
            raw = np.full(slot * len(grp) + 16, 0xa5, dtype=np.uint8)
            base = (-raw.ctypes.data) % 16
            buf = raw[base:base + slot * len(grp)]
            placed = run_jobs(L, lib.lh264_debug_view_cpu, size, grp, lambda case: case.buf.ctypes.data, buf.ctypes.data, slot)
            check(buf, placed, (path, window, size, grp[0][4]))
            assert np.all(raw[:base] == 0xa5) and np.all(raw[base + buf.size:] == 0xa5)


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d@%d,%d" % w)
def test_placed_planes_on_the_host(window):
    """pack_band_placed stepped: every content, every output, both formats, the places of places(), destination offsets 0..15"""
    _step("yuv", window)


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d@%d,%d" % w)
def test_placed_rgb_on_the_host(window):
    """pack_band_rgb_placed stepped: both layouts, the four standards, a bar pixel is the conversion of the fill"""
    _step("rgb", window)


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d@%d,%d" % w)
def test_placed_floats_on_the_host(window):
    """pack_band_sample_placed stepped: both layouts, the three float types, destination offsets 0, 4, 8, 12"""
    _step("float", window)


def test_the_plan_covers_what_it_says():
    for path, n_var in (("yuv", 2), ("rgb", 2), ("float", 6)):
        by_size = plan(path)
        assert sorted(by_size) == sorted(OUTPUTS)
        seen = [j for jobs in by_size.values() for j in jobs]
        assert {j[0] for j in seen} == set(WINDOWS) and {j[1] for j in seen} == set(CONTENTS) and {j[3] for j in seen} == set(FILLS)
        assert len({j[4] for j in seen}) == n_var and {j[6] for j in seen} == {0, 1, 2, 3}
        assert {j[5] for j in seen} == (set(range(0, 16, 4)) if path == "float" else set(range(16)))
        pl = {(j[2], s) for s, jobs in by_size.items() for j in jobs}
        assert ((2, 2, 220, 220), (224, 224)) in pl and ((6, 0, 216, 224), (224, 224)) in pl and ((222, 222, 2, 2), (224, 224)) in pl
        assert ((0, 2, 224, 220), (224, 224)) in pl and ((0, 20, 224, 184), (224, 224)) in pl and ((2046, 0, 2, 2), (4096, 2)) in pl


def test_the_whole_output_is_the_unplaced_kernels():
    """a place that is the whole output delivers lh264_debug_resize_cpu / _rgb_cpu / _sample_cpu byte for byte, whatever the fill"""
    L, lib = _lib()
    mul, add = float_factors()
    sm = L.DecodeSample()
    sm.struct_bytes, sm.type = 32, L.SAMPLE["float16"]
    for k in range(3):
        sm.mul[k], sm.add[k] = float(mul[k]), float(add[k])
    for window in WINDOWS:
        case = case_of(window, "random")
        for size in ((10, 6), (46, 38), (224, 224)):
            for colour, sample, nbytes, fmt in ((0, None, size[0] * size[1] * 3 // 2, L.FMT_NV12), (1, None, size[0] * size[1] * 3, 0), (2, sm, size[0] * size[1] * 6, 0)):
                a, b = np.full(nbytes + 32, 0xa5, dtype=np.uint8), np.full(nbytes + 32, 0xa5, dtype=np.uint8)
                ja, jb = L.PackJob(), L.PackJob()
                case.fill_job(ja, case.buf.ctypes.data, a.ctypes.data + (-a.ctypes.data) % 16, fmt, 0)
                case.fill_job(jb, case.buf.ctypes.data, b.ctypes.data + (-b.ctypes.data) % 16, fmt, 0)
                pl = L.PackPlace(0, 0, size[0], size[1], fill_word(FILLS[3]), 0)
                std = (C.c_uint8 * 1)(3)
                assert lib.lh264_debug_view_cpu(C.byref(ja), C.byref(pl), 1, size[0], size[1], colour, std, C.byref(sample) if sample else None) == 0
                if sample:
                    assert lib.lh264_debug_sample_cpu(C.byref(jb), 1, size[0], size[1], colour, std, C.byref(sample)) == 0
                elif colour:
                    assert lib.lh264_debug_rgb_cpu(C.byref(jb), 1, size[0], size[1], colour, std) == 0
                else:
                    assert lib.lh264_debug_resize_cpu(C.byref(jb), 1, size[0], size[1]) == 0
                ga, gb = a[(-a.ctypes.data) % 16:], b[(-b.ctypes.data) % 16:]
                assert np.array_equal(ga[:nbytes], gb[:nbytes]) and not np.all(ga[:nbytes] == 0xa5), (window, size, colour)


# ---- the struct and the arguments -------------------------------------------------------------------------------------------------------
def test_layout_of_the_view_struct():
    """sizeof 32 with fit at 4, fill at 8, n_crops at 12, crops at 16, the reserved words at 24 and 28; the rectangle 16 and the place
    24 bytes: the Python mirrors and a C compiler agree"""
    L, lib = _lib()
    V, P = L.DecodeView, L.PackPlace
    assert C.sizeof(V) == 32 and (V.fit.offset, V.fill.offset, V.n_crops.offset, V.crops.offset, V.reserved0.offset, V.reserved1.offset) == (4, 8, 12, 16, 24, 28)
    assert C.sizeof(L.Rect) == 16 and C.sizeof(P) == 24 and (P.w.offset, P.fill.offset, P.reserved.offset) == (8, 16, 20)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lh264.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u %u\\n", ' \
          'sizeof(lh264_decode_view_t), offsetof(lh264_decode_view_t, fit), offsetof(lh264_decode_view_t, fill), offsetof(lh264_decode_view_t, n_crops), ' \
          'offsetof(lh264_decode_view_t, crops), offsetof(lh264_decode_view_t, reserved0), offsetof(lh264_decode_view_t, reserved1), sizeof(lh264_rect_t), ' \
          'sizeof(lh264_pack_place_t), offsetof(lh264_pack_place_t, fill), offsetof(lh264_pack_place_t, reserved), LH264_FIT_STRETCH, LH264_FIT_COVER, LH264_FIT_CONTAIN); return 0; }\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        assert subprocess.check_output([os.path.join(d, "t")]).decode().split() == ["32", "4", "8", "12", "16", "24", "28", "16", "24", "16", "20", "0", "1", "2"]
    assert L.FIT == {"stretch": 0, "cover": 1, "contain": 2}
    txt = open(os.path.join(ROOT, "include", "lh264.h")).read()
    for name in ("lh264_decode_batch_ex3", "lh264_decoded_picture_view", "lh264_view_rects", "lh264_parser_window", "lh264_debug_view_cpu", "lh264_debug_view_dev"):
        assert "int %s (" % name in txt and name in L.EXPORTS, name


def test_arguments_are_checked_before_the_device():
    """every LH264_E_ARG case of the view is reported where there is no device and leaves `out` alone; a valid view is accepted
    (LH264_E_NODEVICE where there is no device); a NULL view is refused or accepted exactly as lh264_decode_batch_ex2 is"""
    L, lib = _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    ptrs, lens = (C.c_char_p * 2)(data, data), (C.c_size_t * 2)(len(data), len(data))
    outs = (C.c_void_p * 2)()
    sentinel = 0x4321
    import torch
    accepted = 0 if torch.cuda.is_available() else L.E_NODEVICE

    def call(o, v, ext=None, sm=None, ex2=False):
        outs[0] = outs[1] = sentinel
        args = (ptrs, lens, 2, 1, C.byref(o) if o is not None else None, C.byref(ext) if ext is not None else None, C.byref(sm) if sm is not None else None)
        rc = lib.lh264_decode_batch_ex2(*args, outs) if ex2 else lib.lh264_decode_batch_ex3(*args, C.byref(v) if v is not None else None, outs)
        if rc == 0:
            lib.lh264_decoded_free(outs[0])
            lib.lh264_decoded_free(outs[1])
        else:
            assert outs[0] == sentinel and outs[1] == sentinel
        return rc

    def view(**kw):
        v = L.DecodeView()
        v.struct_bytes = 32
        for k, x in kw.items():
            setattr(v, k, x)
        return v
    sized, plain = L.DecodeOptsV6(), L.DecodeOptsV6()
    sized.struct_bytes = plain.struct_bytes = 88
    sized.out_width = sized.out_height = 224
    one = (L.Rect * 1)(L.Rect(16, 0, 144, 144))
    two = (L.Rect * 2)(L.Rect(16, 0, 144, 144), L.Rect(0, 0, 0, 0))
    three = (L.Rect * 3)()
    for nbytes in (0, 24, 28, 31, 33, 36, 40):
        assert call(sized, view(struct_bytes=nbytes)) == L.E_ARG, nbytes
    for fit in (3, 4, 0xffffffff):
        assert call(sized, view(fit=fit)) == L.E_ARG, fit
    for fit in (1, 2):
        assert call(plain, view(fit=fit)) == L.E_ARG and call(None, view(fit=fit)) == L.E_ARG, fit      # no size
    for fit, fill in ((0, 1), (1, 0x808010), (2, 0x1000000), (2, 0xff000000), (0, 0x80000000)):
        assert call(sized, view(fit=fit, fill=fill)) == L.E_ARG, (fit, fill)
    for r0, r1 in ((1, 0), (0, 1), (0xffffffff, 0)):
        assert call(sized, view(reserved0=r0, reserved1=r1)) == L.E_ARG, (r0, r1)
    assert call(sized, view(n_crops=3, crops=three)) == L.E_ARG                          # neither 0, 1 nor n
    for n_crops in (1, 2):
        assert call(sized, view(n_crops=n_crops)) == L.E_ARG, n_crops                    # crops NULL
    for bad in ((-2, 0, 4, 4), (0, -2, 4, 4), (1, 0, 4, 4), (0, 1, 4, 4), (0, 0, 3, 4), (0, 0, 4, 3), (0, 0, -4, 4), (0, 0, 4, -4), (0, 0, 0, 4), (0, 0, 4, 0), (2, 2, 0, 0x7ffffffe)):
        assert call(plain, view(n_crops=1, crops=(L.Rect * 1)(L.Rect(*bad)))) == L.E_ARG, bad
        assert call(plain, view(n_crops=2, crops=(L.Rect * 2)(L.Rect(0, 0, 0, 0), L.Rect(*bad)))) == L.E_ARG, bad
    # what is accepted: no view, an empty view, each fit with a size, every fill under contain, crops for all and per stream, a crop
    # no window will fit (that is known at the picture), with colour and a float type
    assert call(sized, None) == call(sized, None, ex2=True) == accepted and call(None, None) == call(None, None, ex2=True) == accepted
    for o, v in ((plain, view()), (sized, view()), (sized, view(fit=1)), (sized, view(fit=2)), (sized, view(fit=2, fill=0xffffff)), (sized, view(fit=2, fill=0xf05a51)),
                 (plain, view(n_crops=1, crops=one)), (sized, view(fit=1, n_crops=2, crops=two)), (plain, view(n_crops=1, crops=(L.Rect * 1)(L.Rect(0, 0, 16384, 16384)))),
                 (None, view()), (None, view(n_crops=2, crops=two))):
        assert call(o, v) == accepted
    ext = L.DecodeExt()
    ext.struct_bytes, ext.colour = 24, 2
    sm = L.DecodeSample()
    sm.struct_bytes, sm.type = 32, L.SAMPLE["float16"]
    for k in range(3):
        sm.mul[k] = 1.0
    assert call(sized, view(fit=2, fill=0x808010), ext, sm) == accepted
    assert call(sized, view(fit=3), ext, sm) == L.E_ARG
    # a NULL view is lh264_decode_batch_ex2: the same refusals
    bad_o = L.DecodeOptsV6()
    bad_o.struct_bytes, bad_o.out_width = 88, 223
    bad_sm = L.DecodeSample()
    bad_sm.struct_bytes, bad_sm.type = 32, 4
    for o, e, s in ((bad_o, None, None), (sized, ext, bad_sm), (sized, None, sm)):
        assert call(o, None, e, s) == call(o, None, e, s, ex2=True) == L.E_ARG
    assert call(bad_o, view(fit=1)) == L.E_ARG


def test_the_debug_entry_points_check_their_arguments():
    """places NULL, a place that is odd, below 2 x 2 or outside the picture, a fill above 24 bits, a reserved word, and what the
    siblings refuse, are LH264_E_ARG from both entry points and nothing is written; lh264_debug_view_dev without a device is
    LH264_E_NODEVICE"""
    L, lib = _lib()
    case = SC.Case(16, 16, 0, 0)
    buf = np.full(8192, 0xa5, dtype=np.uint8)
    j = L.PackJob()
    case.fill_job(j, case.buf.ctypes.data, buf.ctypes.data + (-buf.ctypes.data) % 16 + 64, L.FMT_I420, 0)
    std = (C.c_uint8 * 1)(0)
    sm = L.DecodeSample()
    sm.struct_bytes, sm.type = 32, L.SAMPLE["float32"]
    ok = L.PackPlace(2, 2, 12, 12, 0x808010, 0)
    for fn in (lib.lh264_debug_view_cpu, lib.lh264_debug_view_dev):
        for bad in ((1, 2, 12, 12, 0, 0), (2, 1, 12, 12, 0, 0), (2, 2, 11, 12, 0, 0), (2, 2, 12, 11, 0, 0), (0, 0, 0, 16, 0, 0), (0, 0, 16, 0, 0, 0), (-2, 0, 16, 16, 0, 0),
                    (0, -2, 16, 16, 0, 0), (2, 0, 16, 16, 0, 0), (0, 2, 16, 16, 0, 0), (0, 0, 18, 16, 0, 0), (16, 16, 2, 2, 0, 0), (0x7ffffffe, 0, 4, 4, 0, 0),
                    (2, 2, 12, 12, 0x1000000, 0), (2, 2, 12, 12, 0x80000000, 0), (2, 2, 12, 12, 0, 1)):
            for colour, s in ((0, None), (1, None), (2, sm)):
                assert fn(C.byref(j), C.byref(L.PackPlace(*bad)), 1, 16, 16, colour, std, C.byref(s) if s else None) == L.E_ARG, (bad, colour)
        assert fn(C.byref(j), None, 1, 16, 16, 0, std, None) == L.E_ARG and fn(None, C.byref(ok), 1, 16, 16, 0, std, None) == L.E_ARG
        assert fn(C.byref(j), C.byref(ok), 0, 16, 16, 0, std, None) == L.E_ARG
        for size in ((0, 0), (16, 0), (15, 16), (4098, 16)):
            assert fn(C.byref(j), C.byref(ok), 1, size[0], size[1], 0, std, None) == L.E_ARG, size
        assert fn(C.byref(j), C.byref(ok), 1, 16, 16, 3, std, None) == L.E_ARG and fn(C.byref(j), C.byref(ok), 1, 16, 16, 1, None, None) == L.E_ARG
        assert fn(C.byref(j), C.byref(ok), 1, 16, 16, 0, std, C.byref(sm)) == L.E_ARG          # a float type without a layout
        j.reserved = 1
        assert fn(C.byref(j), C.byref(ok), 1, 16, 16, 0, std, None) == L.E_ARG
        j.reserved, j.format = 0, L.FMT_NV12
        assert fn(C.byref(j), C.byref(ok), 1, 16, 16, 1, std, None) == L.E_ARG
        j.format = L.FMT_I420
        j.dst += 2
        assert fn(C.byref(j), C.byref(ok), 1, 16, 16, 2, std, C.byref(sm)) == L.E_ARG          # a float destination that is no multiple of 4
        j.dst -= 2
    assert np.all(buf == 0xa5)
    import torch
    if not torch.cuda.is_available():
        assert lib.lh264_debug_view_dev(C.byref(j), C.byref(ok), 1, 16, 16, 0, std, None) == L.E_NODEVICE
        assert np.all(buf == 0xa5)


def test_the_window_of_a_stream():
    """lh264_parser_window: BA_MW_D is 176 x 144; CVFC1_Sony_C's SPS crops, and the window is what the parser gives its first picture,
    not the coded size; a file without an SPS that parses is LH264_E_UNSUPPORTED and leaves the outputs alone"""
    L, lib = _lib()
    import losslessh264_amd as lh
    assert lh.stream_window(open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()) == (176, 144)
    data = open(os.path.join(STREAMS, "CVFC1_Sony_C.jsv"), "rb").read()
    win = lh.stream_window(data)
    frames, err, _ = lh.parse_file(data)
    assert err == "" and win == (frames[0].crop_w, frames[0].crop_h) and win != (frames[0].mb_w * 16, frames[0].mb_h * 16)
    assert lh.stream_window(b"") is None and lh.stream_window(b"\x00\x00\x01\x65\x88\x84\x00") is None and lh.stream_window(b"\x00\x00\x01\x67\xff") is None
    w, h = C.c_int32(7), C.c_int32(7)
    assert lib.lh264_parser_window(None, 0, C.byref(w), C.byref(h)) == L.E_ARG
    assert lib.lh264_parser_window(b"\x00\x00\x01\x09\x10", 5, C.byref(w), C.byref(h)) == L.E_UNSUPPORTED and (w.value, h.value) == (7, 7)
    assert lib.lh264_parser_window(data, len(data), None, None) == 0


def test_python_refuses_a_bad_view():
    import losslessh264_amd as lh
    _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    for bad in (dict(fit="fill"), dict(fit="cover"), dict(fit="contain"), dict(fit=1, size=(224, 224)), dict(fill=(16, 128, 128)), dict(fill=(16, 128, 128), fit="cover", size=(224, 224)),
                dict(fit="contain", size=(224, 224), fill=(16, 128)), dict(fit="contain", size=(224, 224), fill=(16, 128, 256)), dict(fit="contain", size=(224, 224), fill=(16, 128, -1)),
                dict(fit="contain", size=(224, 224), fill=(16.0, 128, 128)), dict(fit="contain", size=(224, 224), fill=0x808010),
                dict(crop=(0, 0, 176)), dict(crop=(1, 0, 4, 4)), dict(crop=(0, 0, 3, 4)), dict(crop=(0, 0, 0, 0)), dict(crop=(-2, 0, 4, 4)), dict(crop=(0, 0, 4.0, 4)),
                dict(crop=[(0, 0, 4, 4), None]), dict(crop=[]), dict(crop="0,0,4,4")):
        with pytest.raises(ValueError):
            lh.decode_batch([data], **bad)


def test_the_command_lines_refuse_a_bad_view(tmp_path):
    """--fit takes cover | contain and needs --size, --fill takes y,cb,cr in 0..255 and needs --fit contain, --crop takes x,y,w,h even:
    anything else ends both command lines with the usage code before a stream is read or a device looked for"""
    src = os.path.join(STREAMS, "BA_MW_D.264")
    _lib()
    bad = [["--fit", "fill", "--size", "224x224"], ["--fit", "cover"], ["--fit", "contain"], ["--fill", "16,128,128"], ["--fill", "16,128,128", "--fit", "cover", "--size", "224x224"],
           ["--fit", "contain", "--size", "224x224", "--fill", "16,128"], ["--fit", "contain", "--size", "224x224", "--fill", "16,128,256"],
           ["--fit", "contain", "--size", "224x224", "--fill", "a,b,c"], ["--crop", "0,0,176"], ["--crop", "1,0,4,4"], ["--crop", "0,0,3,4"], ["--crop", "0,0,0,0"],
           ["--crop", "0,0,4,4,4"], ["--crop", "x"]]
    for cmd in ([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"]):
        for args in bad:
            r = subprocess.run(cmd + ["--decode"] + args + [str(tmp_path), src], capture_output=True, timeout=120, cwd=ROOT)
            assert r.returncode == 2 and (b"--fit" in r.stdout + r.stderr or b"--crop" in r.stdout + r.stderr or b"--fill" in r.stdout + r.stderr), (cmd, args, r.stdout, r.stderr)
            assert os.listdir(str(tmp_path)) == []
