"""Bilinear and bicubic resampling of a sized decode (lh264_decode_batch_ex6) where no device is present: the weight tables
(lh264_filter_taps) against tests/filter_model.py; the code of the three filtered kernels stepped on the host (lh264_debug_filter_cpu)
over synthetic padded pictures against the model, in 0xA5 guard bytes; the model against torch's antialiased interpolation; the layout
of the filter struct and the arguments of the call and of the entry points."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import filter_model as FM
import rgb_model
import sample_model as SM
import scale_cases as SC
import scale_ref
import view_model as VM
from test_decode_sample import IMAGENET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")

NAMES = ["bilinear", "bicubic"]
PAIRS = [(176, 224), (144, 224), (88, 112), (72, 112), (176, 176), (176, 88), (176, 22), (1920, 224), (1080, 224), (960, 112), (16, 2), (2, 16), (8, 6), (6, 8),
         (10, 4), (3, 2), (1, 2), (5, 16), (33, 2), (4096, 2), (2, 4096), (16384, 2)]
WINDOWS = [(2, 2), (6, 10), (16, 16), (64, 48), (176, 144), (2048, 4), (4, 2048)]
SIZES = [(2, 2), (6, 10), (8, 8), (16, 16), (22, 18), (224, 224)]
CONTENTS = ["random", "checker", 0, 255, "step"]
FILL = (81, 90, 240)
TORCH_CASES = [((144, 176), (224, 224)), ((72, 88), (112, 112)), ((1080, 1920), (224, 224)), ((16, 16), (6, 10)), ((6, 10), (16, 16)), ((2, 2), (8, 8)),
               ((144, 176), (18, 22)), ((48, 64), (2, 2))]


def _lib():
    import __graft_entry__ as g
    g.build()
    from losslessh264_amd import _lib as L
    return L, L.lib()


def fill_word(f):
    return f[0] | f[1] << 8 | f[2] << 16


# ---- the weights ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_weights_are_the_models(name):
    """lh264_filter_taps against the model for every delivered coordinate of every length pair; every row sums to 2^14, every weight
    fits int16, the absolute weights of a row stay at or below 20,480, and equal lengths give the single weight 2^14"""
    _lib()
    import losslessh264_amd as lh
    for src, dst in PAIRS:
        got = lh.filter_taps(name, src, dst)
        want = FM.rows(name, src, dst)
        assert len(got) == dst and got == want, (name, src, dst, [(a, b) for a, b in zip(got, want) if a != b][:2])
        for X, (first, k) in enumerate(want):
            assert sum(k) == 16384 and all(-32768 <= v <= 32767 for v in k) and sum(abs(v) for v in k) <= 20480, (name, src, dst, X)
            assert first >= 0 and first + len(k) <= src and k[0] != 0 and k[-1] != 0
            if src == dst:
                assert (first, k) == (X, [16384])
    # enlarging, bilinear has two taps a column and one at an edge
    if name == "bilinear":
        for src, dst in ((176, 224), (2, 16), (5, 16)):
            rows = FM.rows(name, src, dst)
            assert {len(k) for _, k in rows} <= {1, 2} and rows[0] == (0, [16384]) and rows[-1] == (src - 1, [16384])
    # long rows: the rounding leaves a remainder, which the largest tap takes - it stands out from its neighbours
    long_row = FM.rows(name, 4096, 2)[0][1]
    peak = max(range(len(long_row)), key=lambda i: abs(long_row[i] - long_row[i - 1]) if i else 0)
    assert len(long_row) > 2000 and abs(long_row[peak] - long_row[peak - 1]) > 2


def test_the_weights_by_hand():
    """2 -> 4 bilinear: centres -1/4, 1/4, 3/4, 5/4; cut at the edges the outer columns replicate, the inner ones weigh 3 : 1"""
    assert FM.rows("bilinear", 2, 4) == [(0, [16384]), (0, [12288, 4096]), (0, [4096, 12288]), (1, [16384])]
    # 4 -> 2 bilinear: the triangle is twice as wide; column 0 sees x = 0, 1, 2 with raw weights 6, 6, 2 (n = 2, 2, 6 of m = 8), R = 14:
    # k = 7022, 7022, 2341, one too many, which the first of the two largest gives back
    assert FM.rows("bilinear", 4, 2)[0] == (0, [7021, 7022, 2341])
    assert FM.raw("bicubic", 0, 8) == 2 * 8 ** 3 and FM.raw("bicubic", 8, 8) == 0 and FM.raw("bicubic", 12, 8) == -12 ** 3 + 5 * 144 * 8 - 8 * 12 * 64 + 4 * 512 < 0


def test_filter_taps_checks_its_arguments():
    L, lib = _lib()
    first, n = C.c_int32(7), C.c_int(7)
    buf = (C.c_int16 * 8)()
    ok = (1, 176, 224, 0)
    assert lib.lh264_filter_taps(*ok, C.byref(first), buf, 8, C.byref(n)) == 0 and (first.value, n.value, buf[0]) == (0, 1, 16384)
    assert lib.lh264_filter_taps(2, 4096, 2, 0, C.byref(first), None, 0, C.byref(n)) == 0 and n.value > 8          # the count, whatever the cap
    assert lib.lh264_filter_taps(2, 4096, 2, 0, C.byref(first), buf, 8, C.byref(n)) == 0 and n.value > 8
    first.value = n.value = 7
    for bad in ((0, 176, 224, 0), (3, 176, 224, 0), (1, 0, 224, 0), (1, 16385, 2, 0), (1, 176, 0, 0), (1, 176, 4097, 0), (1, 176, 224, -1), (1, 176, 224, 224)):
        assert lib.lh264_filter_taps(*bad, C.byref(first), buf, 8, C.byref(n)) == L.E_ARG, bad
    assert lib.lh264_filter_taps(*ok, None, buf, 8, C.byref(n)) == L.E_ARG and lib.lh264_filter_taps(*ok, C.byref(first), buf, 8, None) == L.E_ARG
    assert lib.lh264_filter_taps(*ok, C.byref(first), buf, -1, C.byref(n)) == L.E_ARG and lib.lh264_filter_taps(*ok, C.byref(first), None, 8, C.byref(n)) == L.E_ARG
    assert (first.value, n.value) == (7, 7)
    import losslessh264_amd as lh
    for bad in (("area", 4, 4), ("lanczos", 4, 4), ("bilinear", 0, 4), ("bicubic", 4, 4097)):
        with pytest.raises(ValueError):
            lh.filter_taps(*bad)


# ---- the stepped kernel code ------------------------------------------------------------------------------------------------------------
_cases = {}


def case_of(window, content, crop=(0, 0), pic=None):
    """a padded picture whose window holds the content; "step": 0 left of the middle column, 255 from it on"""
    key = (window, content, crop, pic)
    if key not in _cases:
        kw = dict(pic_w=pic[0], pic_h=pic[1]) if pic else {}
        case = SC.Case(window[0], window[1], crop[0], crop[1], seed=19 * window[0] + window[1], content=0 if content == "step" else content, **kw)
        if content == "step":
            w, h = window
            case.Y = np.repeat((np.arange(w) >= w // 2).astype(np.uint8)[None, :] * 255, h, axis=0)
            case.U = np.repeat((np.arange(w // 2) >= w // 4).astype(np.uint8)[None, :] * 255, h // 2, axis=0)
            case.V = 255 - case.U
            m = SC.MARGIN
            pw, ph = (pic if pic else (((crop[0] + w + 15) & ~15) + 16, ((crop[1] + h + 15) & ~15) + 16))
            planes = [SC._plane(case.Y, crop[0], crop[1], pw, ph, m), SC._plane(case.U, crop[0] // 2, crop[1] // 2, pw // 2, ph // 2, m // 2),
                      SC._plane(case.V, crop[0] // 2, crop[1] // 2, pw // 2, ph // 2, m // 2)]
            assert planes[0].shape[1] == case.stride_y and sum(p.size for p in planes) == case.buf.size
            case.buf = np.concatenate([p.reshape(-1) for p in planes])
        _cases[key] = case
    return _cases[key]


def float_factors():
    import losslessh264_amd as lh
    return tuple(tuple(SM.f32(x) for x in t) for t in lh.normalise(*IMAGENET))


def expected(case, size, place, fill, name, variant, std):
    """the bytes the definition gives for one job (flat uint8): variant ("yuv", fmt) | ("rgb", layout) | ("float", layout, type)"""
    memo = case.__dict__.setdefault("_filtered", {})
    key = (size, place, fill, name)
    if key not in memo:
        memo[key] = FM.placed_planes(case.Y, case.U, case.V, place or (0, 0) + tuple(size), fill, size, name)
    planes = memo[key]
    if variant[0] == "yuv":
        return np.frombuffer(scale_ref.pack(*planes, variant[1]), dtype=np.uint8)
    rgb = FM.rgb_of(planes, variant[1], std)
    if variant[0] == "rgb":
        return rgb
    return FM.float_of(rgb, variant[1], variant[2], *float_factors())


def job_bytes(size, variant):
    return size[0] * size[1] * 3 // 2 if variant[0] == "yuv" else size[0] * size[1] * 3 * (SM.ELEMENT_BYTES[variant[2]] if variant[0] == "float" else 1)


def run_jobs(L, fn, size, name, jobs_of, src_ptr_of, dst_ptr, slot):
    """one call of a filtered entry point over jobs_of = [(case, place or None, fill, variant, offset, std)], all of one variant and all
    placed or none: job q's picture at dst_ptr + q * slot + GUARD + its offset -> [(first byte, expected bytes)]"""
    n = len(jobs_of)
    jobs, pls, std = (L.PackJob * n)(), (L.PackPlace * n)(), (C.c_uint8 * n)()
    first = jobs_of[0][3]
    with_places = jobs_of[0][1] is not None
    out = []
    for q, (case, place, fill, variant, off, sd) in enumerate(jobs_of):
        assert variant[0] == first[0] and (variant[0] == "yuv" or variant == first) and (place is not None) == with_places      # one call, one kernel instance
        at = q * slot + SC.GUARD + off
        case.fill_job(jobs[q], src_ptr_of(case), dst_ptr + at, variant[1] if variant[0] == "yuv" else L.FMT_I420, 0)
        if place is not None:
            pls[q].x, pls[q].y, pls[q].w, pls[q].h = place
            pls[q].fill = fill_word(fill)
        std[q] = sd
        out.append((at, expected(case, size, place, fill, name, variant, sd)))
    colour = 0 if first[0] == "yuv" else rgb_model.LAYOUTS[first[1]]
    sm = None
    if first[0] == "float":
        mul, add = float_factors()
        sm = L.DecodeSample()
        sm.struct_bytes, sm.type = 32, L.SAMPLE[first[2]]
        for k in range(3):
            sm.mul[k], sm.add[k] = float(mul[k]), float(add[k])
    assert fn(jobs, pls if with_places else None, n, size[0], size[1], FM.FILTERS[name], colour, std, C.byref(sm) if sm is not None else None) == 0
    return out


def check(got, placed, what):
    mask = np.ones(got.size, dtype=bool)
    for at, exp in placed:
        assert np.array_equal(got[at:at + exp.size], exp), (what, at, np.flatnonzero(got[at:at + exp.size] != exp)[:8])
        mask[at:at + exp.size] = False
    assert np.all(got[mask] == 0xa5), what


def step_on_host(L, lib, size, name, jobs_of, what):
    slot = (SC.GUARD + 16 + job_bytes(size, jobs_of[0][3]) + SC.GUARD + 15) & ~15
    raw = np.full(slot * len(jobs_of) + 16, 0xa5, dtype=np.uint8)
    base = (-raw.ctypes.data) % 16
    buf = raw[base:base + slot * len(jobs_of)]
    placed = run_jobs(L, lib.lh264_debug_filter_cpu, size, name, jobs_of, lambda case: case.buf.ctypes.data, buf.ctypes.data, slot)
    check(buf, placed, what)
    assert np.all(raw[:base] == 0xa5) and np.all(raw[base + buf.size:] == 0xa5)


def plane_jobs(window):
    """per (size, filter) the jobs of one call over a window: every content in both formats; random content at destination offsets
    0..3 and 7 (every alignment of a 4-byte piece, and an odd one beyond it), the others at 0 and 3"""
    out = {}
    for size in SIZES:
        for name in NAMES:
            out[(size, name)] = [(case_of(window, content), None, FILL, ("yuv", fmt), off, 0)
                                 for content in CONTENTS for fmt in (0, 1) for off in ((0, 1, 2, 3, 7) if content == "random" else (0, 3))]
    return out


def placed_jobs():
    """the placed jobs: small windows at places that leave bars of 2 columns and 2 rows, and the rectangles of view_rects for 176 x 144
    and 1920 x 1080 at 224 x 224 - contain places the whole window, cover's source rectangle is the job's window"""
    out = {}
    for name in NAMES:
        small = []
        for window in ((6, 10), (16, 16)):
            for size in ((16, 16), (22, 18)):
                for place in ((2, 2, size[0] - 4, size[1] - 4), (size[0] - 2, size[1] - 2, 2, 2), (0, 0) + size):
                    small.append((window, size, place))
        for window, size, place in small:
            out.setdefault((size, name), []).extend((case_of(window, "random"), place, FILL, ("yuv", fmt), off, 0) for fmt in (0, 1) for off in (0, 5))
        for (w, h), pic in (((176, 144), None), ((1920, 1080), (1920, 1088))):
            src, dst = VM.rects(w, h, None, "contain", (224, 224))
            out.setdefault(((224, 224), name), []).extend((case_of((w, h), "random", pic=pic), dst, FILL, ("yuv", fmt), 1, 0) for fmt in (0, 1))
            src, dst = VM.rects(w, h, None, "cover", (224, 224))
            assert dst == (0, 0, 224, 224) and src[2:] == (h, h)
            out[((224, 224), name)].append((case_of(src[2:], "random", crop=src[:2], pic=pic or (192, 160)), dst, FILL, ("yuv", 0), 2, 0))
    return out


def colour_jobs():
    """RGB24 / RGBP and the three float types: the two smallest windows and 176 x 144 -> 224 x 224, unplaced and placed, the four standards"""
    out = {}
    variants = [("rgb", l) for l in ("rgb24", "rgbp")] + [("float", l, t) for l in ("rgb24", "rgbp") for t in ("float32", "float16", "bfloat16")]
    for name in NAMES:
        for variant in variants:
            for window, size in (((2, 2), (8, 8)), ((6, 10), (16, 16)), ((176, 144), (224, 224))):
                offs = (0, 4) if variant[0] == "float" else (0, 3)
                out.setdefault((size, name, variant, False), []).extend((case_of(window, "random"), None, FILL, variant, off, q) for q, off in enumerate(offs))
                place = (2, 2, size[0] - 4, size[1] - 4)
                out.setdefault((size, name, variant, True), []).extend((case_of(window, "checker"), place, FILL, variant, off, 2 + q) for q, off in enumerate(offs))
    return out


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d" % w)
def test_filtered_planes_on_the_host(window):
    """pack_band_filtered stepped: every content, every size, both formats, both filters"""
    L, lib = _lib()
    for (size, name), jobs_of in plane_jobs(window).items():
        step_on_host(L, lib, size, name, jobs_of, (window, size, name))


def test_filtered_planes_placed_on_the_host():
    L, lib = _lib()
    for (size, name), jobs_of in placed_jobs().items():
        step_on_host(L, lib, size, name, jobs_of, (size, name))


def test_filtered_colour_and_floats_on_the_host():
    """RGB bytes are rgb_model's function of the filtered planes, float elements sample_model's fma of those bytes, bars included"""
    L, lib = _lib()
    for (size, name, variant, _), jobs_of in colour_jobs().items():
        step_on_host(L, lib, size, name, jobs_of, (size, name, variant))


def test_bicubic_clips_at_both_ends():
    """the checkerboard and the step under bicubic leave 0..255 on both sides before the clip: 176 x 144 -> 224 x 224 has such samples
    (so the stepped comparison above covers the clamp), and the delivered bytes there are 0 and 255"""
    for content in ("checker", "step"):
        case = case_of((176, 144), content)
        raw = FM.unclipped(case.Y, 224, 224, "bicubic")
        below, above = int((raw < 0).sum()), int((raw > 255).sum())
        assert below > 0 and above > 0, (content, below, above)
        out = FM.resample_plane(case.Y, 224, 224, "bicubic")
        assert np.all(out[raw < 0] == 0) and np.all(out[raw > 255] == 255)
    raw = FM.unclipped(case_of((176, 144), "checker").Y, 224, 224, "bilinear")
    assert raw.min() >= 0 and raw.max() <= 255          # a triangle has no negative weight


def _deliver(L, lib, case, size, name):
    n = size[0] * size[1] * 3 // 2
    buf = np.full(n + 32, 0xa5, dtype=np.uint8)
    at = (-buf.ctypes.data) % 16
    j = L.PackJob()
    case.fill_job(j, case.buf.ctypes.data, buf.ctypes.data + at, L.FMT_I420, 0)
    if name == "area":
        assert lib.lh264_debug_resize_cpu(C.byref(j), 1, size[0], size[1]) == 0
    else:
        assert lib.lh264_debug_filter_cpu(C.byref(j), None, 1, size[0], size[1], FM.FILTERS[name], 0, None, None) == 0
    return buf[at:at + n].copy()


def test_the_filters_differ_from_the_area_average_and_from_one_another():
    """every enlarging and every non-integer shrinking case on random content: three different pictures; a size equal to the window:
    the window, from all three"""
    L, lib = _lib()
    n = 0
    for window in WINDOWS:
        case = case_of(window, "random")
        own = np.frombuffer(scale_ref.pack(case.Y, case.U, case.V, 0), dtype=np.uint8)
        for size in SIZES + [window]:
            got = {name: _deliver(L, lib, case, size, name) for name in ["area"] + NAMES}
            if size == window:
                assert all(np.array_equal(g, own) for g in got.values()), window
                continue
            larger = size[0] > window[0] or size[1] > window[1]
            fractional = (size[0] < window[0] and window[0] % size[0]) or (size[1] < window[1] and window[1] % size[1])
            if larger or fractional:
                assert not np.array_equal(got["area"], got["bilinear"]) and not np.array_equal(got["area"], got["bicubic"]) and not np.array_equal(got["bilinear"], got["bicubic"]), (window, size)
                n += 1
    assert n >= 25


# ---- the model against torch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_model_against_torch(name):
    """float64 F.interpolate (antialias=True), rounded half up and clipped: the model differs by at most 1, and on random content in at
    most 2 % of the samples"""
    import torch
    import torch.nn.functional as F
    for (h, w), (oh, ow) in TORCH_CASES:
        rng = np.random.default_rng(1000 * h + w)
        checker = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
        for content, p in (("random", rng.integers(0, 256, (h, w), dtype=np.uint8)), ("checker", checker)):
            ours = FM.resample_plane(p, ow, oh, name).astype(np.int64)
            t = F.interpolate(torch.from_numpy(p.astype(np.float64))[None, None], size=(oh, ow), mode=name, antialias=True, align_corners=False)[0, 0].numpy()
            ref = np.clip(np.floor(t + 0.5), 0, 255).astype(np.int64)
            diff = np.abs(ours - ref)
            share = float((diff != 0).mean())
            print(name, (h, w), (oh, ow), content, "max", int(diff.max()), "share %.4f" % share)
            assert diff.max() <= 1, (name, (h, w), (oh, ow), content, int(diff.max()))
            if content == "random":
                assert share <= 0.02, (name, (h, w), (oh, ow), share)


# ---- the struct and the arguments -------------------------------------------------------------------------------------------------------
def test_layout_of_the_filter_struct():
    L, lib = _lib()
    T = L.DecodeFilter
    assert C.sizeof(T) == 16 and (T.filter.offset, T.reserved0.offset, T.reserved1.offset) == (4, 8, 12)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lh264.h"\nint main(void){ printf("%zu %zu %zu %zu %u %u %u\\n", sizeof(lh264_decode_filter_t), ' \
          'offsetof(lh264_decode_filter_t, filter), offsetof(lh264_decode_filter_t, reserved0), offsetof(lh264_decode_filter_t, reserved1), ' \
          'LH264_FILTER_AREA, LH264_FILTER_BILINEAR, LH264_FILTER_BICUBIC); return 0; }\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        assert subprocess.check_output([os.path.join(d, "t")]).decode().split() == ["16", "4", "8", "12", "0", "1", "2"]
    assert L.FILTER == {"area": 0, "bilinear": 1, "bicubic": 2}
    for name in ("lh264_decode_batch_ex6", "lh264_decoded_filter", "lh264_filter_taps", "lh264_debug_filter_cpu", "lh264_debug_filter_dev"):
        assert name in L.EXPORTS, name
    assert lib.lh264_decoded_filter(None) == L.E_ARG


def test_arguments_are_checked_before_the_device():
    """every LH264_E_ARG case of the filter is reported where there is no device and leaves `out` alone; a valid filter is accepted
    (LH264_E_NODEVICE where there is no device); NULL and LH264_FILTER_AREA are refused or accepted exactly as lh264_decode_batch_ex5 is"""
    L, lib = _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    ptrs, lens = (C.c_char_p * 2)(data, data), (C.c_size_t * 2)(len(data), len(data))
    outs = (C.c_void_p * 2)()
    sentinel = 0x4321
    import torch
    accepted = 0 if torch.cuda.is_available() else L.E_NODEVICE

    def call(o, f, ext=None, sm=None, view=None, ex5=False):
        outs[0] = outs[1] = sentinel
        ref = lambda s: C.byref(s) if s is not None else None
        args = (ptrs, lens, 2, 1, ref(o), ref(ext), ref(sm), ref(view), None, None)
        rc = lib.lh264_decode_batch_ex5(*args, outs) if ex5 else lib.lh264_decode_batch_ex6(*args, ref(f), outs)
        if rc == 0:
            lib.lh264_decoded_free(outs[0])
            lib.lh264_decoded_free(outs[1])
        else:
            assert outs[0] == sentinel and outs[1] == sentinel
        return rc

    def filt(**kw):
        f = L.DecodeFilter()
        f.struct_bytes = 16
        for k, x in kw.items():
            setattr(f, k, x)
        return f
    sized, plain, scaled = L.DecodeOptsV6(), L.DecodeOptsV6(), L.DecodeOptsV6()
    sized.struct_bytes = plain.struct_bytes = scaled.struct_bytes = 88
    sized.out_width = sized.out_height = 224
    scaled.scale_log2 = 1
    for nbytes in (0, 8, 12, 15, 17, 20, 32):
        assert call(sized, filt(struct_bytes=nbytes, filter=1)) == L.E_ARG, nbytes
    for f in (3, 4, 0xffffffff):
        assert call(sized, filt(filter=f)) == L.E_ARG, f
    for r0, r1 in ((1, 0), (0, 1), (0xffffffff, 0)):
        assert call(sized, filt(filter=2, reserved0=r0, reserved1=r1)) == L.E_ARG and call(sized, filt(reserved0=r0, reserved1=r1)) == L.E_ARG, (r0, r1)
    for f in (1, 2):
        assert call(plain, filt(filter=f)) == L.E_ARG and call(None, filt(filter=f)) == L.E_ARG and call(scaled, filt(filter=f)) == L.E_ARG, f
    # accepted: NULL, area with and without a size, both filters with a size, with a view, a colour and a float type
    assert call(sized, None) == call(sized, None, ex5=True) == accepted and call(None, None) == call(None, None, ex5=True) == accepted
    for o, f in ((None, filt()), (plain, filt()), (scaled, filt()), (sized, filt()), (sized, filt(filter=1)), (sized, filt(filter=2))):
        assert call(o, f) == accepted
    view = L.DecodeView()
    view.struct_bytes, view.fit, view.fill = 32, 2, 0x808010
    ext = L.DecodeExt()
    ext.struct_bytes, ext.colour = 24, 2
    sm = L.DecodeSample()
    sm.struct_bytes, sm.type = 32, L.SAMPLE["float16"]
    for k in range(3):
        sm.mul[k] = 1.0
    assert call(sized, filt(filter=2), ext, sm, view) == accepted
    assert call(sized, filt(filter=3), ext, sm, view) == L.E_ARG
    # what lh264_decode_batch_ex5 refuses is refused with a filter too
    bad_o = L.DecodeOptsV6()
    bad_o.struct_bytes, bad_o.out_width = 88, 223
    assert call(bad_o, filt(filter=1)) == call(bad_o, None) == call(bad_o, None, ex5=True) == L.E_ARG


def test_the_debug_entry_points_check_their_arguments():
    """a filter that is not 1 or 2, and what lh264_debug_view_* refuse (but places may be NULL), are LH264_E_ARG from both entry points
    and nothing is written; lh264_debug_filter_dev without a device is LH264_E_NODEVICE"""
    L, lib = _lib()
    case = SC.Case(16, 16, 0, 0)
    buf = np.full(8192, 0xa5, dtype=np.uint8)
    j = L.PackJob()
    case.fill_job(j, case.buf.ctypes.data, buf.ctypes.data + (-buf.ctypes.data) % 16 + 64, L.FMT_I420, 0)
    std = (C.c_uint8 * 1)(0)
    sm = L.DecodeSample()
    sm.struct_bytes, sm.type = 32, L.SAMPLE["float32"]
    ok = L.PackPlace(2, 2, 12, 12, 0x808010, 0)
    for fn in (lib.lh264_debug_filter_cpu, lib.lh264_debug_filter_dev):
        for f in (0, 3, 0xffffffff):
            for pl in (None, C.byref(ok)):
                assert fn(C.byref(j), pl, 1, 16, 16, f, 0, std, None) == L.E_ARG, f
        for bad in ((1, 2, 12, 12, 0, 0), (2, 2, 12, 11, 0, 0), (0, 0, 0, 16, 0, 0), (-2, 0, 16, 16, 0, 0), (0, 2, 16, 16, 0, 0), (16, 16, 2, 2, 0, 0),
                    (2, 2, 12, 12, 0x1000000, 0), (2, 2, 12, 12, 0, 1)):
            for colour, s in ((0, None), (1, None), (2, sm)):
                assert fn(C.byref(j), C.byref(L.PackPlace(*bad)), 1, 16, 16, 1, colour, std, C.byref(s) if s else None) == L.E_ARG, (bad, colour)
        assert fn(None, None, 1, 16, 16, 1, 0, std, None) == L.E_ARG and fn(C.byref(j), None, 0, 16, 16, 1, 0, std, None) == L.E_ARG
        for size in ((0, 0), (16, 0), (15, 16), (4098, 16)):
            assert fn(C.byref(j), None, 1, size[0], size[1], 2, 0, std, None) == L.E_ARG, size
        assert fn(C.byref(j), None, 1, 16, 16, 2, 3, std, None) == L.E_ARG and fn(C.byref(j), None, 1, 16, 16, 2, 1, None, None) == L.E_ARG
        assert fn(C.byref(j), None, 1, 16, 16, 2, 0, std, C.byref(sm)) == L.E_ARG          # a float type without a layout
        j.reserved = 1
        assert fn(C.byref(j), None, 1, 16, 16, 1, 0, std, None) == L.E_ARG
        j.reserved, j.format = 0, L.FMT_NV12
        assert fn(C.byref(j), None, 1, 16, 16, 1, 1, std, None) == L.E_ARG
        j.format = L.FMT_I420
        j.dst += 2
        assert fn(C.byref(j), None, 1, 16, 16, 1, 2, std, C.byref(sm)) == L.E_ARG          # a float destination that is no multiple of 4
        j.dst -= 2
    assert np.all(buf == 0xa5)
    import torch
    if not torch.cuda.is_available():
        assert lib.lh264_debug_filter_dev(C.byref(j), None, 1, 16, 16, 1, 0, std, None) == L.E_NODEVICE
        assert np.all(buf == 0xa5)


def test_python_refuses_a_bad_filter():
    import losslessh264_amd as lh
    _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    for bad in (dict(filter="lanczos", size=(224, 224)), dict(filter=1, size=(224, 224)), dict(filter=None, size=(224, 224)), dict(filter="bilinear"), dict(filter="bicubic", scale=1)):
        with pytest.raises(ValueError):
            lh.decode_batch([data], **bad)


def test_the_command_lines_refuse_a_bad_filter(tmp_path):
    """--filter takes area | bilinear | bicubic, the latter two with --size only: anything else ends both command lines with the usage
    code before a stream is read or a device looked for"""
    src = os.path.join(STREAMS, "BA_MW_D.264")
    _lib()
    bad = [["--filter", "lanczos", "--size", "224x224"], ["--filter", "bicubic"], ["--filter", "bilinear", "--scale", "1"], ["--size", "224x224", "--filter"]]
    for cmd in ([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"]):
        for args in bad:
            r = subprocess.run(cmd + ["--decode"] + args + [str(tmp_path), src], capture_output=True, timeout=120, cwd=ROOT)
            assert r.returncode == 2 and b"--filter" in r.stdout + r.stderr, (cmd, args, r.stdout, r.stderr)
            assert os.listdir(str(tmp_path)) == []
