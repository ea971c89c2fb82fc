"""RGB pictures (lh264_decode_batch_ex, colour) where no device is present: the header's table of factors against the model's own; the
integer function against the real-valued formula over every (Y, Cb, Cr); the code of decode_pack_rgb_kernel stepped on the host
(lh264_debug_rgb_cpu) over directed windows no stream has, against tests/rgb_model.py; the layout of lh264_decode_ext_t and the
arguments of the call; lh264_parser_colour on rewritten SPSs; the usage errors of both command lines."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import h264_synth
import resize_ref
import rgb_model as M
import scale_cases as SC
import scale_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
EDGE = [0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 254, 255]


def _lib():
    import __graft_entry__ as g
    g.build()
    from losslessh264_amd import _lib as L
    return L, L.lib()


# ---- the factors and their accuracy ------------------------------------------------------------------------------------------------------
def test_the_headers_table_is_the_models():
    """LH264_COLOUR_FACTORS, read through a C compiler, row by row in the order of the standard byte, equals the factors the model
    derives from Kr and Kb; the two the definition quotes are there"""
    src = '#include <stdio.h>\n#include <stdint.h>\n#include "lh264.h"\nstatic const int32_t f[4][5] = LH264_COLOUR_FACTORS;\n' \
          'int main(void){ for (int s = 0; s < 4; s++) printf("%d %d %d %d %d\\n", f[s][0], f[s][1], f[s][2], f[s][3], f[s][4]); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        rows = [[int(x) for x in ln.split()] for ln in subprocess.check_output([os.path.join(d, "t")]).decode().splitlines()]
    assert rows == [M.factors(*std)[1] for std in M.STANDARDS]
    assert M.factors("bt601", "full")[1][1] == 91881 and M.factors("bt601", "limited")[1][0] == 76309
    assert [M.factors(*std)[0] for std in M.STANDARDS] == [16, 16, 0, 0]


def test_the_integer_function_is_within_one_of_the_real_formula():
    """all 2^24 (Y, Cb, Cr) and all four standards: |integer - round half up (real)| <= 1 in every channel (the five factors are off by
    at most 1/2 of 1/65536 each, times at most 239 + 2*128: less than 0.01 of a step before the rounding).  Prints the share of triples
    in which any channel differs"""
    cb, cr = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for std in M.STANDARDS:
        differing = 0
        for y in range(256):
            yy = np.full_like(cb, y)
            a, b = M.convert(yy, cb, cr, *std), M.convert_real(yy, cb, cr, *std)
            d = [np.abs(p.astype(np.int16) - q.astype(np.int16)) for p, q in zip(a, b)]
            assert max(int(x.max()) for x in d) <= 1, (std, y)
            differing += int(np.count_nonzero((d[0] | d[1] | d[2]) != 0))
        print("%s %s: %d of %d triples differ by 1 in some channel (%.4f %%)" % (std[0], std[1], differing, 1 << 24, 100.0 * differing / (1 << 24)))
        assert differing < (1 << 24) // 50


def test_the_model_on_numbers_done_by_hand():
    """grey stays grey; the limited range maps 16 to 0 and 235 to 255; saturated chroma clips at both ends"""
    for std in M.STANDARDS:
        lo, hi = (16, 235) if std[1] == "limited" else (0, 255)
        assert [int(c[0]) for c in M.convert([lo], [128], [128], *std)] == [0, 0, 0]
        assert [int(c[0]) for c in M.convert([hi], [128], [128], *std)] == [255, 255, 255]
    assert [int(c[0]) for c in M.convert([128], [128], [255], "bt601", "full")] == [255, 37, 128]      # 128 + 1.402*127 = 306; 128 - .714136*127 = 37.3
    assert [int(c[0]) for c in M.convert([128], [255], [0], "bt601", "full")] == [0, 176, 255]         # 128 - 179.5 < 0; 128 - 43.7 + 91.4 = 175.7
    y = np.array([[10, 20], [30, 40]], dtype=np.uint8)
    u, v = np.array([[128]], dtype=np.uint8), np.array([[128]], dtype=np.uint8)
    assert M.rgb_from_planes(y, u, v, "rgb24", "bt601", "full").tolist() == [10, 10, 10, 20, 20, 20, 30, 30, 30, 40, 40, 40]
    assert M.rgb_from_planes(y, u, v, "rgbp", "bt601", "full").tolist() == [10, 20, 30, 40] * 3


# ---- directed windows through the kernel's code -----------------------------------------------------------------------------------------
class Pic(SC.Case):
    """a scale_cases.Case with given window planes"""

    def __init__(self, Y, U, V, crop_x=0, crop_y=0):
        h, w = Y.shape
        SC.Case.__init__(self, w, h, crop_x, crop_y)
        self.Y, self.U, self.V = Y, U, V
        m = SC.MARGIN
        pic_w, pic_h = ((crop_x + w + 15) & ~15) + 16, ((crop_y + h + 15) & ~15) + 16
        planes = [SC._plane(Y, crop_x, crop_y, pic_w, pic_h, m), SC._plane(U, crop_x // 2, crop_y // 2, pic_w // 2, pic_h // 2, m // 2),
                  SC._plane(V, crop_x // 2, crop_y // 2, pic_w // 2, pic_h // 2, m // 2)]
        assert [p.shape[1] for p in planes[:2]] == [self.stride_y, self.stride_c]
        self.buf = np.concatenate([p.reshape(-1) for p in planes])


def triples_window():
    """94 x 94: the 2x2 quad k carries triple k of EDGE^3 - its chroma samples, and the luma value in all four of its samples (the
    quads behind the 2197 triples repeat the last)"""
    t = np.array([(y, cb, cr) for y in EDGE for cb in EDGE for cr in EDGE], dtype=np.uint8)
    assert len(t) == 2197 <= 47 * 47
    q = np.concatenate([t, np.repeat(t[-1:], 47 * 47 - len(t), axis=0)]).reshape(47, 47, 3)
    return Pic(np.repeat(np.repeat(q[:, :, 0], 2, axis=0), 2, axis=1), q[:, :, 1].copy(), q[:, :, 2].copy())


def directed():
    """[(name, case, [sizings])], a sizing ("scale", s) or ("size", (W, H)); computed once"""
    if not hasattr(directed, "memo"):
        out = [("triples 94x94", triples_window(), [("scale", 0)])]
        for k, (w, h) in enumerate([(2, 2), (4, 2), (6, 2), (6, 16), (10, 6), (18, 34)]):
            out.append(("%dx%d" % (w, h), SC.Case(w, h, 0, 0, seed=31 + k), [("scale", 0)]))
        for k, (w, h, x, y) in enumerate([(10, 6, 6, 2), (18, 34, 2, 6)]):
            out.append(("%dx%d@%d,%d" % (w, h, x, y), SC.Case(w, h, x, y, seed=41 + k),
                        [("scale", 0), ("scale", 1), ("scale", 2), ("scale", 3), ("size", (2, 2)), ("size", (10, 6)), ("size", (6, 18))]))
        directed.memo = out
    return directed.memo


def delivered_planes(case, sizing):
    memo = case.__dict__.setdefault("_delivered", {})
    if sizing not in memo:
        memo[sizing] = scale_ref.scale_planes(case.Y, case.U, case.V, sizing[1]) if sizing[0] == "scale" else resize_ref.resize_planes(case.Y, case.U, case.V, sizing[1])
    return memo[sizing]


def expect_rgb(case, sizing, layout, std):
    memo = case.__dict__.setdefault("_rgb", {})
    if (sizing, layout, std) not in memo:
        memo[(sizing, layout, std)] = M.rgb_from_planes(*delivered_planes(case, sizing), layout, *M.STANDARDS[std])
    return memo[(sizing, layout, std)]


JOBS = [(off, std) for off in range(4) for std in range(4)]      # one table: every destination offset with every standard


def run_table(L, fn, case, sizing, layout, src_ptr, dst_ptr, slot):
    """one call of an RGB entry point with a job per (destination offset, standard), job k's picture at dst_ptr + k * slot + GUARD + off
    -> [(first byte of job k's picture, its expected bytes)]"""
    jobs = (L.PackJob * len(JOBS))()
    std = (C.c_uint8 * len(JOBS))(*[s for _, s in JOBS])
    at = []
    for k, (off, s) in enumerate(JOBS):
        at.append(k * slot + SC.GUARD + off)
        case.fill_job(jobs[k], src_ptr, dst_ptr + at[k], L.FMT_I420, sizing[1] if sizing[0] == "scale" else 0)
    ow, oh = sizing[1] if sizing[0] == "size" else (0, 0)
    assert fn(jobs, len(JOBS), ow, oh, M.LAYOUTS[layout], std) == 0
    return [(at[k], expect_rgb(case, sizing, layout, s)) for k, (_, s) in enumerate(JOBS)]


def slot_bytes(case, sizing):
    y = delivered_planes(case, sizing)[0]
    return (SC.GUARD + 4 + 3 * y.size + SC.GUARD + 3) & ~3


def check_table(got, placed, what):
    mask = np.ones(got.size, dtype=bool)
    for at, exp in placed:
        assert np.array_equal(got[at:at + exp.size], exp), (what, np.flatnonzero(got[at:at + exp.size] != exp)[:8])
        mask[at:at + exp.size] = False
    assert np.all(got[mask] == 0xa5), what


@pytest.mark.parametrize("layout", ["rgb24", "rgbp"])
def test_rgb_pack_on_the_host(layout):
    """every directed window under every sizing: destination offsets 0..3 from a 4-byte boundary, the four standards side by side in
    one table; the bytes are the model's and the 0xA5 around every destination is intact.  Rows of 3*ow bytes with 3*ow mod 4 in 0 and
    2, pictures of 2 to 34 rows (one band, a band and a pair, two bands and a pair), both clips in all three channels"""
    L, lib = _lib()
    rows, heights, clips = set(), set(), set()
    for name, case, sizings in directed():
        for sizing in sizings:
            slot = slot_bytes(case, sizing)
            buf = np.full(slot * len(JOBS) + 8, 0xa5, dtype=np.uint8)
            base = (-buf.ctypes.data) % 4
            placed = run_table(L, lib.lh264_debug_rgb_cpu, case, sizing, layout, case.buf.ctypes.data, buf.ctypes.data + base, slot)
            check_table(buf[base:], placed, (name, sizing, layout))
            oh, ow = delivered_planes(case, sizing)[0].shape
            rows.add(3 * ow % 4)
            heights.add(oh)
            for _, exp in placed:
                clips |= {(c, v) for c in range(3) for v in (0, 255) if np.any((exp.reshape(-1, 3)[:, c] if layout == "rgb24" else exp.reshape(3, -1)[c]) == v)}
    assert rows == {0, 2} and {2, 6, 16, 18, 34} <= heights and len(clips) == 6


def test_the_debug_entry_points_check_their_arguments():
    """a layout, a standard byte, a size, a scale or a format that is not defined, a NULL table and n <= 0 are LH264_E_ARG from both
    entry points and nothing is written; lh264_debug_rgb_dev without a device is LH264_E_NODEVICE"""
    L, lib = _lib()
    case = SC.Case(16, 16, 0, 0)
    buf = np.full(4096, 0xa5, dtype=np.uint8)
    j = L.PackJob()
    case.fill_job(j, case.buf.ctypes.data, buf.ctypes.data + 64, L.FMT_I420, 0)
    std = (C.c_uint8 * 1)(0)
    for fn in (lib.lh264_debug_rgb_cpu, lib.lh264_debug_rgb_dev):
        for layout in (0, 3, -1):
            assert fn(C.byref(j), 1, 0, 0, layout, std) == L.E_ARG, layout
        for bad in ((16, 0), (0, 16), (15, 16), (16, 15), (4098, 16), (-2, 16), (1, 1)):
            assert fn(C.byref(j), 1, bad[0], bad[1], 1, std) == L.E_ARG, bad
        assert fn(None, 1, 0, 0, 1, std) == L.E_ARG and fn(C.byref(j), 0, 0, 0, 1, std) == L.E_ARG and fn(C.byref(j), 1, 0, 0, 1, None) == L.E_ARG
        for s in (4, 255):
            std[0] = s
            assert fn(C.byref(j), 1, 0, 0, 1, std) == L.E_ARG, s
        std[0] = 0
        j.reserved = 4
        assert fn(C.byref(j), 1, 0, 0, 1, std) == L.E_ARG
        j.reserved = 1
        assert fn(C.byref(j), 1, 16, 16, 1, std) == L.E_ARG          # a size and a scale
        j.reserved, j.format = 0, L.FMT_NV12
        assert fn(C.byref(j), 1, 0, 0, 1, std) == L.E_ARG
        j.format, j.crop_w = L.FMT_I420, 15
        assert fn(C.byref(j), 1, 0, 0, 1, std) == L.E_ARG
        j.crop_w = 16
    assert np.all(buf == 0xa5)
    import torch
    if not torch.cuda.is_available():
        assert lib.lh264_debug_rgb_dev(C.byref(j), 1, 0, 0, 1, std) == L.E_NODEVICE
        assert np.all(buf == 0xa5)


# ---- the struct and the arguments of the call ---------------------------------------------------------------------------------------------
def test_layout_of_the_ext_struct():
    """sizeof 24 with struct_bytes, colour, matrix, range, reserved0, reserved1 at 0, 4, .., 20, by a C compiler and in the mirror; the
    values of the constants; the frozen options struct is still 88 bytes and the ABI version 3"""
    L, lib = _lib()
    E = L.DecodeExt
    names = ["struct_bytes", "colour", "matrix", "range", "reserved0", "reserved1"]
    assert C.sizeof(E) == 24 and [getattr(E, n).offset for n in names] == [0, 4, 8, 12, 16, 20]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lh264.h"\nint main(void){ printf("%zu %zu ", sizeof(lh264_decode_ext_t), sizeof(lh264_decode_opts_t));\n' + \
          "".join('printf("%%zu ", offsetof(lh264_decode_ext_t, %s));\n' % n for n in names) + \
          'printf("%u %u %u %u %u %u %u %u %u %d\\n", LH264_COLOUR_YUV, LH264_COLOUR_RGB24, LH264_COLOUR_RGBP, LH264_MATRIX_AUTO, LH264_MATRIX_BT601, LH264_MATRIX_BT709, ' \
          'LH264_RANGE_AUTO, LH264_RANGE_LIMITED, LH264_RANGE_FULL, LH264_ABI_VERSION); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    assert out == ["24", "88", "0", "4", "8", "12", "16", "20", "0", "1", "2", "0", "1", "2", "0", "1", "2", "3"]
    assert (L.COLOUR, L.MATRIX, L.RANGE) == ({None: 0, "rgb24": 1, "rgbp": 2}, {"auto": 0, "bt601": 1, "bt709": 2}, {"auto": 0, "limited": 1, "full": 2})
    assert lib.lh264_abi_version() == 3


def test_arguments_are_checked_before_the_device():
    """every LH264_E_ARG case of the ext struct is reported on a machine without a device and leaves `out` alone; ext == NULL and
    colour == 0 are accepted exactly as lh264_decode_batch is, and so is every valid colour, with and without options"""
    L, lib = _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    ptrs, lens = (C.c_char_p * 1)(data), (C.c_size_t * 1)(len(data))
    outs = (C.c_void_p * 1)()
    sentinel = 0x4321

    def call(o, e):
        outs[0] = sentinel
        rc = lib.lh264_decode_batch_ex(ptrs, lens, 1, 1, C.byref(o) if o is not None else None, C.byref(e) if e is not None else None, outs)
        if rc == 0:
            lib.lh264_decoded_free(outs[0])
        else:
            assert outs[0] == sentinel
        return rc
    import torch
    accepted = 0 if torch.cuda.is_available() else L.E_NODEVICE
    o = L.DecodeOptsV6()
    o.struct_bytes = 88

    def ext(**kw):
        e = L.DecodeExt()
        e.struct_bytes = 24
        for k, v in kw.items():
            setattr(e, k, v)
        return e
    for opts in (None, o):
        assert call(opts, None) == accepted
        assert call(opts, ext()) == accepted
        for colour in (1, 2):
            for matrix in (0, 1, 2):
                for rng in (0, 1, 2):
                    assert call(opts, ext(colour=colour, matrix=matrix, range=rng)) == accepted, (colour, matrix, rng)
        for nbytes in (0, 4, 16, 20, 23, 25, 28, 32, 88):
            assert call(opts, ext(struct_bytes=nbytes)) == L.E_ARG, nbytes
            assert call(opts, ext(struct_bytes=nbytes, colour=1)) == L.E_ARG, nbytes
        for bad in (dict(colour=3), dict(colour=0xffffffff), dict(colour=1, matrix=3), dict(colour=1, range=3), dict(colour=2, matrix=0x80000000),
                    dict(reserved0=1), dict(reserved1=1), dict(colour=1, reserved0=0xffffffff), dict(colour=2, reserved1=7),
                    dict(matrix=1), dict(matrix=2), dict(range=1), dict(range=2), dict(matrix=1, range=2)):
            assert call(opts, ext(**bad)) == L.E_ARG, bad
    o.format = L.FMT_NV12
    assert call(o, ext(colour=1)) == L.E_ARG and call(o, ext(colour=2, matrix=1)) == L.E_ARG
    assert call(o, ext()) == accepted and call(o, None) == accepted          # NV12 without colour: as ever
    o.format = L.FMT_I420
    # the options' own rules hold beside a colour, and everything they allow goes with one
    o.reserved4 = 1
    assert call(o, ext(colour=1)) == L.E_ARG
    o.reserved4 = 0
    o.flags = 2
    assert call(o, ext(colour=1)) == L.E_ARG
    o.flags = L.DECODE_SHA1_PICTURES | L.DECODE_SHA1_STREAM | L.DECODE_NO_PICTURES
    o.out_width, o.out_height, o.parse, o.parse_flags, o.pick = 224, 224, 1, L.PARSE_FLAG_CABAC, 2
    assert call(o, ext(colour=2, range=2)) == accepted
    o.out_width = o.out_height = o.pick = 0
    o.scale_log2, o.conceal, o.flags = 3, L.CONCEAL["slice_copy"], L.DECODE_DEVICE_OUT
    assert call(o, ext(colour=1, matrix=2)) == accepted
    for nbytes in (72, 64, 56, 48, 40):
        o.struct_bytes = nbytes
        assert call(o, ext(colour=1)) == accepted, nbytes
    # the handle calls take a bad handle
    m, f = C.c_uint32(9), C.c_int32(9)
    assert lib.lh264_decoded_picture_colour(None, 0, C.byref(m), C.byref(f)) == L.E_ARG and (m.value, f.value) == (9, 9)


def test_python_refuses_bad_colour_keywords():
    import losslessh264_amd as lh
    _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    for kw in (dict(colour="rgb"), dict(colour="bgr24"), dict(colour=1), dict(colour=True), dict(colour="rgb24", matrix="bt2020"), dict(colour="rgb24", matrix=None),
               dict(colour="rgbp", colour_range="tv"), dict(matrix="bt709"), dict(colour_range="full"), dict(colour="rgb24", fmt="nv12")):
        with pytest.raises(ValueError):
            lh.decode_batch([data], **kw)
    b = lh.DecodedBatch(None, [], True, None, (224, 224))
    with pytest.raises(RuntimeError):
        b.colours(0)                                 # no colour


# ---- what a stream says about colour ------------------------------------------------------------------------------------------------------
def _bits(data):
    return "".join("{:08b}".format(x) for x in data)


def unescape(nal):
    out = bytearray()
    zeros = 0
    for x in nal:
        if zeros >= 2 and x == 3:
            zeros = 0
            continue
        out.append(x)
        zeros = zeros + 1 if x == 0 else 0
    return bytes(out)


def with_vui(data, vui):
    """the stream with the VUI of its first SPS replaced: vui = None (no VUI) or the bit string that follows
    vui_parameters_present_flag = 1.  The SPS must end in that flag (nothing of a VUI behind it that this does not replace)"""
    at = data.index(b"\x00\x00\x01\x67") + 3
    end = min(x for x in (data.find(b"\x00\x00\x01", at), data.find(b"\x00\x00\x00", at), len(data)) if x >= 0)
    rbsp = _bits(unescape(data[at + 1:end]))
    body = rbsp[:rbsp.rindex("1")]                    # without the stop bit and the alignment
    assert body.endswith("0")                         # vui_parameters_present_flag of the stream as committed
    body = body[:-1] + ("0" if vui is None else "1" + vui) + "1"
    body += "0" * (-len(body) % 8)
    payload = bytes(int(body[k:k + 8], 2) for k in range(0, len(body), 8))
    return data[:at + 1] + h264_synth.escape(payload)[0] + data[end:]


def vui(aspect="0", overscan="0", signal="0"):
    """a whole VUI: the three parts the front end reads, then chroma_loc_info, timing_info, both HRDs, pic_struct and
    bitstream_restriction absent"""
    return aspect + overscan + signal + "000000"


def signal(full, matrix=None):
    """video_signal_type_present_flag, video_format 5, video_full_range_flag, and a colour description (primaries 2, transfer 2) or none"""
    return "1" + "101" + str(int(full)) + ("0" if matrix is None else "1" + "{:08b}{:08b}{:08b}".format(2, 2, matrix))


EXT_SAR = "1" + "{:08b}{:016b}{:016b}".format(255, 0x0100, 0x0003)      # (bytes the escaping has to work on)
COLOUR_STREAMS = [
    ("no VUI", None, (2, False, 0)),
    ("a VUI without a signal type", vui(), (2, False, 0)),
    ("a signal type without a colour description", vui(signal=signal(0)), (2, False, 1)),
    ("full range, no colour description", vui(signal=signal(1)), (2, True, 1)),
    ("BT.709", vui(signal=signal(0, 1)), (1, False, 3)),
    ("unspecified", vui(signal=signal(0, 2)), (2, False, 3)),
    ("BT.470BG", vui(signal=signal(0, 5)), (5, False, 3)),
    ("SMPTE 170M, full range", vui(signal=signal(1, 6)), (6, True, 3)),
    ("BT.2020", vui(signal=signal(0, 9)), (9, False, 3)),
    ("BT.709 full range behind an extended SAR and overscan", vui(aspect=EXT_SAR, overscan="11", signal=signal(1, 1)), (1, True, 3)),
    ("a plain SAR", vui(aspect="1" + "{:08b}".format(1), signal=signal(0, 6)), (6, False, 3)),
]


def colour_stream(name, src="BA_MW_D.264"):
    data = open(os.path.join(STREAMS, src), "rb").read()
    for n, v, _ in COLOUR_STREAMS:
        if n == name:
            return with_vui(data, v)
    raise KeyError(name)


def test_what_the_first_sps_says():
    """lh264_parser_colour on BA_MW_D.264 with its SPS rewritten: no VUI, a VUI without a signal type, matrix_coefficients 1, 2, 5, 6
    and 9, full range on and off, an extended SAR in front; and on the streams as committed"""
    import losslessh264_amd as lh
    L, lib = _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    assert with_vui(data, None) == data                                    # the rewrite of nothing is the stream
    for name, v, want in COLOUR_STREAMS:
        assert lh.stream_colour(with_vui(data, v)) == want, name
    assert lh.stream_colour(data) == (2, False, 0)
    assert lh.stream_colour(open(os.path.join(STREAMS, "test_qcif_cabac.264"), "rb").read()) is not None
    assert lh.stream_colour(b"") is None and lh.stream_colour(b"\x00\x00\x01\x68\xce\x38\x80") is None
    assert lh.stream_colour(data[:8]) is None                              # an SPS cut short is no SPS
    mc = C.c_int32(7)
    assert lib.lh264_parser_colour(None, 0, C.byref(mc), None, None) == L.E_ARG and mc.value == 7
    assert lib.lh264_parser_colour(data, len(data), None, None, None) == 0
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lh264.h")).read(), flags=re.S)
    for name in ("lh264_decode_batch_ex", "lh264_decoded_picture_colour", "lh264_parser_colour", "lh264_debug_rgb_cpu", "lh264_debug_rgb_dev"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name) and name in L.EXPORTS, name


def test_the_walk_only_reads():
    """a stream with a VUI parses to the records, symbols and default stream of the stream without one - the default stream apart from
    the SPS payload it keeps -, so what the coder makes of it is the same"""
    import losslessh264_amd as lh
    _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    frames0, err0, main0 = lh.parse_file(data)
    assert err0 == "" and len(frames0) == 100
    for name in ("BT.709 full range behind an extended SAR and overscan", "BT.2020"):
        new = colour_stream(name)
        frames, err, main = lh.parse_file(new)
        assert err == "" and len(frames) == len(frames0), name
        for a, b in zip(frames0, frames):
            for field in ("mbs", "coeffs", "levels", "slices", "covered", "syn", "slice_syn", "syn_syms", "syn_off"):
                assert np.array_equal(getattr(a, field), getattr(b, field)), (name, field)
            assert (a.mb_w, a.mb_h, a.crop_x, a.crop_y, a.crop_w, a.crop_h, a.frame_num, a.idr, a.ref_ids) == (b.mb_w, b.mb_h, b.crop_x, b.crop_y, b.crop_w, b.crop_h, b.frame_num, b.idr, b.ref_ids)
        grown = len(new) - len(data)
        assert grown > 0 and len(main) - len(main0) == grown, name
        end = data.index(b"\x00\x00\x00\x01\x68")      # where the SPS ends, in the stream and in its default stream alike
        assert main0[:end] == data[:end] and main[:end + grown] == new[:end + grown] and main0[end:] == main[end + grown:], name


# ---- the command lines --------------------------------------------------------------------------------------------------------------------
def test_the_command_lines_refuse_bad_colour_options(tmp_path):
    """--rgb takes rgb24 | rgbp and no --nv12 beside it, --matrix and --range take their names and need --rgb: anything else ends both
    command lines with the usage code before a stream is read or a device looked for"""
    src = os.path.join(STREAMS, "BA_MW_D.264")
    _lib()
    bad = [["--rgb", v] for v in ("rgb", "bgr24", "RGB24", "1", "")] + [["--rgb", "rgb24", "--nv12"], ["--nv12", "--rgb", "rgbp"],
           ["--rgb", "rgb24", "--matrix", "bt2020"], ["--rgb", "rgb24", "--range", "tv"], ["--matrix", "bt709"], ["--range", "full"],
           ["--matrix", "auto"], ["--rgb", "rgbp", "--matrix", ""]]
    for cmd in ([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"]):
        for args in bad:
            r = subprocess.run(cmd + ["--decode"] + args + [str(tmp_path), src], capture_output=True, timeout=120, cwd=ROOT)
            assert r.returncode == 2 and b"--rgb: rgb24 | rgbp" in r.stdout + r.stderr, (cmd, args, r.stdout, r.stderr)
            assert os.listdir(str(tmp_path)) == []
