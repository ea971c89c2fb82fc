"""Pictures of one given size (lh264_decode_batch, out_width x out_height) where no device is present: the code of
decode_pack_resized_kernel stepped on the host (lh264_debug_resize_cpu) over synthetic padded pictures, against the definition in numpy
(tests/resize_ref.py); the definition's own properties; the layout of the 88-byte options struct and the arguments of the call."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import resize_ref
import scale_cases as SC
import scale_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")

# (w, h, crop_x, crop_y)
WINDOWS = [(2, 2, 0, 0), (4, 2, 0, 0), (6, 10, 0, 0), (18, 14, 0, 0), (30, 34, 0, 0), (62, 46, 6, 2), (176, 144, 0, 0), (300, 168, 26, 60)]
CONTENTS = ["random", 0, 255, "checker"]


def targets(w, h):
    """the sizes a w x h window is resampled to: the smallest, its own, a little more, twice, half where that is even, and sizes in no
    simple ratio to it"""
    t = [(2, 2), (w, h), (w + 2, h + 2), (2 * w, 2 * h)]
    if w % 4 == 0 and h % 4 == 0:
        t.append((w // 2, h // 2))
    for s in ((10, 6), (22, 18), (46, 38), (224, 224)):
        t.append(s)
    return sorted(set(t))


def expect(case, size, fmt):
    """the packed picture the definition gives for a scale_cases.Case (computed once per case, size and format)"""
    memo = case.__dict__.setdefault("_resized", {})
    if size not in memo:
        memo[size] = resize_ref.resize_planes(case.Y, case.U, case.V, size)
    return np.frombuffer(scale_ref.pack(*memo[size], fmt), dtype=np.uint8)


def _lib():
    import __graft_entry__ as g
    g.build()
    from losslessh264_amd import _lib as L
    return L, L.lib()


def _run_offsets(L, lib, case, size, fmt, offsets):
    """one lh264_debug_resize_cpu call with a job per destination offset from a 16-byte boundary, each in 0xA5 guard bytes of its own
    -> the delivered bytes are the definition's and every guard byte is intact"""
    exp = expect(case, size, fmt)
    assert exp.size == size[0] * size[1] * 3 // 2
    slot = (SC.GUARD + 16 + exp.size + SC.GUARD + 15) & ~15
    buf = np.full(slot * len(offsets) + 32, 0xa5, dtype=np.uint8)
    base = (-buf.ctypes.data) % 16
    jobs = (L.PackJob * len(offsets))()
    at = []
    for k, off in enumerate(offsets):
        at.append(base + k * slot + SC.GUARD + off)
        case.fill_job(jobs[k], case.buf.ctypes.data, buf.ctypes.data + at[k], fmt, 0)
        assert (jobs[k].dst - off) % 16 == 0
    assert lib.lh264_debug_resize_cpu(jobs, len(offsets), size[0], size[1]) == 0
    mask = np.ones(buf.size, dtype=bool)
    for k, off in enumerate(offsets):
        got = buf[at[k]:at[k] + exp.size]
        assert np.array_equal(got, exp), (case.crop, size, fmt, off, np.flatnonzero(got != exp)[:8])
        mask[at[k]:at[k] + exp.size] = False
    assert np.all(buf[mask] == 0xa5), (case.crop, size, fmt)
    return buf[at[0]:at[0] + exp.size]


def test_reference_examples():
    """the definition on numbers small enough to do by hand, and its weights"""
    assert resize_ref.weights(3, 2).tolist() == [[2, 1, 0], [0, 1, 2]]           # 3 -> 2: the middle sample is shared
    assert resize_ref.weights(2, 4).tolist() == [[2, 0], [2, 0], [0, 2], [0, 2]]   # 2 -> 4: every sample twice
    assert resize_ref.weights(2, 3).tolist() == [[2, 0], [1, 1], [0, 2]]           # 2 -> 3: a blended seam
    p = np.array([[0, 90, 255]], dtype=np.uint8)
    assert resize_ref.resize_plane(p, 2, 1).tolist() == [[30, 200]]                # (0*2 + 90) / 3 = 30; (90 + 510) / 3 = 200
    p = np.array([[0, 255], [255, 255]], dtype=np.uint8)
    assert resize_ref.resize_plane(p, 1, 1).tolist() == [[191]]                    # 765 / 4 = 191.25
    p = np.array([[0, 255], [0, 255]], dtype=np.uint8)
    assert resize_ref.resize_plane(p, 1, 1).tolist() == [[128]]                    # 127.5: half goes up
    assert resize_ref.resize_plane(p, 3, 2).tolist() == [[0, 128, 255], [0, 128, 255]]


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d@%d,%d" % w)
def test_resized_pack_on_the_host(window):
    """every listed window to every target, every content, both formats, the destination at every offset 0..15 from a 16-byte
    boundary: the delivered bytes are the definition's and the guard bytes around every destination are intact.  All 0 and all 255
    deliver 0 and 255 (the weights of a sample sum to D exactly)"""
    L, lib = _lib()
    w, h = window[:2]
    sizes = targets(w, h)
    assert len(sizes) >= 6 and (2, 2) in sizes and (w, h) in sizes and (w + 2, h + 2) in sizes and (224, 224) in sizes and (2 * w, 2 * h) in sizes
    for content in CONTENTS:
        case = SC.Case(*window, seed=7 * w + h, content=content)
        for size in sizes:
            for fmt in (L.FMT_I420, L.FMT_NV12):
                got = _run_offsets(L, lib, case, size, fmt, range(16))
                if content in (0, 255):
                    assert np.all(got == content), (window, size, content)


@pytest.mark.parametrize("value", [1, 127, 128, 254])
def test_a_flat_plane_keeps_its_value(value):
    """(2*v*D + D) / (2*D) = v + 1/2 exactly: a quotient estimated one too high or too low shows here, at sizes in no simple ratio"""
    L, lib = _lib()
    case = SC.Case(62, 46, 6, 2, content=value)
    for size in ((46, 38), (10, 6), (224, 224), (64, 48)):
        got = _run_offsets(L, lib, case, size, L.FMT_I420, (0, 3))
        assert np.all(got == value), (value, size)


def test_own_size_is_the_window():
    """ow == w and oh == h delivers the window itself - by identity, not by the reference"""
    L, lib = _lib()
    for window in WINDOWS:
        case = SC.Case(*window, seed=3)
        for fmt in (L.FMT_I420, L.FMT_NV12):
            want = np.frombuffer(scale_ref.pack(case.Y, case.U, case.V, fmt), dtype=np.uint8)
            assert np.array_equal(expect(case, window[:2], fmt), want)
            assert np.array_equal(_run_offsets(L, lib, case, window[:2], fmt, (0, 5)), want), window


@pytest.mark.parametrize("s", [1, 2, 3])
def test_power_of_two_ratios_are_the_scale_means(s):
    """w = B*ow and h = B*oh, B = 2, 4, 8: exactly the scale_log2 mean of tests/scale_ref.py - QCIF at 88 x 72, 44 x 36 and 22 x 18 is
    byte for byte scale 1, 2, 3; so is a 32 x 48 window inside a larger picture"""
    L, lib = _lib()
    B = 1 << s
    for window in ((176, 144, 0, 0), (32, 48, 6, 2)):
        w, h = window[:2]
        case = SC.Case(*window, seed=11 + s)
        size = (w // B, h // B)
        assert scale_ref.scaled_size(w, h, s) == size
        for fmt in (L.FMT_I420, L.FMT_NV12):
            want = case.expect(s, fmt)
            assert np.array_equal(expect(case, size, fmt), want)
            assert np.array_equal(_run_offsets(L, lib, case, size, fmt, (0, 1)), want), (window, s)
    assert (176 // B, 144 // B) == {1: (88, 72), 2: (44, 36), 3: (22, 18)}[s]


def test_twice_the_size_repeats_every_sample():
    """ow = 2w and oh = 2h: every sample twice each way, no blending"""
    L, lib = _lib()
    for window in ((18, 14, 0, 0), (62, 46, 6, 2)):
        w, h = window[:2]
        case = SC.Case(*window, seed=21)
        twice = [np.repeat(np.repeat(p, 2, axis=0), 2, axis=1) for p in (case.Y, case.U, case.V)]
        for fmt in (L.FMT_I420, L.FMT_NV12):
            want = np.frombuffer(scale_ref.pack(*twice, fmt), dtype=np.uint8)
            assert np.array_equal(expect(case, (2 * w, 2 * h), fmt), want)
            assert np.array_equal(_run_offsets(L, lib, case, (2 * w, 2 * h), fmt, (0, 6)), want), window


def test_a_large_window():
    """4096 x 2304 to 64 x 36: 2*S + D passes 2^32 (D = 9.4 M samples), the smallest case in which a 32-bit sum goes wrong.  All 255
    delivers 255 everywhere; random samples deliver the definition's bytes"""
    L, lib = _lib()
    assert 2 * 255 * 4096 * 2304 + 4096 * 2304 >= 1 << 32
    for content in (255, "random"):
        case = SC.Case(4096, 2304, 0, 0, seed=5, content=content, pic_w=4096, pic_h=2304)
        got = _run_offsets(L, lib, case, (64, 36), L.FMT_I420, (0,))
        if content == 255:
            assert np.all(got == 255)


def test_two_jobs_back_to_back():
    """two jobs in one call: the second picture starts where the first ended (tight: 10 x 6 pictures are 90 bytes, 2 mod 4)"""
    L, lib = _lib()
    a, b = SC.Case(18, 14, 0, 0, seed=5), SC.Case(62, 46, 6, 2, seed=6)
    for fmt in (L.FMT_I420, L.FMT_NV12):
        ea, eb = expect(a, (10, 6), fmt), expect(b, (10, 6), fmt)
        buf = np.full(ea.size + eb.size + 2 * SC.GUARD + 64, 0xa5, dtype=np.uint8)
        at = (-buf.ctypes.data) % 16 + SC.GUARD
        jobs = (L.PackJob * 2)()
        a.fill_job(jobs[0], a.buf.ctypes.data, buf.ctypes.data + at, fmt, 0)
        b.fill_job(jobs[1], b.buf.ctypes.data, buf.ctypes.data + at + ea.size, fmt, 0)
        assert lib.lh264_debug_resize_cpu(jobs, 2, 10, 6) == 0
        assert np.array_equal(buf[at:at + ea.size + eb.size], np.concatenate([ea, eb]))
        assert np.all(buf[:at] == 0xa5) and np.all(buf[at + ea.size + eb.size:] == 0xa5)


def test_layout_of_the_options_struct():
    """sizeof 88, out_width at 72, out_height at 76, reserved4 at 80, reserved5 at 84; the 72-byte struct is still there and named V5;
    the header carries the fields in that order behind reserved3, and the new entry points"""
    L, lib = _lib()
    V6 = L.DecodeOptsV6
    assert C.sizeof(V6) == 88 and (V6.out_width.offset, V6.out_height.offset, V6.reserved4.offset, V6.reserved5.offset) == (72, 76, 80, 84)
    assert C.sizeof(L.DecodeOptsV5) == 72 and L.DECODE_OPTS_BYTES_V5 == 72
    assert [f[0] for f in V6._fields_[:len(L.DecodeOptsV5._fields_)]] == [f[0] for f in L.DecodeOptsV5._fields_]
    txt = open(os.path.join(ROOT, "include", "lh264.h")).read()
    assert re.search(r"uint32_t pick;[^}]*uint32_t reserved3;[^}]*uint32_t out_width, out_height;[^}]*uint32_t reserved4, reserved5;[^}]*\} lh264_decode_opts_t;", txt, flags=re.S)
    assert re.search(r"#define LH264_DECODE_OPTS_BYTES_V5 72u", txt)
    for decl in ("int lh264_debug_resize_cpu (const lh264_pack_job_t* jobs, int n, int out_w, int out_h);",
                 "int lh264_debug_resize_dev (const lh264_pack_job_t* jobs, int n, int out_w, int out_h);"):
        assert decl in txt, decl
    # ... and a C compiler agrees with the mirror
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lh264.h"\nint main(void){ printf("%zu %zu %zu %zu %zu\\n", sizeof(lh264_decode_opts_t), ' \
          'offsetof(lh264_decode_opts_t, out_width), offsetof(lh264_decode_opts_t, out_height), offsetof(lh264_decode_opts_t, reserved4), offsetof(lh264_decode_opts_t, reserved5)); return 0; }\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        assert subprocess.check_output([os.path.join(d, "t")]).decode().split() == ["88", "72", "76", "80", "84"]


def test_arguments_are_checked_before_the_device():
    """every LH264_E_ARG case of the size is reported on a machine without a device (none becomes LH264_E_NODEVICE) and leaves `out`
    alone; a valid size is accepted (LH264_E_NODEVICE where there is no device); the 72-byte struct does not read what lies behind it"""
    L, lib = _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    ptrs, lens = (C.c_char_p * 1)(data), (C.c_size_t * 1)(len(data))
    outs = (C.c_void_p * 1)()
    sentinel = 0x4321

    def call(o):
        outs[0] = sentinel
        rc = lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(o), outs)
        if rc == 0:
            lib.lh264_decoded_free(outs[0])
        else:
            assert outs[0] == sentinel
        return rc
    import torch
    accepted = 0 if torch.cuda.is_available() else L.E_NODEVICE
    o = L.DecodeOptsV6()
    o.struct_bytes = 88
    for bad in ((224, 0), (0, 224), (223, 224), (224, 225), (1, 1), (3, 2), (4098, 2), (2, 4098), (0x80000000, 2), (0xffffffff, 0xffffffff), (0x10000 + 224, 224)):
        o.out_width, o.out_height = bad
        assert call(o) == L.E_ARG, bad
    for size in ((0, 0), (224, 224)):
        o.out_width, o.out_height = size
        for r4, r5 in ((1, 0), (0, 1), (0xffffffff, 0), (0, 0x80000000)):
            o.reserved4, o.reserved5 = r4, r5
            assert call(o) == L.E_ARG, (size, r4, r5)
    o.reserved4 = o.reserved5 = 0
    for s in (1, 2, 3):
        o.out_width, o.out_height, o.scale_log2 = 224, 224, s
        assert call(o) == L.E_ARG, s
        o.out_width, o.out_height = 0, 0          # the scale alone: as ever
        assert call(o) == accepted, s
    o.scale_log2 = 0
    o.out_width, o.out_height, o.reserved3 = 224, 224, 1      # the 72-byte struct's rule holds in the 88-byte struct
    assert call(o) == L.E_ARG
    o.reserved3 = 0
    for size in ((0, 0), (2, 2), (224, 224), (4096, 4096), (2, 4096), (398, 224)):
        o.out_width, o.out_height = size
        assert call(o) == accepted, size
    # with every format, digest flag, conceal, parse and pick value
    o.out_width, o.out_height = 224, 224
    o.format, o.flags, o.parse, o.parse_flags, o.pick = L.FMT_NV12, L.DECODE_SHA1_PICTURES | L.DECODE_SHA1_STREAM | L.DECODE_NO_PICTURES, 1, L.PARSE_FLAG_CABAC, 2
    assert call(o) == accepted
    o.pick, o.conceal, o.flags = 0, L.CONCEAL["slice_copy"], L.DECODE_DEVICE_OUT
    assert call(o) == accepted
    o.format = o.flags = o.parse = o.parse_flags = o.conceal = 0
    # struct_bytes 72 (and 64, 56, 48, 40) with garbage behind: accepted, the new words are not read
    o.out_width, o.out_height, o.reserved4, o.reserved5 = 0xdeadbeef, 3, 0xdeadbeef, 0xdeadbeef
    for nbytes in (72, 64, 56, 48, 40):
        o.struct_bytes = nbytes
        assert call(o) == accepted, nbytes
    o.struct_bytes, o.scale_log2 = 72, 2
    assert call(o) == accepted                        # (the size is not read there: no clash with the scale)
    o.scale_log2 = 0
    for nbytes in (0, 44, 68, 76, 80, 84, 92, 96):
        o.struct_bytes, o.out_width, o.out_height, o.reserved4, o.reserved5 = nbytes, 0, 0, 0, 0
        assert call(o) == L.E_ARG, nbytes


def test_the_debug_entry_points_check_their_arguments():
    """a bad size, a job with reserved != 0, a NULL table and n <= 0 are LH264_E_ARG from both entry points, and nothing is written;
    lh264_debug_resize_dev without a device is LH264_E_NODEVICE"""
    L, lib = _lib()
    case = SC.Case(16, 16, 0, 0)
    buf = np.full(4096, 0xa5, dtype=np.uint8)
    j = L.PackJob()
    case.fill_job(j, case.buf.ctypes.data, buf.ctypes.data + 64, L.FMT_I420, 0)
    for fn in (lib.lh264_debug_resize_cpu, lib.lh264_debug_resize_dev):
        for bad in ((0, 0), (16, 0), (0, 16), (15, 16), (16, 15), (4098, 16), (16, 4098), (-2, 16), (1, 1)):
            assert fn(C.byref(j), 1, bad[0], bad[1]) == L.E_ARG, bad
        assert fn(None, 1, 16, 16) == L.E_ARG and fn(C.byref(j), 0, 16, 16) == L.E_ARG and fn(C.byref(j), -1, 16, 16) == L.E_ARG
        for reserved in (1, 2, 3, -1):
            j.reserved = reserved
            assert fn(C.byref(j), 1, 16, 16) == L.E_ARG, reserved
        j.reserved = 0
        j.crop_w = 15
        assert fn(C.byref(j), 1, 16, 16) == L.E_ARG
        j.crop_w = 16
    assert np.all(buf == 0xa5)
    import torch
    if not torch.cuda.is_available():
        assert lib.lh264_debug_resize_dev(C.byref(j), 1, 16, 16) == L.E_NODEVICE
        assert np.all(buf == 0xa5)


def test_python_refuses_a_bad_size():
    import losslessh264_amd as lh
    _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    for bad in ((224, 0), (0, 0), (223, 224), (224, 4098), (224,), (224, 224, 3), 224, "224x224", (224.0, 224), (True, 2), (-2, 2), ("224", "224")):
        with pytest.raises(ValueError):
            lh.decode_batch([data], size=bad)
    for s in (1, 2, 3):
        with pytest.raises(ValueError):
            lh.decode_batch([data], size=(224, 224), scale=s)
    b = lh.DecodedBatch(None, [], True)
    with pytest.raises(RuntimeError):
        b.frames(0)                                  # no size
    b = lh.DecodedBatch(None, [], False, None, (224, 224))
    with pytest.raises(RuntimeError):
        b.frames(0)                                  # not device_out


def test_the_command_lines_refuse_a_bad_size(tmp_path):
    """--size takes WxH, both even, 2..4096, and no non-zero --scale beside it: anything else ends both command lines with the usage
    code before a stream is read or a device looked for"""
    src = os.path.join(STREAMS, "BA_MW_D.264")
    _lib()
    bad = [["--size", v] for v in ("224", "224x", "x224", "223x224", "224x0", "0x0", "4098x2", "224x224x2", "-2x2", "2 x2", "99999x2", "axb")]
    bad += [["--size", "224x224", "--scale", "1"], ["--scale", "3", "--size", "224x224"]]
    for cmd in ([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"]):
        for args in bad:
            r = subprocess.run(cmd + ["--decode"] + args + [str(tmp_path), src], capture_output=True, timeout=120, cwd=ROOT)
            assert r.returncode == 2 and b"--size: WxH" in r.stdout + r.stderr, (cmd, args, r.stdout, r.stderr)
            assert os.listdir(str(tmp_path)) == []
