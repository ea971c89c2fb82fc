"""Reduced-size pictures (lh264_decode_batch, scale_log2 1..3) where no device is present: the code of decode_pack_scaled_kernel stepped
on the host (lh264_debug_pack_cpu with the job's `reserved` word = scale_log2) over synthetic padded pictures, against the definition
in numpy (tests/scale_ref.py); the arguments of the call."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scale_cases as SC
import scale_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")


def _lib():
    import __graft_entry__ as g
    g.build()
    from losslessh264_amd import _lib as L
    return L, L.lib()


def _dst(n):
    """a buffer of 0xA5 and the index of a 16-byte boundary in it with GUARD + 16 bytes in front and n + GUARD + 16 behind"""
    buf = np.full(n + 2 * SC.GUARD + 64, 0xa5, dtype=np.uint8)
    return buf, (-buf.ctypes.data) % 16 + SC.GUARD


def _run(L, lib, case, s, fmt, off):
    exp = case.expect(s, fmt)
    buf, base = _dst(exp.size)
    at = base + off
    j = L.PackJob()
    case.fill_job(j, case.buf.ctypes.data, buf.ctypes.data + at, fmt, s)
    assert (j.dst - off) % 16 == 0
    assert lib.lh264_debug_pack_cpu(C.byref(j), 1) == 0
    return buf, at, exp


def _check(buf, at, exp, what):
    assert np.array_equal(buf[at:at + exp.size], exp), what
    assert np.all(buf[:at] == 0xa5) and np.all(buf[at + exp.size:] == 0xa5), what     # the guards (and everything else around)


def test_reference_examples():
    """the definition's own examples: QCIF at s = 3 is 22 x 18 and 594 bytes; 1920 x 1080 at s = 3 has 68 chroma rows"""
    assert scale_ref.scaled_size(176, 144, 3) == (22, 18) and 22 * 18 * 3 // 2 == 594
    assert scale_ref.scaled_size(1920, 1080, 3) == (240, 136)
    assert scale_ref.scaled_size(16, 16, 3) == (2, 2) and scale_ref.scaled_size(2, 2, 1) == (2, 2) and scale_ref.scaled_size(176, 144, 0) == (176, 144)
    y = np.arange(16, dtype=np.uint8).reshape(4, 4)
    u = np.array([[10, 20], [30, 41]], dtype=np.uint8)
    Y, U, V = scale_ref.scale_planes(y, u, u, 1)
    assert Y.tolist() == [[3, 5], [11, 13]] and U.tolist() == [[25]] and V.tolist() == [[25]]      # (0+1+4+5+2)>>2 = 3; (101+2)>>2 = 25
    y = np.array([[0, 255], [255, 255]], dtype=np.uint8)
    Y, U, V = scale_ref.scale_planes(y, y[:1, :1], y[:1, :1], 2)      # 2 x 2 at s = 2: the clamped coordinates repeat the last row and column
    assert Y.tolist() == [[(15 * 255 + 8) >> 4, 255], [255, 255]] and U.tolist() == [[0]]


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("window", SC.WINDOWS, ids=lambda w: "%dx%d@%d,%d" % w)
def test_scaled_pack_on_the_host(window, s):
    """every listed window, both formats, the destination at every offset 0..15 from a 16-byte boundary: the delivered bytes are the
    definition's, the 64 guard bytes in front of and behind the destination are intact"""
    L, lib = _lib()
    case = SC.Case(*window, seed=1000 * s + window[0] * 7 + window[1])
    for fmt in (L.FMT_I420, L.FMT_NV12):
        ow, oh = scale_ref.scaled_size(window[0], window[1], s)
        assert case.expect(s, fmt).size == ow * oh * 3 // 2
        for off in range(16):
            buf, at, exp = _run(L, lib, case, s, fmt, off)
            _check(buf, at, exp, (window, s, fmt, off))


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("window", [(16, 16, 0, 0), (18, 14, 0, 0)], ids=lambda w: "%dx%d" % w[:2])
def test_fixed_contents(window, s):
    """all 255 (no overflow: every result 255), all 0, and a 0 / 255 checkerboard: every mean of a block inside the window is 127.5
    and delivers 128, which pins the rounding"""
    L, lib = _lib()
    w, h = window[:2]
    B = 1 << s
    for content in (255, 0, "checker"):
        case = SC.Case(*window, content=content)
        for fmt in (L.FMT_I420, L.FMT_NV12):
            for off in (0, 2, 5):
                buf, at, exp = _run(L, lib, case, s, fmt, off)
                _check(buf, at, exp, (window, s, content, fmt, off))
                got = buf[at:at + exp.size]
                if content != "checker":
                    assert np.all(got == content)
                    continue
                ow, oh = scale_ref.scaled_size(w, h, s)
                Y, U, V = scale_ref.unpack(got.tobytes(), ow, oh, fmt)
                assert np.all(Y[:h // B, :w // B] == 128) and np.all(U[:h // 2 // B, :w // 2 // B] == 128) and np.all(V[:h // 2 // B, :w // 2 // B] == 128)
                if window[:2] == (16, 16):
                    assert np.all(got == 128)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_two_jobs_back_to_back(s):
    """two jobs in one call: the second picture starts where the first ended (tight: 2 mod 4 behind an 18 x 14 picture at s = 1)"""
    L, lib = _lib()
    a, b = SC.Case(18, 14, 0, 0, seed=5), SC.Case(62, 46, 6, 2, seed=6)
    for fmt in (L.FMT_I420, L.FMT_NV12):
        ea, eb = a.expect(s, fmt), b.expect(s, fmt)
        buf, at = _dst(ea.size + eb.size)
        jobs = (L.PackJob * 2)()
        a.fill_job(jobs[0], a.buf.ctypes.data, buf.ctypes.data + at, fmt, s)
        b.fill_job(jobs[1], b.buf.ctypes.data, buf.ctypes.data + at + ea.size, fmt, s)
        assert lib.lh264_debug_pack_cpu(jobs, 2) == 0
        _check(buf, at, np.concatenate([ea, eb]), (s, fmt))


def test_argument_errors():
    """a job's scale above 3 is LH264_E_ARG; the decode call refuses scale_log2 above 3 and a reserved2 that is not 0 in the 64-byte
    struct before a device is looked for, with `out` untouched; the 56-byte struct is accepted as before; the header declares all of it"""
    L, lib = _lib()
    case = SC.Case(16, 16, 0, 0)
    buf, at = _dst(16 * 16 * 3 // 2)
    j = L.PackJob()
    for bad in (4, 5, -1, 1 << 20):
        case.fill_job(j, case.buf.ctypes.data, buf.ctypes.data + at, L.FMT_I420, bad)
        assert lib.lh264_debug_pack_cpu(C.byref(j), 1) == L.E_ARG
        assert np.all(buf == 0xa5)
        assert lib.lh264_debug_pack_dev(C.byref(j), 1) == L.E_ARG
    jobs = (L.PackJob * 2)()
    case.fill_job(jobs[0], case.buf.ctypes.data, buf.ctypes.data + at, L.FMT_I420, 1)
    case.fill_job(jobs[1], case.buf.ctypes.data, buf.ctypes.data + at, L.FMT_I420, 2)
    assert lib.lh264_debug_pack_dev(jobs, 2) == L.E_ARG          # the jobs of a launch share one scale
    assert lib.lh264_debug_pack_dev(None, 1) == L.E_ARG

    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    sentinel = 0x5a5a5a5a
    ptrs, lens, outs = (C.c_char_p * 1)(data), (C.c_size_t * 1)(len(data)), (C.c_void_p * 1)(sentinel)

    def call(o):
        outs[0] = sentinel
        rc = lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(o), outs)
        if rc == 0:
            lib.lh264_decoded_free(outs[0])
        else:
            assert outs[0] == sentinel
        return rc
    assert C.sizeof(L.DecodeOptsV4) == 64 and L.DecodeOptsV4.scale_log2.offset == 56 and L.DecodeOptsV4.reserved2.offset == 60 and L.DECODE_OPTS_BYTES_V3 == 56
    o = L.DecodeOptsV4()
    o.struct_bytes = 64
    for bad in (4, 5, 0x80000000, 0xffffffff):
        o.scale_log2, o.reserved2 = bad, 0
        assert call(o) == L.E_ARG
    o.scale_log2, o.reserved2 = 0, 1
    assert call(o) == L.E_ARG
    o.scale_log2, o.reserved2 = 3, 1
    assert call(o) == L.E_ARG
    import torch
    accepted = 0 if torch.cuda.is_available() else L.E_NODEVICE
    for s in (0, 1, 2, 3):
        o.scale_log2, o.reserved2 = s, 0
        assert call(o) == accepted
    o.struct_bytes, o.scale_log2, o.reserved2 = 56, 4, 1          # the 56-byte struct: accepted as before, the words behind it are not read
    assert call(o) == accepted
    o.struct_bytes = 60
    assert call(o) == L.E_ARG
    import losslessh264_amd as lh
    for bad in (4, -1, "2", None):
        with pytest.raises(ValueError):
            lh.decode_batch([data], scale=bad)
    assert lib.lh264_decoded_picture_source_size(None, 0, None, None) == L.E_ARG

    txt = open(os.path.join(ROOT, "include", "lh264.h")).read()
    assert re.search(r"uint32_t parse_flags;[^}]*uint32_t scale_log2;[^}]*uint32_t reserved2;[^}]*\} lh264_decode_opts_t;", txt, flags=re.S)
    assert re.search(r"#define LH264_DECODE_OPTS_BYTES_V3 56u", txt) and re.search(r"#define LH264_DECODE_OPTS_BYTES_V2 48u", txt)
    assert "int lh264_debug_pack_dev (const lh264_pack_job_t* jobs, int n);" in txt
    assert "int lh264_decoded_picture_source_size (const lh264_decoded_t* d, int idx, int32_t* width, int32_t* height);" in txt


def test_the_command_lines_refuse_a_scale_out_of_range(tmp_path):
    """--scale takes 0..3: anything else ends both command lines with the usage code before a stream is read or a device looked for"""
    src = os.path.join(STREAMS, "BA_MW_D.264")
    _lib()
    for cmd in ([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"]):
        for bad in ("4", "-1", "x"):
            r = subprocess.run(cmd + ["--decode", "--scale", bad, str(tmp_path), src], capture_output=True, timeout=120, cwd=ROOT)
            assert r.returncode == 2 and b"--scale: 0 | 1 | 2 | 3" in r.stdout + r.stderr, (cmd, bad, r.stdout, r.stderr)
            assert os.listdir(str(tmp_path)) == []
