"""Bilinear and bicubic resampling on the device (lh264_decode_batch_ex6): the three filtered production kernels over the jobs of
tests/test_decode_filter.py, byte for byte what the host stepping and the model give, and the call - its views, formats and modes -
against tests/filter_model.py applied to the full-size pictures of the same call made without a size."""
import ctypes as C
import hashlib
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
from test_decode_filter import NAMES, WINDOWS, check, colour_jobs, job_bytes, placed_jobs, plane_jobs, run_jobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK = 0
SIZE = (224, 224)
FIRST = [0, 1, 2, 3]

_cache = {}


def _read(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _res(b, n, data=None):
    """what a call delivered, per stream: (status, text, picture records, bytes, source sizes, picture numbers)"""
    out = [(b.status(i), b.error(i), b.pictures(i), data[i] if data is not None else b.data(i), b.source_sizes(i), b.picture_indices(i)) for i in range(n)]
    b.free()
    return out


def _full(names, fmt="i420", **kw):
    """ONE decode_batch of the named streams without a size per (streams, format, other arguments), shared by the tests"""
    key = (tuple(names), fmt) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _cache:
        import losslessh264_amd as lh
        _cache[key] = _res(lh.decode_batch([_read(n) for n in names], fmt=fmt, **kw), len(names))
    return _cache[key]


def _model(full, fmt, name, i, crop=None, fit="stretch", fill=FM.VM.DEFAULT_FILL):
    return FM.view_packed(full[i][3], full[i][2], fmt, SIZE, name, crop=crop, fit=fit, fill=fill)


# ---- 1: the production kernels over the jobs of the host tests ------------------------------------------------------------------------------
def _launch(groups):
    """every group [(size, filter, jobs)] as one launch of its production kernel: sources in one device tensor of the cases' exact
    bytes, destinations in 0xA5 - the bytes are the model's (which the host stepping gives too) and every guard byte is intact"""
    import torch
    from losslessh264_amd import _lib as L
    lib = L.lib()
    cases = {}
    for _, _, jobs_of in groups:
        for j in jobs_of:
            cases[id(j[0])] = j[0]
    at, offs = 0, {}
    for key, case in cases.items():
        offs[key] = at
        at += (case.buf.size + 255) & ~255
    host = np.zeros(at, dtype=np.uint8)
    for key, case in cases.items():
        host[offs[key]:offs[key] + case.buf.size] = case.buf
    src = torch.from_numpy(host).cuda()
    assert src.data_ptr() % 16 == 0
    for size, name, jobs_of in groups:
        slot = (SC.GUARD + 16 + job_bytes(size, jobs_of[0][3]) + SC.GUARD + 15) & ~15
        dst = torch.full((slot * len(jobs_of),), 0xa5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        placed = run_jobs(L, lib.lh264_debug_filter_dev, size, name, jobs_of, lambda case: src.data_ptr() + offs[id(case)], dst.data_ptr(), slot)
        check(dst.cpu().numpy(), placed, (size, name, jobs_of[0][3]))


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d" % w)
def test_filtered_planes_on_the_device(window):
    _launch([(size, name, jobs_of) for (size, name), jobs_of in plane_jobs(window).items()])


def test_filtered_planes_placed_on_the_device():
    _launch([(size, name, jobs_of) for (size, name), jobs_of in placed_jobs().items()])


def test_filtered_colour_and_floats_on_the_device():
    _launch([(size, name, jobs_of) for (size, name, _variant, _placed), jobs_of in colour_jobs().items()])


# ---- 2: the call against the model of its full-size pictures ----------------------------------------------------------------------------------
QCIF = ["streams/BA_MW_D.264", "streams/test_qcif_cabac.264"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_the_call_delivers_the_model_of_its_full_size_pictures(name, fmt):
    """size=(224, 224) on a CAVLC and a CABAC QCIF stream, stretch, cover and contain: bytes and records are the model's"""
    import losslessh264_amd as lh
    full = _full(QCIF, fmt, select=FIRST)
    assert all(r[0] == OK and r[4] == [(176, 144)] * 4 and r[5] == FIRST for r in full)
    datas = [_read(n) for n in QCIF]
    for kw in (dict(), dict(fit="cover"), dict(fit="contain", fill=(81, 90, 240))):
        b = lh.decode_batch(datas, fmt=fmt, size=SIZE, filter=name, select=FIRST, **kw)
        assert b.filter == name and b._lib.lh264_decoded_filter(b._h[0]) == FM.FILTERS[name]
        got = _res(b, 2)
        for i in range(2):
            data, recs = _model(full, fmt, name, i, **kw)
            assert got[i][0] == OK and got[i][2] == recs and got[i][3] == data and got[i][4:] == full[i][4:], (name, fmt, kw, QCIF[i])
    area = _res(lh.decode_batch(datas, fmt=fmt, size=SIZE, select=FIRST), 2)
    assert area[0][3] != got[0][3]


@pytest.mark.parametrize("name", NAMES)
def test_two_window_sizes_in_one_batch(name):
    """176 x 144 and a cropped SPS's window under one size: each stream is resampled by tables of its own"""
    import losslessh264_amd as lh
    names = ["streams/BA_MW_D.264", "streams/CVFC1_Sony_C.jsv"]
    full = _full(names, select=[0, 1])
    assert full[0][4][0] != full[1][4][0] and all(r[0] == OK and len(r[2]) == 2 for r in full)
    got = _res(lh.decode_batch([_read(n) for n in names], size=SIZE, filter=name, select=[0, 1]), 2)
    for i in range(2):
        data, recs = _model(full, "i420", name, i)
        assert got[i][0] == OK and got[i][2] == recs and got[i][3] == data, (name, names[i])


def test_modes_deliver_the_host_mode_bytes():
    """device output (frames (i) is (pictures, 336, 224)), a sink, and digests with and without pictures deliver the host mode's bytes;
    the SHA-1 is hashlib's over them"""
    import losslessh264_amd as lh
    datas = [_read(n) for n in QCIF]
    kw = dict(size=SIZE, filter="bicubic", select=FIRST)
    want = _res(lh.decode_batch(datas, **kw), 2)
    full = _full(QCIF, "i420", select=FIRST)
    assert all(want[i][3] == _model(full, "i420", "bicubic", i)[0] for i in range(2))
    b = lh.decode_batch(datas, device_out=True, **kw)
    frames = [b.frames(i) for i in range(2)]
    assert [tuple(f.shape) for f in frames] == [(4, 336, 224)] * 2
    assert _res(b, 2, [f.cpu().numpy().tobytes() for f in frames]) == want
    seen = [[], []]

    def sink(stream, first, pics, data):
        seen[stream].append(data)
        return 0
    b = lh.decode_batch(datas, sink=sink, round_pictures=2, **kw)
    assert _res(b, 2, [b"".join(x) for x in seen]) == want
    b = lh.decode_batch(datas, sha1="both", **kw)
    digs = [(b.picture_sha1(i), b.stream_sha1(i)) for i in range(2)]
    assert _res(b, 2) == want
    for i in range(2):
        assert digs[i][0] == [hashlib.sha1(want[i][3][p[4]:p[4] + p[5]]).digest() for p in want[i][2]] and digs[i][1] == hashlib.sha1(want[i][3]).digest()
    b = lh.decode_batch(datas, sha1="both", pictures=False, **kw)
    assert [(b.picture_sha1(i), b.stream_sha1(i)) for i in range(2)] == digs
    res = _res(b, 2)
    assert all(res[i][3] == b"" and res[i][:3] == want[i][:3] for i in range(2))


@pytest.mark.parametrize("case", ["pick", "conceal", "parse", "crops"])
def test_with_the_other_arguments(case):
    """pick, concealment, the device parse route and a per-stream crop: the model of the same call without size and filter"""
    import losslessh264_amd as lh
    name = "bilinear" if case in ("pick", "crops") else "bicubic"
    if case == "crops":
        crops = [(16, 0, 144, 144), None]
        full = _full(QCIF, select=FIRST)
        got = _res(lh.decode_batch([_read(n) for n in QCIF], size=SIZE, filter=name, select=FIRST, crop=crops, fit="contain"), 2)
        for i in range(2):
            data, recs = _model(full, "i420", name, i, crop=crops[i], fit="contain")
            assert got[i][0] == OK and got[i][2] == recs and got[i][3] == data, i
        return
    stream, more = {"pick": ("streams/MIDR_MW_D.264", dict(pick="idr")), "conceal": ("conceal/sva_mid5.264", dict(conceal="mv_copy")),
                    "parse": ("streams/BA_MW_D.264", dict(parse="device", select=FIRST))}[case]
    full = _full([stream], **more)
    b = lh.decode_batch([_read(stream)], size=SIZE, filter=name, **more)
    route = b.parse_path(0)
    got = _res(b, 1)
    data, recs = _model(full, "i420", name, 0)
    assert len(recs) >= 1 and got[0][:2] == full[0][:2] and got[0][2] == recs and got[0][3] == data and got[0][4:] == full[0][4:], case
    if case == "parse":
        assert route == "device"


def test_rgbp_float16():
    """colour and the float type act on the filtered planes: RGBP float16 at (224, 224), cover, is rgb_model + sample_model of the
    model's planes, and frames (i) is (pictures, 3, 224, 224)"""
    import torch
    import losslessh264_amd as lh
    full = _full(QCIF, select=FIRST)
    mul, add = lh.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    tab = SM.table("float16", tuple(SM.f32(x) for x in mul), tuple(SM.f32(x) for x in add))
    b = lh.decode_batch([_read(n) for n in QCIF], size=SIZE, filter="bicubic", select=FIRST, fit="cover", colour="rgbp", dtype="float16", mul=mul, add=add, device_out=True)
    for i in range(2):
        fr = b.frames(i)
        assert tuple(fr.shape) == (4, 3, 224, 224) and fr.dtype == torch.float16
        data, recs = _model(full, "i420", "bicubic", i, fit="cover")
        exp = []
        for (w, h, fn, idr, at, n), std in zip(recs, b.colours(i)):
            rgb = rgb_model.rgb_from_planes(*scale_ref.unpack(data[at:at + n], w, h, scale_ref.FMT_I420), "rgbp", *std)
            exp.append(SM.apply_picture(rgb, "rgbp", tab).tobytes())
        assert b.tensor(i).cpu().numpy().tobytes() == b"".join(exp), i
    b.free()


def test_area_is_the_call_as_it_was():
    """filter="area", a filter struct that names LH264_FILTER_AREA, NULL and lh264_decode_batch_ex5 deliver the same bytes with the same
    launch shape (lh264_decode_last_chains)"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    lib = L.lib()
    datas = [_read(n) for n in QCIF]
    n = len(datas)
    ptrs, lens = (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas])
    opts = L.DecodeOptsV6()
    opts.struct_bytes, opts.out_width, opts.out_height = C.sizeof(L.DecodeOptsV6), 224, 224
    area = L.DecodeFilter()
    area.struct_bytes = 16

    def run(fn, *tail):
        outs = (C.c_void_p * n)()
        assert fn(ptrs, lens, n, 0, C.byref(opts), None, None, None, None, None, *tail, outs) == OK
        ch = (C.c_longlong * 3)()
        lib.lh264_decode_last_chains(ch)
        return _res(lh.DecodedBatch(lib, [outs[i] for i in range(n)], False), n), list(ch)
    want = run(lib.lh264_decode_batch_ex5)
    assert all(r[0] == OK and len(r[2]) > 4 for r in want[0])
    assert run(lib.lh264_decode_batch_ex6, None) == want and run(lib.lh264_decode_batch_ex6, C.byref(area)) == want
    b = lh.decode_batch(datas, size=SIZE, filter="area")
    assert b.filter == "area" and lib.lh264_decoded_filter(b._h[0]) == 0
    assert _res(b, n) == want[0] == _res(lh.decode_batch(datas, size=SIZE), n)


def test_the_command_lines_take_a_filter(tmp_path):
    """both command lines write the bytes the call delivers for --size 224x224 --filter bicubic"""
    import losslessh264_amd as lh
    src = os.path.join(GOLDEN, QCIF[0])
    want = _res(lh.decode_batch([_read(QCIF[0])], size=SIZE, filter="bicubic"), 1)[0][3]
    assert len(want) > 4 * 224 * 336
    for k, cmd in enumerate(([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"])):
        d = tmp_path / str(k)
        d.mkdir()
        r = subprocess.run(cmd + ["--decode", "--size", "224x224", "--filter", "bicubic", str(d), src], capture_output=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (cmd, r.stdout.decode(), r.stderr.decode())
        assert open(str(d / (os.path.basename(src) + ".yuv")), "rb").read() == want, cmd
