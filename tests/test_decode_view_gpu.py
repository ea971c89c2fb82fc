"""Fitted views on the device (lh264_decode_batch_ex3: a caller's crop, cover, letterbox): the three placed production kernels over
the case table of tests/test_decode_view.py, and the call - every mode of it - against tests/view_model.py of the same call made without
a view and without a size."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import rgb_model
import sample_model as SM
import scale_cases as SC
import view_model as VM
from test_decode_resize_gpu import STOPPED, STREAMS, _datas, _read
from test_decode_view import FILLS, WINDOWS, case_of, check, fill_word, float_factors, groups, job_bytes, plan, run_jobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK, E_ARG = 0, -2
# a crop that fits every window of STREAMS (the smallest is 16 x 16), and one per stream with None entries
SMALL = (2, 4, 12, 10)
PER_STREAM = [(16, 0, 144, 144), None, (2, 2, 8, 8), None, (420, 0, 1080, 1080), None, None, (0, 0, 176, 144)]
CONFIGS = {
    "cover224": dict(fit="cover", size=(224, 224)), "contain224": dict(fit="contain", size=(224, 224), fill=(81, 90, 240)),
    "cover22": dict(fit="cover", size=(22, 18)), "contain22": dict(fit="contain", size=(22, 18)),
    "crop": dict(crop=SMALL), "crop+scale": dict(crop=(2, 4, 12, 10), scale=1), "crop+cover": dict(crop=(0, 2, 16, 10), fit="cover", size=(22, 18)),
    "crops": dict(crop=PER_STREAM), "crops+contain": dict(crop=PER_STREAM, fit="contain", size=(46, 38)),
}

_cache = {}


def _res(b, n, data=None):
    """what a call delivered, per stream: (status, text, picture records, bytes, source sizes, concealed, views)"""
    out = [(b.status(i), b.error(i), b.pictures(i), data[i] if data is not None else b.data(i), b.source_sizes(i), b.concealed(i), b.views(i)) for i in range(n)]
    b.free()
    return out


def _base(fmt="i420", **kw):
    """ONE decode_batch over STREAMS without a view and without a size per (format, other arguments), shared by the tests"""
    key = (fmt,) + tuple(sorted(kw.items()))
    if key not in _cache:
        import losslessh264_amd as lh
        _cache[key] = _res(lh.decode_batch(_datas(), fmt=fmt, **kw), len(STREAMS))
    return _cache[key]


def _crop_of(view_kw, i):
    c = view_kw.get("crop")
    return c[i] if isinstance(c, list) else c


def _model(base, fmt, view_kw, i):
    """view_model of stream i of the base call -> (bytes, records, views, stop)"""
    kw = {k: v for k, v in view_kw.items() if k != "crop"}
    return VM.view_packed(base[i][3], base[i][2], fmt, crop=_crop_of(view_kw, i), **kw)


def _same_as_model(got, base, fmt, view_kw, what, streams=None):
    for i in (range(len(got)) if streams is None else streams):
        name = STREAMS[i]
        data, recs, views, stop = _model(base, fmt, view_kw, i)
        crop = _crop_of(view_kw, i)
        if stop is None:
            assert got[i][0] == base[i][0] and got[i][1] == base[i][1], (what, name, got[i][:2])
        else:
            w, h = base[i][2][stop][:2]
            assert got[i][0] == E_ARG and got[i][1] == "picture %d: the crop {%d, %d, %d, %d} does not fit the picture's %d x %d window" % ((stop,) + tuple(crop) + (w, h)), (what, name, got[i][:2])
        assert got[i][2] == recs, (what, name)
        assert got[i][3] == data, (what, name)
        assert got[i][4] == base[i][4][:len(recs)] and got[i][5] == base[i][5][:len(recs)], (what, name)
        assert got[i][6] == views, (what, name, got[i][6][:2], views[:2])


# ---- 1: the production kernels over the case table ---------------------------------------------------------------------------------------
def _src_on_device(by_size):
    import torch
    cases = {}
    for jobs in by_size.values():
        for j in jobs:
            cases[(j[0], j[1])] = case_of(j[0], j[1])
    at, offs = 0, {}
    for key, case in cases.items():
        offs[id(case)] = at
        at += (case.buf.size + 255) & ~255
    host = np.zeros(at, dtype=np.uint8)
    for case in cases.values():
        host[offs[id(case)]:offs[id(case)] + case.buf.size] = case.buf
    return torch.from_numpy(host).cuda(), offs


@pytest.mark.parametrize("path", ["yuv", "rgb", "float"])
def test_placed_kernels_on_the_device(path):
    """the case table of tests/test_decode_view.py, every case a job: one launch of the production kernel per output size (and, for RGB
    and floats, per layout and type: a launch has one).  The bytes are the model's and the 0xA5 between the jobs' destinations is
    intact"""
    import torch
    from losslessh264_amd import _lib as L
    lib = L.lib()
    by_size = plan(path)
    src, offs = _src_on_device(by_size)
    assert src.data_ptr() % 16 == 0
    launches = 0
    for size, jobs_of in sorted(by_size.items()):
        for grp in groups(jobs_of):
            slot = (SC.GUARD + 16 + job_bytes(size, grp[0][4]) + SC.GUARD + 15) & ~15
            dst = torch.full((slot * len(grp),), 0xa5, dtype=torch.uint8, device="cuda")
            assert dst.data_ptr() % 16 == 0
            torch.cuda.synchronize()
            placed = run_jobs(L, lib.lh264_debug_view_dev, size, grp, lambda case: src.data_ptr() + offs[id(case)], dst.data_ptr(), slot)
            check(dst.cpu().numpy(), placed, (path, size, grp[0][4]))
            launches += 1
    assert launches == 7 * {"yuv": 1, "rgb": 2, "float": 6}[path]


def test_the_whole_output_is_the_unplaced_kernels_on_the_device():
    """a place that is the whole output delivers the bytes of lh264_debug_resize_dev / _rgb_dev / _sample_dev"""
    import torch
    from losslessh264_amd import _lib as L
    lib = L.lib()
    mul, add = float_factors()
    sm = L.DecodeSample()
    sm.struct_bytes, sm.type = 32, L.SAMPLE["bfloat16"]
    for k in range(3):
        sm.mul[k], sm.add[k] = float(mul[k]), float(add[k])
    for window in WINDOWS:
        case = case_of(window, "random")
        src = torch.from_numpy(case.buf).cuda()
        for size in ((10, 6), (224, 224)):
            for colour, sample, nbytes, fmt in ((0, None, size[0] * size[1] * 3 // 2, L.FMT_NV12), (1, None, size[0] * size[1] * 3, 0), (2, sm, size[0] * size[1] * 6, 0)):
                a, b = (torch.full((nbytes + 32,), 0xa5, dtype=torch.uint8, device="cuda") for _ in range(2))
                ja, jb = L.PackJob(), L.PackJob()
                case.fill_job(ja, src.data_ptr(), a.data_ptr() + 16, fmt, 0)
                case.fill_job(jb, src.data_ptr(), b.data_ptr() + 16, fmt, 0)
                pl = L.PackPlace(0, 0, size[0], size[1], fill_word(FILLS[3]), 0)
                std = (C.c_uint8 * 1)(1)
                torch.cuda.synchronize()
                assert lib.lh264_debug_view_dev(C.byref(ja), C.byref(pl), 1, size[0], size[1], colour, std, C.byref(sample) if sample else None) == OK
                if sample:
                    assert lib.lh264_debug_sample_dev(C.byref(jb), 1, size[0], size[1], colour, std, C.byref(sample)) == OK
                elif colour:
                    assert lib.lh264_debug_rgb_dev(C.byref(jb), 1, size[0], size[1], colour, std) == OK
                else:
                    assert lib.lh264_debug_resize_dev(C.byref(jb), 1, size[0], size[1]) == OK
                ga, gb = a.cpu().numpy(), b.cpu().numpy()
                assert np.array_equal(ga, gb) and not np.all(ga[16:16 + nbytes] == 0xa5) and np.all(ga[:16] == 0xa5) and np.all(ga[16 + nbytes:] == 0xa5), (window, size, colour)


# ---- 2: the call against the model ---------------------------------------------------------------------------------------------------------
def test_the_streams_are_not_vacuous():
    base = _base()
    sizes = set()
    for name, r in zip(STREAMS, base):
        assert (r[0] == OK) == (name not in STOPPED) and (len(r[2]) >= 1 or name == "streams/Error_I_P.264"), name
        assert r[6] == [((0, 0, w, h), (0, 0, w, h)) for (w, h) in r[4]], name      # views of a call without a view
        sizes |= set(r[4])
    assert {(176, 144), (300, 168), (16, 16), (1920, 1080)} <= sizes
    assert all(c is None or VM.crop_fits(c, *base[i][4][0]) for i, c in enumerate(PER_STREAM) if base[i][4])


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_call_delivers_the_model_of_its_output_without_a_view(name):
    """one decode_batch over the streams per configuration: bytes, picture records, statuses, texts and views(i) are view_model's of the
    same call without a view and without a size"""
    import losslessh264_amd as lh
    kw = CONFIGS[name]
    got = _res(lh.decode_batch(_datas(), **kw), len(STREAMS))
    _same_as_model(got, _base(), "i420", kw, name)
    if "size" in kw:
        assert all(p[:2] == kw["size"] for r in got for p in r[2])
    if name == "contain224":
        assert got[0][6][0] == ((0, 0, 176, 144), (0, 20, 224, 184)) and got[4][6][0] == ((0, 0, 1920, 1080), (0, 48, 224, 126))
    if name == "cover224":
        assert got[0][6][0] == ((16, 0, 144, 144), (0, 0, 224, 224)) and got[4][6][0] == ((420, 0, 1080, 1080), (0, 0, 224, 224))


def test_identities():
    """an empty view is lh264_decode_batch_ex2; cover and contain at a size of the stream's own aspect are the stretch; a crop equal to
    the window is no crop"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    lib = L.lib()
    base = _base()
    datas = _datas()
    n = len(datas)
    ptrs, lens = (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas])
    v = L.DecodeView()
    v.struct_bytes = 32
    outs = (C.c_void_p * n)()
    assert lib.lh264_decode_batch_ex3(ptrs, lens, n, 0, None, None, None, C.byref(v), outs) == OK
    assert _res(lh.DecodedBatch(lib, [outs[i] for i in range(n)], False), n) == base
    one = [datas[0]]
    stretch = _res(lh.decode_batch(one, size=(88, 72)), 1)
    for fit in ("cover", "contain"):
        assert _res(lh.decode_batch(one, size=(88, 72), fit=fit), 1) == stretch, fit
    assert _res(lh.decode_batch(one, crop=(0, 0, 176, 144)), 1) == [base[0]]
    assert _res(lh.decode_batch(one, crop=(0, 0, 176, 144), size=(88, 72), fit="contain", fill=(1, 2, 3)), 1) == stretch


def test_a_crop_that_stops_a_stream():
    """a 176 x 144 crop on the stream with the 16 x 16 pictures (its first three are 640 x 480, which the crop fits), and on BA_MW_D
    followed by the 152 x 100 Static.264: LH264_E_ARG at the first picture whose window the crop does not fit, with a text that names the picture, the rectangle and the window; the pictures in front of it are the model's; the other
    stream of the batch is untouched"""
    import losslessh264_amd as lh
    small, qcif, static = _read("cabac_edge/cabac_skip.264"), _read("streams/BA_MW_D.264"), _read("streams/Static.264")
    datas = [small, qcif, qcif + static]
    base = _res(lh.decode_batch(datas), 3)
    assert [r[0] for r in base] == [OK] * 3 and len(base[2][2]) > len(base[1][2]) and base[2][4][-1] == (152, 100)
    crop = (0, 0, 176, 144)
    got = _res(lh.decode_batch(datas, crop=crop, size=(22, 18), fit="contain"), 3)
    n = len(base[1][2])
    assert base[0][4] == [(640, 480)] * 3 + [(16, 16)] * 2
    assert got[0][0] == E_ARG and got[0][1] == "picture 3: the crop {0, 0, 176, 144} does not fit the picture's 16 x 16 window"
    assert got[2][0] == E_ARG and got[2][1] == "picture %d: the crop {0, 0, 176, 144} does not fit the picture's 152 x 100 window" % n
    for i in (0, 1, 2):
        data, recs, views, stop = VM.view_packed(base[i][3], base[i][2], "i420", crop=crop, fit="contain", size=(22, 18))
        assert stop == (3, None, n)[i] and len(recs) == (3, n, n)[i]
        assert got[i][2] == recs and got[i][3] == data and got[i][6] == views, i
    assert got[1][0] == OK and got[1][1] == ""


# ---- 3: modes -------------------------------------------------------------------------------------------------------------------------------
def test_modes_deliver_the_model():
    """contain at (224, 224) on five streams of four window sizes: device output, a sink, digests with and without pictures, the cuts of
    the work and the device parse route deliver the host mode's bytes, which are the model's; pick, conceal and NV12 the model of the
    same call without a view"""
    import losslessh264_amd as lh
    m = 5
    kw = dict(fit="contain", size=(224, 224), fill=(81, 90, 240))
    datas = _datas()[:m]
    want = _res(lh.decode_batch(datas, **kw), m)
    _same_as_model(want, _base(), "i420", kw, "host mode", range(m))

    def same(res, what):
        for i in range(m):
            assert res[i] == want[i], (what, STREAMS[i])
    b = lh.decode_batch(datas, device_out=True, **kw)
    frames = [b.frames(i) for i in range(m)]
    assert [tuple(f.shape) for f in frames] == [(len(want[i][2]), 336, 224) for i in range(m)]
    same(_res(b, m, [f.cpu().numpy().tobytes() for f in frames]), "device_out")
    seen = [[] for _ in range(m)]

    def sink(stream, first, pics, data):
        seen[stream].append(data)
        return 0
    b = lh.decode_batch(datas, sink=sink, round_pictures=2, **kw)
    same(_res(b, m, [b"".join(x) for x in seen]), "sink")
    b = lh.decode_batch(datas, sha1="both", **kw)
    digs = [(b.picture_sha1(i), b.stream_sha1(i)) for i in range(m)]
    same(_res(b, m), "sha1")
    for i in range(m):
        assert digs[i][0] == [hashlib.sha1(want[i][3][p[4]:p[4] + p[5]]).digest() for p in want[i][2]], STREAMS[i]
        assert digs[i][1] == hashlib.sha1(want[i][3]).digest(), STREAMS[i]
    b = lh.decode_batch(datas, sha1="both", pictures=False, **kw)
    assert [(b.picture_sha1(i), b.stream_sha1(i)) for i in range(m)] == digs
    res = _res(b, m)
    for i in range(m):
        assert res[i][3] == b"" and res[i][:3] == want[i][:3] and res[i][4:] == want[i][4:], STREAMS[i]
    for more in (dict(round_pictures=8), dict(parse="device")):
        same(_res(lh.decode_batch(datas, **more, **kw), m), more)
    got = _res(lh.decode_batch(_datas(), fmt="nv12", **kw), len(STREAMS))
    _same_as_model(got, _base("nv12"), "nv12", kw, "nv12")
    for data, more in ((_read("streams/MIDR_MW_D.264"), dict(pick="idr")), (_read("conceal/sva_mid5.264"), dict(conceal="mv_copy"))):
        base = _res(lh.decode_batch([data], **more), 1)[0]
        got = _res(lh.decode_batch([data], **more, **kw), 1)[0]
        exp = VM.view_packed(base[3], base[2], "i420", **kw)
        assert len(base[2]) >= 1 and got[:2] == base[:2] and got[2] == exp[1] and got[3] == exp[0] and got[4:6] == base[4:6] and got[6] == exp[2], more


def test_rgbp_float16_contain():
    """colour and the float type act on the delivered planes, bars included: RGBP float16 at (224, 224) is rgb_model + sample_model of
    view_model's planes, and frames(i) is (pictures, 3, 224, 224)"""
    import torch
    import losslessh264_amd as lh
    m = 5
    datas = _datas()[:m]
    mul, add = lh.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    kw = dict(fit="contain", size=(224, 224), fill=(81, 90, 240))
    b = lh.decode_batch(datas, colour="rgbp", dtype="float16", mul=mul, add=add, device_out=True, **kw)
    base = _base()
    tab = SM.table("float16", tuple(SM.f32(x) for x in mul), tuple(SM.f32(x) for x in add))
    for i in range(m):
        fr = b.frames(i)
        data, recs, views, stop = _model(base, "i420", kw, i)
        assert tuple(fr.shape) == (len(recs), 3, 224, 224) and fr.dtype == torch.float16 and stop is None and b.views(i) == views
        got = b.tensor(i).cpu().numpy().tobytes()
        stds = b.colours(i)
        exp, memo = [], {}
        for (w, h, fn, idr, at, n), std in zip(recs, stds):
            key = (data[at:at + n], std)
            if key not in memo:
                rgb = rgb_model.rgb_packed(key[0], [(w, h, fn, idr, 0, n)], "rgbp", std)[0]
                memo[key] = SM.apply_picture(np.frombuffer(rgb, dtype=np.uint8), "rgbp", tab).tobytes()
            exp.append(memo[key])
        assert got == b"".join(exp), STREAMS[i]
        # a bar element is the fma of the converted fill
        y, cb, cr = (np.full((1, 1), v, dtype=np.uint8) for v in (81, 90, 240))
        bar = [int(c[0, 0]) for c in rgb_model.convert(y, cb, cr, *stds[0])]
        if views[0][1][1] > 0:
            assert fr[0, :, 0, 0].contiguous().cpu().view(torch.int16).numpy().astype(np.uint16).tolist() == [int(tab[c, bar[c]]) for c in range(3)], STREAMS[i]
        else:
            assert STREAMS[i] == "cabac_edge/cabac_skip.264"      # 16 x 16 has the size's aspect: no bar
    b.free()


# ---- 4: the command lines -----------------------------------------------------------------------------------------------------------------
def test_the_command_lines_take_a_view(tmp_path):
    """both command lines write .yuv / .rgb files equal to the model for --fit contain --fill 81,90,240 --size 46x38 and for
    --crop 16,0,144,144"""
    base = _base()[0]
    src = os.path.join(GOLDEN, STREAMS[0])
    contain = VM.view_packed(base[3], base[2], "i420", fit="contain", fill=(81, 90, 240), size=(46, 38))
    crop = VM.view_packed(base[3], base[2], "i420", crop=(16, 0, 144, 144))
    rgb = rgb_model.rgb_packed(contain[0], contain[1], "rgb24", ("bt601", "limited"))[0]
    assert len(contain[0]) == len(base[2]) * 46 * 38 * 3 // 2 and len(crop[0]) == len(base[2]) * 144 * 144 * 3 // 2
    for k, cmd in enumerate(([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"])):
        for q, (args, suffix, want) in enumerate(((["--fit", "contain", "--fill", "81,90,240", "--size", "46x38"], ".yuv", contain[0]), (["--crop", "16,0,144,144"], ".yuv", crop[0]),
                                                 (["--rgb", "rgb24", "--size", "46x38", "--fill", "81,90,240", "--fit", "contain"], ".rgb", rgb))):
            d = tmp_path / ("%d_%d" % (k, q))
            d.mkdir()
            r = subprocess.run(cmd + ["--decode"] + args + [str(d), src], capture_output=True, timeout=300, cwd=ROOT)
            assert r.returncode == 0, (cmd, args, r.stdout.decode(), r.stderr.decode())
            assert open(str(d / (os.path.basename(src) + suffix)), "rb").read() == want, (cmd, args)
