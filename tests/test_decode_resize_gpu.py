"""Pictures of one given size on the device: decode_pack_resized_kernel on synthetic windows (lh264_debug_resize_dev) against the
definition in numpy (tests/resize_ref.py), and lh264_decode_batch with a size against resize_ref of the same call without one - bytes,
picture records, statuses and texts - in every mode of the call.  Every reference is computed once."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import resize_ref
import scale_cases as SC
import scale_ref
from test_decode_resize import CONTENTS, WINDOWS, expect, targets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK = 0
# the streams of tests/test_decode_scale_gpu.py: QCIF, 300 x 168, 16 x 16, CABAC, 1080p, and the two that stop
STREAMS = ["streams/BA_MW_D.264", "streams/CVFC1_Sony_C.jsv", "cabac_edge/cabac_skip.264", "streams/test_qcif_cabac.264", "streams/syn1080p_IP_8f.264",
           "streams/BA_MW_D_IDR_LOST.264", "streams/Error_I_P.264", "streams/BA_MW_D.264+streams/Error_I_P.264"]
STOPPED = {"streams/Error_I_P.264": 0, "streams/BA_MW_D.264+streams/Error_I_P.264": 100}
SIZES = [(224, 224), (22, 18), (176, 144)]

_cache = {}


def _read(name):
    return b"".join(open(os.path.join(GOLDEN, part), "rb").read() for part in name.split("+"))


def _datas():
    if "datas" not in _cache:
        _cache["datas"] = [_read(n) for n in STREAMS]
    return _cache["datas"]


def _result(b, n, data=None):
    """what a call delivered, per stream: (status, text, picture records, bytes, source sizes, concealed)"""
    out = [(b.status(i), b.error(i), b.pictures(i), data[i] if data is not None else b.data(i), b.source_sizes(i), b.concealed(i)) for i in range(n)]
    b.free()
    return out


def _call(fmt, size):
    """ONE host-mode decode_batch over STREAMS per (format, size), shared by the tests"""
    if (fmt, size) not in _cache:
        import losslessh264_amd as lh
        _cache[(fmt, size)] = _result(lh.decode_batch(_datas(), fmt=fmt, size=size), len(STREAMS))
    return _cache[(fmt, size)]


def _expected(fmt, size):
    """resize_ref of the call without a size"""
    if ("x", fmt, size) not in _cache:
        _cache[("x", fmt, size)] = [resize_ref.resize_packed(r[3], r[2], fmt, size) for r in _call(fmt, None)]
    return _cache[("x", fmt, size)]


# ---- 1: synthetic windows on the device ---------------------------------------------------------------------------------------------
def _plan():
    """the cases, and per target size the jobs of its one launch: [(case index, format, destination offset from a 16-byte boundary)]"""
    if "plan" not in _cache:
        cases, by_size = [], {}
        for window in WINDOWS:
            for content in CONTENTS:
                cases.append(SC.Case(*window, seed=13 * window[0] + window[1], content=content))
                offsets = range(16) if content == "random" else (0, 2, 5)
                for size in targets(*window[:2]):
                    by_size.setdefault(size, []).extend((len(cases) - 1, fmt, off) for fmt in (0, 1) for off in offsets)
        cases.append(SC.Case(1920, 1080, 0, 0, seed=77, pic_w=1920, pic_h=1088))
        for size in ((224, 224), (398, 224)):
            by_size.setdefault(size, []).extend((len(cases) - 1, fmt, off) for fmt in (0, 1) for off in (0, 7))
        for content in (255, "random"):      # 2*S + D passes 2^32
            cases.append(SC.Case(4096, 2304, 0, 0, seed=5, content=content, pic_w=4096, pic_h=2304))
            by_size.setdefault((64, 36), []).extend((len(cases) - 1, fmt, 3) for fmt in (0, 1))
        _cache["plan"] = (cases, by_size)
    return _cache["plan"]


def _src_on_device():
    """every case's padded picture in one device tensor -> (tensor, [offset of case k])"""
    if "src" not in _cache:
        import torch
        cases = _plan()[0]
        at, offs = 0, []
        for case in cases:
            offs.append(at)
            at += (case.buf.size + 255) & ~255
        host = np.zeros(at, dtype=np.uint8)
        for case, o in zip(cases, offs):
            host[o:o + case.buf.size] = case.buf
        _cache["src"] = (torch.from_numpy(host).cuda(), offs)
    return _cache["src"]


def test_resized_pack_on_the_device():
    """one launch of the production kernel per target size holds every window that goes to that size - every content, both formats,
    the destination offsets - as a job of its own; the delivered bytes are the definition's and the 0xA5 between the jobs'
    destinations (64 guard bytes and more) is intact.  1920 x 1080 inside a 1920 x 1088 picture goes to 224 x 224 and 398 x 224, and
    4096 x 2304 (all 255, and random) to 64 x 36"""
    import torch
    from losslessh264_amd import _lib as L
    lib = L.lib()
    cases, by_size = _plan()
    src, offs = _src_on_device()
    assert src.data_ptr() % 16 == 0
    assert len(by_size[(224, 224)]) >= 8 * (32 + 3 * 6) + 4 and (398, 224) in by_size and len(by_size[(64, 36)]) >= 4 and len(by_size) >= 25
    for size, jobs_of in sorted(by_size.items()):
        n = size[0] * size[1] * 3 // 2
        slot = (SC.GUARD + 16 + n + SC.GUARD + 15) & ~15
        dst = torch.full((slot * len(jobs_of),), 0xa5, dtype=torch.uint8, device="cuda")
        assert dst.data_ptr() % 16 == 0
        jobs = (L.PackJob * len(jobs_of))()
        at = []
        for q, (k, fmt, off) in enumerate(jobs_of):
            at.append(q * slot + SC.GUARD + off)
            cases[k].fill_job(jobs[q], src.data_ptr() + offs[k], dst.data_ptr() + at[q], fmt, 0)
        torch.cuda.synchronize()
        assert lib.lh264_debug_resize_dev(jobs, len(jobs_of), size[0], size[1]) == OK
        got = dst.cpu().numpy()
        mask = np.ones(got.size, dtype=bool)
        for q, (k, fmt, off) in enumerate(jobs_of):
            exp = expect(cases[k], size, fmt)
            assert np.array_equal(got[at[q]:at[q] + n], exp), (cases[k].crop, size, fmt, off)
            mask[at[q]:at[q] + n] = False
        assert np.all(got[mask] == 0xa5), size
    k255 = len(cases) - 2
    assert np.all(expect(cases[k255], (64, 36), 0) == 255)


# ---- 2: the call against the call without a size ---------------------------------------------------------------------------------------
def test_the_streams_are_not_vacuous():
    """without a size every stream is LH264_OK except the two that Error_I_P's bytes stop; the batch mixes four window sizes"""
    base = _call("i420", None)
    sizes = set()
    for name, (st, err, pics, data, src, conc) in zip(STREAMS, base):
        assert (st == OK) == (name not in STOPPED), (name, st, err)
        if name in STOPPED:
            assert "picture %d" % STOPPED[name] in err and len(pics) == STOPPED[name], (name, err, len(pics))
        assert (len(pics) >= 1 or name == "streams/Error_I_P.264") and len(data) == sum(p[5] for p in pics), name
        assert src == [(p[0], p[1]) for p in pics], name
        sizes |= set(src)
    assert {(176, 144), (300, 168), (16, 16), (1920, 1080)} <= sizes, sizes


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_call_delivers_resize_ref_of_its_output_without_a_size(size, fmt):
    """every delivered picture of every stream has the one size; the bytes are resize_ref of the size-less call's, the statuses, texts
    and stop positions are that call's, source_sizes still gives the windows"""
    base, got, exp = _call(fmt, None), _call(fmt, size), _expected(fmt, size)
    n = size[0] * size[1] * 3 // 2
    for i, name in enumerate(STREAMS):
        assert got[i][0] == base[i][0] and got[i][1] == base[i][1], (name, got[i][:2])      # status and text
        assert got[i][2] == exp[i][1], name                                                   # width, height, frame_num, idr, offset, bytes
        assert [(p[0], p[1], p[5]) for p in got[i][2]] == [(size[0], size[1], n)] * len(base[i][2]), name
        assert got[i][3] == exp[i][0], name
        assert got[i][4] == base[i][4] == [(p[0], p[1]) for p in base[i][2]], name            # source_sizes
        assert got[i][5] == base[i][5], name
    if size == (176, 144):      # its own size: the QCIF streams come out as they are
        assert got[0][3] == base[0][3] and got[3][3] == base[3][3]


def test_a_size_of_half_the_window_is_scale_1():
    """size=(88, 72) on BA_MW_D.264 equals scale=1 byte for byte: same bytes, two kernels"""
    import losslessh264_amd as lh
    data = _datas()[0]
    for fmt in ("i420", "nv12"):
        a = _result(lh.decode_batch([data], fmt=fmt, size=(88, 72)), 1)[0]
        b = _result(lh.decode_batch([data], fmt=fmt, scale=1), 1)[0]
        assert len(a[3]) == 100 * 88 * 72 * 3 // 2 and a == b, fmt


# ---- 3: modes ----------------------------------------------------------------------------------------------------------------------------
def test_modes_deliver_the_host_mode_bytes():
    """(224, 224) on five streams of four window sizes: device output and frames(), a sink, digests with and without pictures, the
    cuts of the work, the parse routes, alone and in the batch"""
    import torch
    import losslessh264_amd as lh
    size, m = (224, 224), 5
    datas, want = _datas()[:m], _call("i420", (224, 224))[:m]
    assert all(len(w[3]) > 0 for w in want)

    def same(res, what):
        for i in range(m):
            assert res[i][:4] == want[i][:4] and res[i][4] == want[i][4], (what, STREAMS[i])
    b = lh.decode_batch(datas, size=size, device_out=True)
    frames = [b.frames(i) for i in range(m)]
    for i in range(m):
        assert tuple(frames[i].shape) == (len(want[i][2]), 336, 224) and frames[i].dtype == torch.uint8 and frames[i].is_cuda
        assert frames[i].cpu().numpy().tobytes() == want[i][3], STREAMS[i]
        k = len(want[i][2]) - 1
        y = np.frombuffer(want[i][3], dtype=np.uint8)[k * 75264:k * 75264 + 50176].reshape(224, 224)
        assert np.array_equal(frames[i][k, :224].cpu().numpy(), y), STREAMS[i]      # the last picture's luma plane
    same(_result(b, m, [f.cpu().numpy().tobytes() for f in frames]), "device_out")
    seen = [[] for _ in range(m)]
    recs = [[] for _ in range(m)]

    def sink(stream, first, pics, data):
        assert first == len(recs[stream]) and len(data) == sum(p[5] for p in pics)
        seen[stream].append(data)
        recs[stream] += pics
        return 0
    b = lh.decode_batch(datas, size=size, sink=sink, round_pictures=5)
    assert [b.data(i) for i in range(m)] == [b""] * m
    res = _result(b, m, [b"".join(x) for x in seen])
    same(res, "sink")
    assert [r[2] for r in res] == recs
    b = lh.decode_batch(datas, size=size, sha1="both")
    digs = [(b.picture_sha1(i), b.stream_sha1(i)) for i in range(m)]
    same(_result(b, m), "sha1")
    for i in range(m):
        assert digs[i][0] == [hashlib.sha1(want[i][3][p[4]:p[4] + p[5]]).digest() for p in want[i][2]], STREAMS[i]
        assert digs[i][1] == hashlib.sha1(want[i][3]).digest(), STREAMS[i]
    b = lh.decode_batch(datas, size=size, sha1="both", pictures=False)
    assert [(b.picture_sha1(i), b.stream_sha1(i)) for i in range(m)] == digs
    res = _result(b, m)
    for i in range(m):
        assert res[i][3] == b"" and res[i][:3] == want[i][:3] and res[i][4] == want[i][4], STREAMS[i]
    for kw in (dict(round_pictures=1), dict(threads=1), dict(parse="device"), dict(parse="device+cabac")):
        same(_result(lh.decode_batch(datas, size=size, **kw), m), kw)
    for i in (1, 2):
        alone = _result(lh.decode_batch([datas[i]], size=size), 1)[0]
        assert alone[:5] == want[i][:5], STREAMS[i]


def test_frames_needs_device_out_and_a_size():
    import losslessh264_amd as lh
    data = _datas()[2]
    for kw in (dict(device_out=True), dict(size=(22, 18))):
        b = lh.decode_batch([data], **kw)
        with pytest.raises(RuntimeError):
            b.frames(0)
        b.free()
    b = lh.decode_batch([_datas()[6]], device_out=True, size=(22, 18))      # Error_I_P.264 delivers nothing: no pictures, the same shape
    assert tuple(b.frames(0).shape) == (0, 27, 22)
    b.free()


# ---- 4: with pick and conceal --------------------------------------------------------------------------------------------------------------
def test_with_pick():
    """pick="idr" acts on what is decoded, the size on what is delivered: resize_ref of the same call without a size"""
    import losslessh264_amd as lh
    data = _read("streams/MIDR_MW_D.264")
    base_b = lh.decode_batch([data], pick="idr")
    got_b = lh.decode_batch([data], pick="idr", size=(46, 38))
    assert base_b.picture_indices(0) == got_b.picture_indices(0) and len(base_b.picture_indices(0)) == 2
    base, got = _result(base_b, 1)[0], _result(got_b, 1)[0]
    exp = resize_ref.resize_packed(base[3], base[2], "i420", (46, 38))
    assert got[:2] == base[:2] and got[2] == exp[1] and got[3] == exp[0] and got[4] == base[4]


def test_with_concealment():
    """the same pictures concealed as without a size; the delivered ones are resize_ref of that call's"""
    import losslessh264_amd as lh
    data = _read("conceal/sva_mid5.264")
    base = _result(lh.decode_batch([data], conceal="slice_copy"), 1)[0]
    got = _result(lh.decode_batch([data], conceal="slice_copy", size=(224, 224)), 1)[0]
    assert len(base[2]) >= 1 and sum(base[5]) > 0
    exp = resize_ref.resize_packed(base[3], base[2], "i420", (224, 224))
    assert got[:2] == base[:2] and got[2] == exp[1] and got[3] == exp[0] and got[4] == base[4] and got[5] == base[5]


# ---- 5: without a size the call is what it was -------------------------------------------------------------------------------------------
def test_no_size_is_what_it_was():
    """size=None in the 88-byte struct delivers what the 72-byte struct delivers, byte for byte - also with a size written behind its
    72 bytes - and the reference's stream SHA-1 still comes out for BA_MW_D.264"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    lib = L.lib()
    new = _call("i420", None)
    datas = _datas()
    n = len(datas)
    ptrs, lens = (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas])
    o = L.DecodeOptsV6()
    o.struct_bytes, o.out_width, o.out_height, o.reserved4 = 72, 224, 224, 9
    outs = (C.c_void_p * n)()
    assert lib.lh264_decode_batch(ptrs, lens, n, 0, C.byref(o), outs) == OK
    old = _result(lh.DecodedBatch(lib, [outs[i] for i in range(n)], False), n)
    assert [r[:5] for r in old] == [r[:5] for r in new]
    sha = json.load(open(os.path.join(GOLDEN, "decoder_sha1.json")))
    assert hashlib.sha1(new[0][3]).hexdigest() == sha["BA_MW_D.264"]


# ---- 6: the arena follows the delivered size ---------------------------------------------------------------------------------------------
_CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import losslessh264_amd as lh
one = open(%r, "rb").read()
b = lh.decode_batch([one] * 64, size=(int(sys.argv[1]), int(sys.argv[2])))
ok = [b.status(i) for i in range(64)].count(0)
nbytes = len(b.data(0))
b.free()
dev, pin = lh.decode_arena_bytes()
print(json.dumps({"ok": ok, "bytes": nbytes, "device": dev, "pinned": pin}))
"""


def test_the_arena_follows_the_delivered_size():
    """64 x BA_MW_D.264 in host mode, a fresh process per size: the page-locked bytes (and the device bytes) the call keeps are smaller
    at 22 x 18 than at 352 x 288, four times the window - the output buffers are sized for what is delivered"""
    code = _CHILD % (ROOT, os.path.join(GOLDEN, "streams", "BA_MW_D.264"))
    got = {}
    for size in ((22, 18), (352, 288)):
        out = subprocess.run([sys.executable, "-c", code, str(size[0]), str(size[1])], check=True, capture_output=True, timeout=600).stdout.decode()
        got[size] = json.loads(out.strip().splitlines()[-1])
        print("size %s: %s" % (size, got[size]))
        assert got[size]["ok"] == 64
    small, large = got[(22, 18)], got[(352, 288)]
    assert small["bytes"] == 100 * 594 and large["bytes"] == 100 * 352 * 288 * 3 // 2
    assert 0 < small["pinned"] < large["pinned"] and 0 < small["device"] < large["device"]
    # the two output buffers of a full round at the larger size alone are more than the difference has to explain
    assert large["pinned"] - small["pinned"] >= 2 * 64 * 8 * (352 * 288 * 3 // 2 - 594) * 9 // 10


# ---- 7: the command lines ------------------------------------------------------------------------------------------------------------------
def test_the_command_lines_take_a_size(tmp_path):
    """lh264dec --decode --size 224x224 and python -m losslessh264_amd --decode --size 224x224 write files of pictures * 224*224*3/2
    bytes, the host-mode bytes of the call; --sha1 writes the digests of those bytes and the delivered size"""
    want = _call("i420", (224, 224))
    srcs = [os.path.join(GOLDEN, STREAMS[0]), os.path.join(GOLDEN, STREAMS[1])]
    for k, cmd in enumerate(([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"])):
        d = tmp_path / str(k)
        d.mkdir()
        r = subprocess.run(cmd + ["--decode", "--size", "224x224", str(d)] + srcs, capture_output=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
        for i, s in enumerate(srcs):
            got = open(str(d / (os.path.basename(s) + ".yuv")), "rb").read()
            assert len(got) == len(want[i][2]) * 224 * 224 * 3 // 2 and got == want[i][3], (cmd, s)
    d = tmp_path / "sha1"
    d.mkdir()
    r = subprocess.run([os.path.join(ROOT, "losslessh264_amd", "lh264dec"), "--decode", "--sha1", "--size", "224x224", str(d), srcs[1]], capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()
    lines = open(str(d / (os.path.basename(srcs[1]) + ".sha1"))).read().split("\n")
    assert lines[0].split() == ["0", "224", "224", str(want[1][2][0][2]), str(want[1][2][0][3]), hashlib.sha1(want[1][3][:75264]).hexdigest()]
    assert lines[len(want[1][2])] == "stream " + hashlib.sha1(want[1][3]).hexdigest()
