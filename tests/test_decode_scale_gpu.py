"""Reduced-size pictures on the device: decode_pack_scaled_kernel on synthetic windows (lh264_debug_pack_dev) against the definition
in numpy (tests/scale_ref.py), and lh264_decode_batch at scale 1..3 against scale_ref of its own scale-0 output - bytes, picture
records, statuses and texts - in every mode of the call.  Every reference is computed once."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scale_cases as SC
import scale_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK = 0
STREAMS = ["streams/BA_MW_D.264", "streams/CVFC1_Sony_C.jsv", "cabac_edge/cabac_skip.264", "streams/test_qcif_cabac.264", "streams/syn1080p_IP_8f.264",
           "streams/BA_MW_D_IDR_LOST.264", "streams/Error_I_P.264", "streams/BA_MW_D.264+streams/Error_I_P.264"]
# Error_I_P.264 alone stops at its picture 0 (macroblocks no slice covers) and delivers nothing, at any scale: it is held to its status
# and text.  Behind BA_MW_D.264 the same bytes stop the stream at picture 100: the 100 pictures in front are delivered, scaled.
STOPPED = {"streams/Error_I_P.264": 0, "streams/BA_MW_D.264+streams/Error_I_P.264": 100}

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


def _call(fmt, s):
    """ONE host-mode decode_batch over STREAMS per (format, scale), shared by the tests"""
    if (fmt, s) not in _cache:
        import losslessh264_amd as lh
        _cache[(fmt, s)] = _result(lh.decode_batch(_datas(), fmt=fmt, scale=s), len(STREAMS))
    return _cache[(fmt, s)]


def _expected(fmt, s):
    """scale_ref of the scale-0 call"""
    if ("x", fmt, s) not in _cache:
        _cache[("x", fmt, s)] = [scale_ref.scale_packed(r[3], r[2], fmt, s) for r in _call(fmt, 0)]
    return _cache[("x", fmt, s)]


# ---- 1: synthetic windows on the device ---------------------------------------------------------------------------------------------
def _cases():
    if "cases" not in _cache:
        cs = [(SC.Case(*w, seed=31 * k + 1), range(16)) for k, w in enumerate(SC.WINDOWS)]
        for w in ((16, 16, 0, 0), (18, 14, 0, 0)):
            cs += [(SC.Case(*w, content=c), (0, 2, 5)) for c in (255, 0, "checker")]
        cs.append((SC.Case(1920, 1080, 0, 0, seed=77, pic_w=1920, pic_h=1088), (0, 2, 7)))      # och = 68 at s = 3: the bottom row averages clamped rows
        cs.append((SC.Case(1280, 720, 0, 0, seed=78, pic_w=1280, pic_h=720), (0, 2, 7)))
        _cache["cases"] = cs
    return _cache["cases"]


def _src_on_device():
    """every case's padded picture in one device tensor -> (tensor, [offset of case k])"""
    if "src" not in _cache:
        import torch
        at, offs = 0, []
        for case, _ in _cases():
            offs.append(at)
            at += (case.buf.size + 255) & ~255
        host = np.zeros(at, dtype=np.uint8)
        for (case, _), o in zip(_cases(), offs):
            host[o:o + case.buf.size] = case.buf
        _cache["src"] = (torch.from_numpy(host).cuda(), offs)
    return _cache["src"]


@pytest.mark.parametrize("s", [1, 2, 3])
def test_scaled_pack_on_the_device(s):
    """one launch of the production kernel per scale holds every window, content, format and destination offset as a job of its own;
    the delivered bytes are the definition's and the 0xA5 between the jobs' destinations (64 guard bytes and more) is intact"""
    import torch
    from losslessh264_amd import _lib as L
    lib = L.lib()
    src, offs = _src_on_device()
    plan, at = [], 0
    for k, (case, offsets) in enumerate(_cases()):
        for fmt in (L.FMT_I420, L.FMT_NV12):
            n = case.expect(s, fmt).size
            for off in offsets:
                plan.append((k, fmt, at + SC.GUARD + off, n))
                at += (SC.GUARD + 16 + n + SC.GUARD + 15) & ~15
    dst = torch.full((at,), 0xa5, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    jobs = (L.PackJob * len(plan))()
    for j, (k, fmt, d, n) in zip(jobs, plan):
        _cases()[k][0].fill_job(j, src.data_ptr() + offs[k], dst.data_ptr() + d, fmt, s)
    torch.cuda.synchronize()
    assert lib.lh264_debug_pack_dev(jobs, len(plan)) == OK
    got = dst.cpu().numpy()
    mask = np.ones(at, dtype=bool)
    for (k, fmt, d, n) in plan:
        case = _cases()[k][0]
        assert np.array_equal(got[d:d + n], case.expect(s, fmt)), (case.crop, s, fmt, d % 16)
        mask[d:d + n] = False
    assert np.all(got[mask] == 0xa5)
    ow, oh = scale_ref.scaled_size(1920, 1080, 3)
    assert (ow, oh) == (240, 136) and len(plan) >= 13 * 32 + 36 + 12


def test_pack_dev_at_scale_0_is_the_copy():
    """lh264_debug_pack_dev with scale 0 launches the copy kernel: the window's samples, cropped"""
    import torch
    from losslessh264_amd import _lib as L
    case = _cases()[11][0]
    assert case.crop == (26, 60, 300, 168)
    src, offs = _src_on_device()
    exp = np.frombuffer(scale_ref.pack(case.Y, case.U, case.V, L.FMT_NV12), dtype=np.uint8)
    dst = torch.full((exp.size + 256,), 0xa5, dtype=torch.uint8, device="cuda")
    j = L.PackJob()
    case.fill_job(j, src.data_ptr() + offs[11], dst.data_ptr() + 70, L.FMT_NV12, 0)
    torch.cuda.synchronize()
    assert L.lib().lh264_debug_pack_dev(C.byref(j), 1) == OK
    got = dst.cpu().numpy()
    assert np.array_equal(got[70:70 + exp.size], exp) and np.all(got[:70] == 0xa5) and np.all(got[70 + exp.size:] == 0xa5)


# ---- 2: the call against the scale-0 call ----------------------------------------------------------------------------------------------
def test_the_streams_are_not_vacuous():
    """at scale 0 every stream is LH264_OK except the two that Error_I_P's bytes stop; every one delivers a picture except Error_I_P
    alone, whose first picture is the one that stops it - the stream that carries it behind BA_MW_D.264 stops at a picture with 100
    pictures in front; and the batch holds at least three window sizes"""
    base = _call("i420", 0)
    sizes = set()
    for name, (st, err, pics, data, src, conc) in zip(STREAMS, base):
        assert (st == OK) == (name not in STOPPED), (name, st, err)
        if name in STOPPED:
            assert "picture %d" % STOPPED[name] in err and len(pics) == STOPPED[name], (name, err, len(pics))
        assert (len(pics) >= 1 or name == "streams/Error_I_P.264") and len(data) == sum(p[5] for p in pics), name
        assert src == [(p[0], p[1]) for p in pics], name
        sizes |= set(src)
    assert len(sizes) >= 3 and (176, 144) in sizes and (300, 168) in sizes and (16, 16) in sizes and (1920, 1080) in sizes, sizes


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_the_call_delivers_scale_ref_of_its_scale_0_output(s, fmt):
    base, got, exp = _call(fmt, 0), _call(fmt, s), _expected(fmt, s)
    for i, name in enumerate(STREAMS):
        assert got[i][0] == base[i][0] and got[i][1] == base[i][1], (name, got[i][:2])      # status and text
        assert got[i][2] == exp[i][1], name                                                   # width, height, frame_num, idr, offset, bytes
        assert got[i][3] == exp[i][0], name
        assert got[i][4] == base[i][4] == [(p[0], p[1]) for p in base[i][2]], name            # source_sizes
        assert got[i][5] == base[i][5], name
    if s == 3:
        assert (22, 18, 594) in [(p[0], p[1], p[5]) for p in got[0][2]] and (2, 2) in [(p[0], p[1]) for p in got[2][2]]


# ---- 3: modes ----------------------------------------------------------------------------------------------------------------------------
def test_modes_deliver_the_host_mode_bytes():
    """s = 2 on the first three streams: device output, a sink, the cuts of the work, the parse routes, alone and in the batch"""
    import losslessh264_amd as lh
    datas, want = _datas()[:3], _call("i420", 2)[:3]
    assert all(len(w[3]) > 0 for w in want)

    def same(res, what):
        for i in range(3):
            assert res[i][:4] == want[i][:4] and res[i][4] == want[i][4], (what, STREAMS[i])
    b = lh.decode_batch(datas, scale=2, device_out=True)
    same(_result(b, 3, [b.tensor(i).cpu().numpy().tobytes() for i in range(3)]), "device_out")
    seen = [[] for _ in range(3)]
    recs = [[] for _ in range(3)]

    def sink(stream, first, pics, data):
        assert first == len(recs[stream]) and len(data) == sum(p[5] for p in pics)
        seen[stream].append(data)
        recs[stream] += pics
        return 0
    b = lh.decode_batch(datas, scale=2, sink=sink, round_pictures=5)
    assert [b.data(i) for i in range(3)] == [b""] * 3
    res = _result(b, 3, [b"".join(x) for x in seen])
    same(res, "sink")
    assert [r[2] for r in res] == recs
    for kw in (dict(round_pictures=1), dict(round_pictures=8), dict(threads=1), dict(parse="device"), dict(parse="device+cabac")):
        same(_result(lh.decode_batch(datas, scale=2, **kw), 3), kw)
    for i in range(3):
        alone = _result(lh.decode_batch([datas[i]], scale=2), 1)[0]
        assert alone[:5] == want[i][:5], STREAMS[i]


# ---- 4: digests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,fmt", [(1, "nv12"), (2, "i420"), (3, "i420")])
def test_digests_are_of_the_delivered_bytes(s, fmt):
    import losslessh264_amd as lh
    n = len(STREAMS)
    b = lh.decode_batch(_datas(), fmt=fmt, scale=s, sha1="both")
    digs = [(b.picture_sha1(i), b.stream_sha1(i)) for i in range(n)]
    res = _result(b, n)
    want = _call(fmt, s)
    for i in range(n):
        assert res[i][:4] == want[i][:4], STREAMS[i]
        assert digs[i][0] == [hashlib.sha1(res[i][3][p[4]:p[4] + p[5]]).digest() for p in res[i][2]], STREAMS[i]
        assert digs[i][1] == hashlib.sha1(res[i][3]).digest(), STREAMS[i]
    b = lh.decode_batch(_datas(), fmt=fmt, scale=s, sha1="both", pictures=False)
    assert [(b.picture_sha1(i), b.stream_sha1(i)) for i in range(n)] == digs
    res = _result(b, n)
    for i in range(n):
        assert res[i][3] == b"" and res[i][:3] == want[i][:3] and res[i][4] == want[i][4], STREAMS[i]


# ---- 5: concealment ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conceal,name", [("mv_copy_freeze", "conceal/sva_head5.264"), ("slice_copy", "conceal/sva_mid5.264")])
def test_concealment_at_scale_1(conceal, name):
    """the same pictures withheld and concealed as at scale 0; the delivered ones are scale_ref of the scale-0 call's"""
    import losslessh264_amd as lh
    data = _read(name)
    base = _result(lh.decode_batch([data], conceal=conceal), 1)[0]
    got = _result(lh.decode_batch([data], conceal=conceal, scale=1), 1)[0]
    assert len(base[2]) >= 1 and sum(base[5]) > 0
    exp = scale_ref.scale_packed(base[3], base[2], "i420", 1)
    assert got[:2] == base[:2] and got[2] == exp[1] and got[3] == exp[0] and got[4] == base[4] and got[5] == base[5]


# ---- 6: scale 0 is what it was ----------------------------------------------------------------------------------------------------------
def test_scale_0_is_what_it_was():
    """scale=0 in the 64-byte struct delivers what the 56-byte struct, the 48-byte struct and NULL options deliver, byte for byte, and
    the reference's stream SHA-1 still comes out for BA_MW_D.264"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    lib = L.lib()
    new = _result(lh.decode_batch(_datas(), scale=0), len(STREAMS))
    assert [r[:5] for r in new] == [r[:5] for r in _call("i420", 0)]
    datas = _datas()
    n = len(datas)
    ptrs, lens = (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas])
    for struct_bytes in (56, 48, None):
        o = L.DecodeOptsV3()
        o.struct_bytes = struct_bytes or 0
        outs = (C.c_void_p * n)()
        assert lib.lh264_decode_batch(ptrs, lens, n, 0, C.byref(o) if struct_bytes else None, outs) == OK
        b = lh.DecodedBatch(lib, [outs[i] for i in range(n)], False)
        old = _result(b, n)
        assert [r[:5] for r in old] == [r[:5] for r in new], struct_bytes
    sha = json.load(open(os.path.join(GOLDEN, "decoder_sha1.json")))
    assert hashlib.sha1(new[0][3]).hexdigest() == sha["BA_MW_D.264"]


# ---- 7: the arena follows the delivered size ---------------------------------------------------------------------------------------------
_CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import losslessh264_amd as lh
one = open(%r, "rb").read()
b = lh.decode_batch([one] * 64, scale=int(sys.argv[1]))
ok = [b.status(i) for i in range(64)].count(0)
nbytes = len(b.data(0))
b.free()
dev, pin = lh.decode_arena_bytes()
print(json.dumps({"ok": ok, "bytes": nbytes, "device": dev, "pinned": pin}))
"""


def test_the_arena_follows_the_delivered_size():
    """64 x BA_MW_D.264 in host mode, a fresh process per scale: the page-locked bytes (and the device bytes) the call keeps are
    smaller at scale 3 than at scale 0 - the output buffers are sized for what is delivered"""
    code = _CHILD % (ROOT, os.path.join(GOLDEN, "streams", "BA_MW_D.264"))
    got = {}
    for s in (3, 0):
        out = subprocess.run([sys.executable, "-c", code, str(s)], check=True, capture_output=True, timeout=600).stdout.decode()
        got[s] = json.loads(out.strip().splitlines()[-1])
        print("scale %d: %s" % (s, got[s]))
        assert got[s]["ok"] == 64
    assert got[0]["bytes"] == 100 * 176 * 144 * 3 // 2 and got[3]["bytes"] == 100 * 594
    assert 0 < got[3]["pinned"] < got[0]["pinned"] and 0 < got[3]["device"] < got[0]["device"]
    # the two output buffers of a full round at scale 0 alone are more than the difference has to explain
    assert got[0]["pinned"] - got[3]["pinned"] >= 2 * 64 * 8 * (176 * 144 * 3 // 2 - 594) * 9 // 10


# ---- 8: the command lines ------------------------------------------------------------------------------------------------------------------
def test_the_command_lines_take_scale(tmp_path):
    """lh264dec --decode --scale 2 and python -m losslessh264_amd --decode --scale 2 write the host-mode bytes of the call; --sha1
    writes the digests of those bytes and the delivered sizes"""
    want = _call("i420", 2)
    srcs = [os.path.join(GOLDEN, STREAMS[0]), os.path.join(GOLDEN, STREAMS[1])]
    for k, cmd in enumerate(([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"])):
        d = tmp_path / str(k)
        d.mkdir()
        r = subprocess.run(cmd + ["--decode", "--scale", "2", str(d)] + srcs, capture_output=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
        for i, s in enumerate(srcs):
            assert open(str(d / (os.path.basename(s) + ".yuv")), "rb").read() == want[i][3], (cmd, s)
    d = tmp_path / "sha1"
    d.mkdir()
    r = subprocess.run([os.path.join(ROOT, "losslessh264_amd", "lh264dec"), "--decode", "--sha1", "--scale", "2", str(d), srcs[1]], capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()
    lines = open(str(d / (os.path.basename(srcs[1]) + ".sha1"))).read().split("\n")
    assert lines[0].split() == ["0", "76", "42", str(want[1][2][0][2]), str(want[1][2][0][3]), hashlib.sha1(want[1][3][:want[1][2][0][5]]).hexdigest()]
    assert lines[len(want[1][2])] == "stream " + hashlib.sha1(want[1][3]).hexdigest()
