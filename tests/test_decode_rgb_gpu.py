"""RGB pictures on the device: decode_pack_rgb_kernel on the directed windows of tests/test_decode_rgb.py (lh264_debug_rgb_dev) against
the same code stepped on the host and against the model, and lh264_decode_batch_ex with a colour against tests/rgb_model.py applied to
the I420 bytes of the same call without one - bytes, picture records, statuses, digests - in every mode of the call; which standard
a stream gets; the call without a colour is the call it was.  Every reference is computed once."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import rgb_model as M
import scale_cases as SC
from test_decode_rgb import JOBS, check_table, colour_stream, directed, run_table, slot_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK = 0
# QCIF CAVLC, QCIF CABAC, and the first 6 pictures (I, then P) of a CIF stream
STREAMS = ["streams/BA_MW_D.264", "streams/test_qcif_cabac.264", "streams/test_cif_P_CABAC_slice.264"]
CIF_PICTURES = 6
UNFLAGGED = ("bt601", "limited")                    # what a stream without a colour description gets
LAYOUTS = ["rgb24", "rgbp"]

_cache = {}


def _head(data, pictures):
    """the stream up to its first `pictures` pictures: cut in front of the slice NAL unit that begins the next one (first_mb_in_slice
    0: the bit behind the NAL header is set)"""
    seen, at = 0, 0
    while True:
        at = data.find(b"\x00\x00\x01", at)
        if at < 0:
            return data
        if data[at + 3] & 31 in (1, 5) and data[at + 4] & 0x80:
            seen += 1
            if seen > pictures:
                return data[:at - 1] if at and data[at - 1] == 0 else data[:at]
        at += 3


def _datas():
    if "datas" not in _cache:
        _cache["datas"] = [open(os.path.join(GOLDEN, n), "rb").read() for n in STREAMS]
        _cache["datas"][2] = _head(_cache["datas"][2], CIF_PICTURES)
    return _cache["datas"]


def _result(b, n, data=None):
    """what a call delivered, per stream: (status, text, picture records, bytes, source sizes, concealed)"""
    out = [(b.status(i), b.error(i), b.pictures(i), data[i] if data is not None else b.data(i), b.source_sizes(i), b.concealed(i)) for i in range(n)]
    b.free()
    return out


def _kw_key(kw):
    return tuple(sorted(kw.items()))


def _base(**kw):
    """ONE host-mode decode_batch over STREAMS without colour per set of keywords, shared by the tests"""
    if _kw_key(kw) not in _cache:
        import losslessh264_amd as lh
        _cache[_kw_key(kw)] = _result(lh.decode_batch(_datas(), **kw), len(STREAMS))
    return _cache[_kw_key(kw)]


def _expected(layout, std=UNFLAGGED, **kw):
    """the model applied to the bytes of the same call without colour -> per stream (bytes, records)"""
    key = ("x", layout, std, _kw_key(kw))
    if key not in _cache:
        _cache[key] = [M.rgb_packed(r[3], r[2], layout, std) for r in _base(**kw)]
    return _cache[key]


def _same(got, layout, what, std=UNFLAGGED, **kw):
    base, exp = _base(**kw), _expected(layout, std, **kw)
    for i, name in enumerate(STREAMS):
        assert got[i][0] == base[i][0] == OK and got[i][1] == base[i][1], (what, name, got[i][:2])
        assert got[i][2] == exp[i][1] and len(exp[i][1]) >= 1, (what, name)                 # width, height, frame_num, idr, offset, bytes
        assert got[i][3] == exp[i][0], (what, name)
        assert got[i][4] == base[i][4] and got[i][5] == base[i][5], (what, name)            # source sizes, concealed


# ---- 1: the kernel on the directed windows -------------------------------------------------------------------------------------------------
def test_rgb_pack_on_the_device():
    """every directed window under every sizing in both layouts, one launch of the production kernel per table of 16 jobs (destination
    offsets 0..3 x the four standards): the bytes are those of the same code stepped on the host, which are the model's, and the 0xA5
    around every destination is intact"""
    import torch
    from losslessh264_amd import _lib as L
    lib = L.lib()
    for name, case, sizings in directed():
        src = torch.from_numpy(case.buf).cuda()
        for sizing in sizings:
            slot = slot_bytes(case, sizing)
            for layout in LAYOUTS:
                host = np.full(slot * len(JOBS), 0xa5, dtype=np.uint8)
                placed = run_table(L, lib.lh264_debug_rgb_cpu, case, sizing, layout, case.buf.ctypes.data, host.ctypes.data, slot)
                dst = torch.full((slot * len(JOBS),), 0xa5, dtype=torch.uint8, device="cuda")
                assert dst.data_ptr() % 4 == 0
                torch.cuda.synchronize()
                run_table(L, lib.lh264_debug_rgb_dev, case, sizing, layout, src.data_ptr(), dst.data_ptr(), slot)
                got = dst.cpu().numpy()
                assert np.array_equal(got, host), (name, sizing, layout, np.flatnonzero(got != host)[:8])
                check_table(got, placed, (name, sizing, layout))


# ---- 2: the call against the model of the call without colour --------------------------------------------------------------------------
def test_the_streams_are_not_vacuous():
    base = _base()
    assert [r[0] for r in base] == [OK] * 3 and all(len(r[2]) >= 1 for r in base)
    assert {r[4][0] for r in base} == {(176, 144), (352, 288)} and [len(r[2]) for r in base] == [100, 30, CIF_PICTURES]
    import losslessh264_amd as lh
    assert [lh.stream_colour(d)[0] in (2, 5, 6) for d in _datas()] == [True] * 3          # nothing here asks for BT.709


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kw", [dict(), dict(scale=3), dict(size=(10, 6)), dict(size=(224, 224)), dict(pick="idr"), dict(parse="device+cabac"),
                                dict(round_pictures=3, threads=1)], ids=lambda kw: "-".join("%s=%s" % x for x in sorted(kw.items())) or "plain")
def test_the_call_delivers_the_model_of_its_output_without_colour(kw, layout):
    """full size, scale 3, two sizes, the IDR pick, the device parse route, other cuts of the work: the RGB bytes are the model of the
    I420 bytes of the same call without colour, the records describe them (3 * w * h bytes a picture), statuses and texts are that
    call's, and every picture says BT.601 limited"""
    import losslessh264_amd as lh
    b = lh.decode_batch(_datas(), colour=layout, **kw)
    cols = [b.colours(i) for i in range(3)]
    got = _result(b, 3)
    _same(got, layout, kw, **kw)
    for i in range(3):
        assert cols[i] == [UNFLAGGED] * len(got[i][2]) and all(p[5] == 3 * p[0] * p[1] for p in got[i][2])
    if kw == dict(size=(10, 6)):
        assert [(p[0], p[1], p[5]) for p in got[0][2]] == [(10, 6, 180)] * 100


def test_a_named_standard_is_applied():
    """matrix="bt709", colour_range="full" on unflagged streams: the model with that standard, and colours() says so"""
    import losslessh264_amd as lh
    b = lh.decode_batch(_datas(), colour="rgb24", matrix="bt709", colour_range="full", size=(46, 38))
    assert b.colours(1) == [("bt709", "full")] * len(b.pictures(1))
    _same(_result(b, 3), "rgb24", "named", std=("bt709", "full"), size=(46, 38))
    assert _expected("rgb24", ("bt709", "full"), size=(46, 38))[0][0] != _expected("rgb24", UNFLAGGED, size=(46, 38))[0][0]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_modes_deliver_the_host_mode_bytes(layout):
    """device output (tensor and frames shapes), a sink, digests with and without pictures, one conceal method"""
    import torch
    import losslessh264_amd as lh
    size, kw = (224, 224), dict(size=(224, 224))
    datas = _datas()
    exp = _expected(layout, **kw)
    b = lh.decode_batch(datas, colour=layout, device_out=True, **kw)
    frames = [b.frames(i) for i in range(3)]
    for i in range(3):
        n = len(exp[i][1])
        assert tuple(frames[i].shape) == ((n, 224, 224, 3) if layout == "rgb24" else (n, 3, 224, 224)) and frames[i].dtype == torch.uint8 and frames[i].is_cuda
        assert b.tensor(i).numel() == n * 3 * 224 * 224
    _same(_result(b, 3, [f.cpu().numpy().tobytes() for f in frames]), layout, "device_out", **kw)
    seen, recs = [[] for _ in range(3)], [[] for _ in range(3)]

    def sink(stream, first, pics, data):
        assert first == len(recs[stream]) and len(data) == sum(p[5] for p in pics)
        seen[stream].append(data)
        recs[stream] += pics
        return 0
    b = lh.decode_batch(datas, colour=layout, sink=sink, round_pictures=5, **kw)
    res = _result(b, 3, [b"".join(x) for x in seen])
    _same(res, layout, "sink", **kw)
    assert [r[2] for r in res] == recs
    b = lh.decode_batch(datas, colour=layout, sha1="both", pictures=False, **kw)
    for i in range(3):
        assert b.picture_sha1(i) == [hashlib.sha1(exp[i][0][p[4]:p[4] + p[5]]).digest() for p in exp[i][1]], STREAMS[i]
        assert b.stream_sha1(i) == hashlib.sha1(exp[i][0]).digest(), STREAMS[i]
        assert b.data(i) == b"" and b.pictures(i) == exp[i][1]
    b.free()
    b = lh.decode_batch(datas, colour=layout, sha1="both")                # ... and with the pictures, at full size
    full = _expected(layout)
    for i in range(3):
        assert b.stream_sha1(i) == hashlib.sha1(full[i][0]).digest() and b.data(i) == full[i][0], STREAMS[i]
    b.free()


def test_with_concealment():
    """the same pictures concealed as without colour; the delivered ones are the model of that call's"""
    import losslessh264_amd as lh
    data = open(os.path.join(GOLDEN, "conceal", "sva_mid5.264"), "rb").read()
    base = _result(lh.decode_batch([data], conceal="slice_copy"), 1)[0]
    assert len(base[2]) >= 1 and sum(base[5]) > 0
    for layout in LAYOUTS:
        got = _result(lh.decode_batch([data], conceal="slice_copy", colour=layout), 1)[0]
        exp = M.rgb_packed(base[3], base[2], layout, UNFLAGGED)
        assert got[:2] == base[:2] and got[2] == exp[1] and got[3] == exp[0] and got[4:] == base[4:], layout


# ---- 3: which standard a stream gets ---------------------------------------------------------------------------------------------------------
def test_a_batch_mixes_standards():
    """BA_MW_D.264 flagged BT.709 full range beside itself unflagged: the same planes convert differently, each as the model says, and
    colours() tells which"""
    import losslessh264_amd as lh
    plain = _datas()[0]
    flagged = colour_stream("BT.709 full range behind an extended SAR and overscan")
    base = _result(lh.decode_batch([flagged, plain], size=(22, 18)), 2)
    assert base[0][2:] == base[1][2:] and base[0][0] == base[1][0] == OK        # the VUI changes no sample
    for layout in LAYOUTS:
        b = lh.decode_batch([flagged, plain], colour=layout, size=(22, 18))
        assert b.colours(0) == [("bt709", "full")] * 100 and b.colours(1) == [UNFLAGGED] * 100
        got = _result(b, 2)
        assert got[0][3] == M.rgb_packed(base[0][3], base[0][2], layout, ("bt709", "full"))[0]
        assert got[1][3] == M.rgb_packed(base[1][3], base[1][2], layout, UNFLAGGED)[0]
        assert got[0][3] != got[1][3]
    # a named range overrides the flag, the matrix still comes from the stream
    b = lh.decode_batch([flagged], colour="rgb24", colour_range="limited", size=(22, 18))
    assert b.colours(0) == [("bt709", "limited")] * 100
    assert b.data(0) == M.rgb_packed(base[0][3], base[0][2], "rgb24", ("bt709", "limited"))[0]
    b.free()
    for name, std in (("BT.470BG", UNFLAGGED), ("SMPTE 170M, full range", ("bt601", "full")), ("unspecified", UNFLAGGED), ("BT.709", ("bt709", "limited"))):
        b = lh.decode_batch([colour_stream(name)], colour="rgbp", size=(22, 18))
        assert b.status(0) == OK and b.colours(0) == [std] * 100, name
        b.free()


def test_a_matrix_without_a_conversion_is_refused_and_can_be_named():
    """matrix_coefficients 9 under matrix="auto": LH264_E_UNSUPPORTED with a text that names the value, nothing delivered, the
    neighbours in the batch unharmed; under matrix="bt601" the stream converts; without colour it decodes as ever"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    plain, nine = _datas()[0], colour_stream("BT.2020")
    want = _expected("rgb24", size=(22, 18))[0]
    b = lh.decode_batch([plain, nine, plain], colour="rgb24", size=(22, 18))
    assert b.status(1) == L.E_UNSUPPORTED and "matrix_coefficients 9" in b.error(1) and b.pictures(1) == [] and b.data(1) == b"" and b.colours(1) == []
    for i in (0, 2):
        assert b.status(i) == OK and b.data(i) == want[0] and b.pictures(i) == want[1], i
    b.free()
    for kw in (dict(parse="device"), dict(pick="idr")):      # the routes that pick a round's pictures twice
        b = lh.decode_batch([nine], colour="rgb24", size=(22, 18), **kw)
        assert b.status(0) == L.E_UNSUPPORTED and "matrix_coefficients 9" in b.error(0) and b.pictures(0) == [], kw
        b.free()
    b = lh.decode_batch([nine], colour="rgb24", matrix="bt601", size=(22, 18))
    assert b.status(0) == OK and b.data(0) == want[0] and b.colours(0) == [UNFLAGGED] * 100
    b.free()
    b = lh.decode_batch([nine], size=(22, 18))
    assert b.status(0) == OK and b.data(0) == _base(size=(22, 18))[0][3]
    b.free()


def test_the_walk_changes_no_compressed_byte():
    """a stream with a VUI compresses to the tagged bytes of the stream without one; its default stream differs by the SPS it keeps"""
    import losslessh264_amd as lh
    plain, flagged = _datas()[0], colour_stream("BT.709 full range behind an extended SAR and overscan")
    (m0, t0, e0), (m1, t1, e1) = lh.compress_batch([plain, flagged])
    assert not e0 and not e1 and t0 == t1 and len(t0) >= 1
    assert len(m1) - len(m0) == len(flagged) - len(plain) and lh.restore(m1, t1) == flagged


# ---- 4: without a colour the call is what it was -----------------------------------------------------------------------------------------
def test_no_colour_is_what_it_was():
    """lh264_decode_batch_ex with ext == NULL, and with colour == 0, gives the bytes, the records and the launch shape
    (lh264_decode_last_chains) of lh264_decode_batch; a handle of such a call has no colour to tell"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    lib = L.lib()
    datas = _datas()
    n = len(datas)
    ptrs, lens = (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas])
    o = L.DecodeOptsV6()
    o.struct_bytes, o.round_pictures = 88, 4
    e = L.DecodeExt()
    e.struct_bytes = 24
    res, chains = [], []
    for call in (lambda outs: lib.lh264_decode_batch(ptrs, lens, n, 0, C.byref(o), outs), lambda outs: lib.lh264_decode_batch_ex(ptrs, lens, n, 0, C.byref(o), None, outs),
                 lambda outs: lib.lh264_decode_batch_ex(ptrs, lens, n, 0, C.byref(o), C.byref(e), outs)):
        outs = (C.c_void_p * n)()
        assert call(outs) == OK
        v = (C.c_longlong * 3)()
        assert lib.lh264_decode_last_chains(v) == OK
        chains.append(list(v))
        m, f = C.c_uint32(9), C.c_int32(9)
        assert lib.lh264_decoded_picture_colour(outs[0], 0, C.byref(m), C.byref(f)) == L.E_ARG
        res.append(_result(lh.DecodedBatch(lib, [outs[i] for i in range(n)], False), n))
    assert res[0] == res[1] == res[2] and chains[0] == chains[1] == chains[2] and chains[0][0] > 1
    assert [r[:5] for r in res[0]] == [r[:5] for r in _base()]


# ---- 5: the command lines ------------------------------------------------------------------------------------------------------------------
def test_the_command_lines_write_rgb(tmp_path):
    """lh264dec --decode --rgb rgb24 --size 22x18 and python -m losslessh264_amd --decode --rgb rgbp --matrix bt709 --range full write
    <name>.rgb, the bytes of the call; --sha1 writes their digests"""
    src = os.path.join(GOLDEN, STREAMS[0])
    name = os.path.basename(src)
    runs = [([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], ["--rgb", "rgb24"], _expected("rgb24", size=(22, 18))[0]),
            ([sys.executable, "-m", "losslessh264_amd"], ["--rgb", "rgbp", "--matrix", "bt709", "--range", "full"], _expected("rgbp", ("bt709", "full"), size=(22, 18))[0])]
    for k, (cmd, args, want) in enumerate(runs):
        d = tmp_path / str(k)
        d.mkdir()
        r = subprocess.run(cmd + ["--decode", "--size", "22x18"] + args + [str(d), src], capture_output=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
        assert os.listdir(str(d)) == [name + ".rgb"] and open(str(d / (name + ".rgb")), "rb").read() == want[0], cmd
    d = tmp_path / "sha1"
    d.mkdir()
    r = subprocess.run(runs[0][0] + ["--decode", "--sha1", "--size", "22x18", "--rgb", "rgb24", str(d), src], capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()
    lines = open(str(d / (name + ".sha1"))).read().split("\n")
    want = runs[0][2]
    assert lines[0].split()[:3] == ["0", "22", "18"] and lines[0].split()[5] == hashlib.sha1(want[0][:1188]).hexdigest()
    assert lines[100] == "stream " + hashlib.sha1(want[0]).hexdigest()
