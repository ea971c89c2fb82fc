"""Float RGB pictures on the device: decode_pack_sample_kernel on the windows of tests/test_decode_sample.py (lh264_debug_sample_dev)
against the same code stepped on the host and against the model, and lh264_decode_batch_ex2 with a float type against
tests/sample_model.py applied to the bytes of the same call with uint8 - bytes, picture records, statuses, source sizes, digests - in
every mode of the call; the typed frames; the call without a float type is the call it was.  Every reference is computed once."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import sample_model as SM
from test_decode_rgb_gpu import STREAMS, _datas, _kw_key, _result
from test_decode_sample import IMAGENET, JOBS, LAYOUTS, TYPES, _sample, check_table, factor_sets, run_table, slot_bytes, windows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK = 0
# a layout with a type each for the modes of the call; the whole matrix is the directed test's
PAIRS = [("rgb24", "float16"), ("rgbp", "bfloat16")]

_cache = {}


def _factors():
    import losslessh264_amd as lh
    return lh.normalise(*IMAGENET)


def _base(layout, **kw):
    """ONE host-mode decode_batch over STREAMS with colour and dtype uint8 per layout and set of keywords, shared by the tests"""
    key = (layout, _kw_key(kw))
    if key not in _cache:
        import losslessh264_amd as lh
        _cache[key] = _result(lh.decode_batch(_datas(), colour=layout, **kw), len(STREAMS))
    return _cache[key]


def _expected(layout, type_name, **kw):
    """the model applied to the bytes of the same call with uint8 -> per stream (bytes, records)"""
    key = ("x", layout, type_name, _kw_key(kw))
    if key not in _cache:
        mul, add = _factors()
        _cache[key] = [SM.apply(r[3], r[2], layout, type_name, mul, add) for r in _base(layout, **kw)]
    return _cache[key]


def _same(got, layout, type_name, what, **kw):
    base, exp = _base(layout, **kw), _expected(layout, type_name, **kw)
    es = SM.ELEMENT_BYTES[type_name]
    for i, name in enumerate(STREAMS):
        assert got[i][0] == base[i][0] == OK and got[i][1] == base[i][1], (what, name, got[i][:2])
        assert got[i][2] == exp[i][1] and len(exp[i][1]) >= 1, (what, name)                 # width, height, frame_num, idr, offset, bytes
        assert all(p[5] == 3 * p[0] * p[1] * es and p[4] % 4 == 0 for p in got[i][2]), (what, name)
        assert got[i][3] == exp[i][0], (what, name)
        assert got[i][4] == base[i][4] and got[i][5] == base[i][5], (what, name)            # source sizes, concealed


# ---- 1: the kernel on the directed windows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", TYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sample_pack_on_the_device(layout, type_name):
    """every window under every sizing with every factor set, one launch of the production kernel per table of 16 jobs (destinations 0,
    4, 8, 12 bytes from a 16-byte boundary x the four standards): the bytes are those of the same code stepped on the host, which are
    the model's, and the 0xA5 around every destination is intact - the fused multiply-add, the packed converts, ties, overflow,
    subnormals and the sign of zero as the device does them"""
    import torch
    from losslessh264_amd import _lib as L
    lib = L.lib()
    for name, case, sizings in windows():
        src = torch.from_numpy(case.buf).cuda()
        for sizing in sizings:
            slot = slot_bytes(case, sizing, type_name)
            for fname, mul, add in factor_sets(type_name):
                host = np.full(slot * len(JOBS) + 16, 0xa5, dtype=np.uint8)
                base = (-host.ctypes.data) % 16
                host = host[base:base + slot * len(JOBS)]
                placed = run_table(L, lib.lh264_debug_sample_cpu, case, sizing, layout, type_name, mul, add, case.buf.ctypes.data, host.ctypes.data, slot)
                dst = torch.full((slot * len(JOBS),), 0xa5, dtype=torch.uint8, device="cuda")
                assert dst.data_ptr() % 16 == 0
                torch.cuda.synchronize()
                run_table(L, lib.lh264_debug_sample_dev, case, sizing, layout, type_name, mul, add, src.data_ptr(), dst.data_ptr(), slot)
                got = dst.cpu().numpy()
                what = (name, sizing, layout, type_name, fname)
                assert np.array_equal(got, host), (what, np.flatnonzero(got != host)[:8])
                check_table(got, placed, what)


# ---- 2: the call against the model of the call with uint8 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(scale=3), dict(size=(64, 48)), dict(pick="idr")], ids=lambda kw: "-".join("%s=%s" % x for x in sorted(kw.items())) or "plain")
def test_the_call_delivers_the_model_of_its_output_with_uint8(kw):
    """full size, scale 3, one size, the IDR pick; host mode, a sink, device output and digests only: the float bytes are the model of
    the uint8 bytes of the same call, the records describe them (3 * w * h * es bytes a picture), statuses, texts and source sizes are
    that call's, and both digests are the delivered bytes'"""
    import losslessh264_amd as lh
    datas = _datas()
    mul, add = _factors()
    for layout, type_name in PAIRS:
        fkw = dict(kw, colour=layout, dtype=type_name, mul=mul, add=add)
        exp = _expected(layout, type_name, **kw)
        b = lh.decode_batch(datas, **fkw)
        assert b.dtype == type_name and b.affine == (mul, add)
        assert [lh._lib.lib().lh264_decoded_sample_type(h) for h in b._h] == [SM.TYPES[type_name]] * 3
        _same(_result(b, 3), layout, type_name, ("host", kw), **kw)
        seen, recs = [[] for _ in range(3)], [[] for _ in range(3)]

        def sink(stream, first, pics, data):
            assert first == len(recs[stream]) and len(data) == sum(p[5] for p in pics)
            seen[stream].append(data)
            recs[stream] += pics
            return 0
        b = lh.decode_batch(datas, sink=sink, round_pictures=5, **fkw)
        res = _result(b, 3, [b"".join(x) for x in seen])
        _same(res, layout, type_name, ("sink", kw), **kw)
        assert [r[2] for r in res] == recs
        b = lh.decode_batch(datas, device_out=True, **fkw)
        tensors = [b.tensor(i) for i in range(3)]
        assert all(t.dtype.is_floating_point is False and t.data_ptr() % 4 == 0 for t in tensors)
        _same(_result(b, 3, [t.cpu().numpy().tobytes() for t in tensors]), layout, type_name, ("device_out", kw), **kw)
        b = lh.decode_batch(datas, sha1="both", pictures=False, **fkw)
        for i in range(3):
            assert b.picture_sha1(i) == [hashlib.sha1(exp[i][0][p[4]:p[4] + p[5]]).digest() for p in exp[i][1]], (STREAMS[i], kw)
            assert b.stream_sha1(i) == hashlib.sha1(exp[i][0]).digest(), (STREAMS[i], kw)
            assert b.data(i) == b"" and b.pictures(i) == exp[i][1]
        b.free()


def test_the_arena_grows_by_the_delivered_bytes():
    """the round's two output buffers are what grows with the element size: for one stream in one round, es times the uint8 call's"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    data = _datas()[1]
    sizes = {}
    for dtype in ("uint8", "float16", "float32"):
        L.lib().lh264_decode_release()
        kw = dict(mul=(1, 1, 1)) if dtype != "uint8" else {}
        b = lh.decode_batch([data], colour="rgbp", size=(64, 48), dtype=dtype, sha1="stream", pictures=False, round_pictures=4, **kw)
        assert b.status(0) == OK
        b.free()
        sizes[dtype] = lh.decode_arena_bytes()[0]
    L.lib().lh264_decode_release()
    n = 4 * 3 * 64 * 48                                                     # a round of 4 pictures, uint8
    per_round = 2 * (n + n // 8)                                            # two buffers, each with the arena's headroom of an eighth
    assert sizes["float16"] - sizes["uint8"] == per_round and sizes["float32"] - sizes["uint8"] == 3 * per_round


# ---- 3: the typed frames ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_frames_are_typed_views(layout):
    """frames(i) has the dtype and the shape, equals frames(i) of the uint8 call put through the same table, and is a view of tensor(i)"""
    import torch
    import losslessh264_amd as lh
    datas = _datas()
    mul, add = _factors()
    b0 = lh.decode_batch(datas, colour=layout, size=(64, 48), device_out=True)
    u8 = [b0.frames(i).cpu().numpy() for i in range(3)]
    b0.free()
    ch = np.arange(3).reshape((1, 1, 1, 3) if layout == "rgb24" else (1, 3, 1, 1))
    for type_name, tt in (("float32", torch.float32), ("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        b = lh.decode_batch(datas, colour=layout, size=(64, 48), device_out=True, dtype=type_name, mul=mul, add=add)
        tab = SM.table(type_name, mul, add)
        for i in range(3):
            f, t = b.frames(i), b.tensor(i)
            n = u8[i].shape[0]
            assert n >= 1 and tuple(f.shape) == ((n, 48, 64, 3) if layout == "rgb24" else (n, 3, 48, 64)) and f.dtype == tt and f.is_cuda and t.dtype == torch.uint8
            assert f.data_ptr() == t.data_ptr() and t.numel() == f.numel() * f.element_size() and b.zero_copy
            bits = f.view(torch.int32 if type_name == "float32" else torch.int16).cpu().numpy().view(tab.dtype)
            assert np.array_equal(bits, tab[np.broadcast_to(ch, u8[i].shape), u8[i]]), (type_name, STREAMS[i])
        b.free()


# ---- 4: without a float type the call is what it was -----------------------------------------------------------------------------------------
def test_no_float_type_is_what_it_was():
    """lh264_decode_batch_ex2 with sample == NULL, and with type U8, gives the bytes, the records and the launch shape
    (lh264_decode_last_chains) of lh264_decode_batch_ex, with a colour and without one; such a handle says uint8"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    lib = L.lib()
    datas = _datas()
    n = len(datas)
    ptrs, lens = (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas])
    o = L.DecodeOptsV6()
    o.struct_bytes, o.round_pictures = 88, 4
    u8 = _sample(L)
    for colour in (0, 2):
        e = L.DecodeExt()
        e.struct_bytes, e.colour = 24, colour
        res, chains = [], []
        for call in (lambda outs: lib.lh264_decode_batch_ex(ptrs, lens, n, 0, C.byref(o), C.byref(e), outs),
                     lambda outs: lib.lh264_decode_batch_ex2(ptrs, lens, n, 0, C.byref(o), C.byref(e), None, outs),
                     lambda outs: lib.lh264_decode_batch_ex2(ptrs, lens, n, 0, C.byref(o), C.byref(e), C.byref(u8), outs)):
            outs = (C.c_void_p * n)()
            assert call(outs) == OK
            v = (C.c_longlong * 3)()
            assert lib.lh264_decode_last_chains(v) == OK
            chains.append(list(v))
            assert [lib.lh264_decoded_sample_type(outs[i]) for i in range(n)] == [0] * n
            res.append(_result(lh.DecodedBatch(lib, [outs[i] for i in range(n)], False), n))
        assert res[0] == res[1] == res[2] and chains[0] == chains[1] == chains[2] and chains[0][0] > 1, colour
        if colour:
            assert [r[:5] for r in res[0]] == [r[:5] for r in _base("rgbp")]
    # a float call has the same launch shape: the kernel takes the RGB kernel's place
    s = _sample(L, type=2, mul=(1.0, 1.0, 1.0))
    outs = (C.c_void_p * n)()
    assert lib.lh264_decode_batch_ex2(ptrs, lens, n, 0, C.byref(o), C.byref(e), C.byref(s), outs) == OK
    v = (C.c_longlong * 3)()
    assert lib.lh264_decode_last_chains(v) == OK and list(v) == chains[0]
    assert [lib.lh264_decoded_sample_type(outs[i]) for i in range(n)] == [2] * n
    for i in range(n):
        lib.lh264_decoded_free(outs[i])


# ---- 5: the command line -------------------------------------------------------------------------------------------------------------------
def test_the_command_line_writes_float_pictures(tmp_path):
    """lh264dec --decode --rgb rgbp --sample f16 --mul .. --add .. --size 22x18 writes <name>.f16, the model's bytes"""
    src = os.path.join(GOLDEN, STREAMS[0])
    name = os.path.basename(src)
    mul, add = _factors()
    base = _base("rgbp", size=(22, 18))[0]
    want = SM.apply(base[3], base[2], "rgbp", "float16", mul, add)[0]
    text = lambda v: ",".join("%.9g" % x for x in v)
    r = subprocess.run([os.path.join(ROOT, "losslessh264_amd", "lh264dec"), "--decode", "--size", "22x18", "--rgb", "rgbp", "--sample", "f16", "--mul", text(mul), "--add", text(add), str(tmp_path), src],
                       capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    assert os.listdir(str(tmp_path)) == [name + ".f16"] and open(str(tmp_path / (name + ".f16")), "rb").read() == want
    assert len(want) == 100 * 3 * 22 * 18 * 2
