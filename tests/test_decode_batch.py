"""lh264_decode_batch without a device: the exports and the argument / no-device behaviour, the sparse coefficient list of the
front end against its dense planes on every committed stream, and the pack kernel's code stepped over host memory
(lh264_debug_pack_cpu) against numpy and against the oracle's pictures."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")


def _lib():
    import __graft_entry__ as g
    g.build()
    from losslessh264_amd import _lib as L
    return L, L.lib()


def _opts(L, **kw):
    o = L.DecodeOpts()
    o.struct_bytes = C.sizeof(L.DecodeOpts)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_exports_and_argument_checks():
    L, lib = _lib()
    for name in ("lh264_decode_batch", "lh264_decoded_status", "lh264_decoded_error", "lh264_decoded_pictures", "lh264_decoded_picture",
                 "lh264_decoded_bytes", "lh264_decoded_bytes_dev", "lh264_decoded_free", "lh264_decode_arena_bytes", "lh264_decode_release",
                 "lh264_debug_pack_cpu", "lh264_parser_set_sparse_coeffs", "lh264_parser_frame_sparse_coeffs"):
        assert hasattr(lib, name), name
    import losslessh264_amd as lh
    assert callable(lh.decode_batch)
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    ptrs = (C.c_char_p * 1)(data)
    lens = (C.c_size_t * 1)(len(data))
    sentinel = 0x5a5a5a5a
    outs = (C.c_void_p * 1)(sentinel)

    @L.DECODE_SINK_FN
    def sink(*a):
        return 0
    bad = [_opts(L, struct_bytes=8), _opts(L, format=2), _opts(L, flags=L.DECODE_DEVICE_OUT, sink=sink), _opts(L, flags=2)]
    for o in bad:
        assert lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(o), outs) == L.E_ARG
        assert outs[0] == sentinel
    assert lib.lh264_decode_batch(ptrs, lens, -1, 1, None, outs) == L.E_ARG
    assert lib.lh264_decode_batch(None, lens, 1, 1, None, outs) == L.E_ARG
    assert outs[0] == sentinel


def test_no_device_is_reported_with_out_untouched():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L, lib = _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    ptrs = (C.c_char_p * 1)(data)
    lens = (C.c_size_t * 1)(len(data))
    sentinel = 0x5a5a5a5a
    outs = (C.c_void_p * 1)(sentinel)
    assert lib.lh264_decode_batch(ptrs, lens, 1, 1, None, outs) == L.E_NODEVICE
    o = _opts(L, format=L.FMT_NV12)
    assert lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(o), outs) == L.E_NODEVICE
    assert outs[0] == sentinel
    import losslessh264_amd as lh
    with pytest.raises(RuntimeError):
        lh.decode_batch([data])


def _parse(L, lib, data, sparse):
    """-> parser handle after lh264_parser_feed_file"""
    p = lib.lh264_parser_create()
    if sparse:
        L.check(lib.lh264_parser_set_sparse_coeffs(p, 1))
    lib.lh264_parser_feed_file(p, data, len(data))
    return p


def test_sparse_coefficients_equal_dense_coefficients():
    """every committed stream, every picture: the list scattered into zeros = the dense planes; sorted, no zero value; records, slices
    and frame infos identical between the two parses"""
    L, lib = _lib()
    files = sorted(glob.glob(os.path.join(STREAMS, "*")))
    n_files = n_pics = n_entries = 0
    for path in files:
        data = open(path, "rb").read()
        pd, ps = _parse(L, lib, data, False), _parse(L, lib, data, True)
        try:
            assert lib.lh264_parser_error(pd) == b"", (os.path.basename(path), lib.lh264_parser_error(pd))
            assert lib.lh264_parser_error(ps) == lib.lh264_parser_error(pd)
            n = lib.lh264_parser_frame_count(pd)
            assert n == lib.lh264_parser_frame_count(ps) and n > 0, path
            for i in range(n):
                a, b = np.zeros(1, dtype=L.FRAME_INFO_DTYPE), np.zeros(1, dtype=L.FRAME_INFO_DTYPE)
                L.check(lib.lh264_parser_frame_info(pd, i, a.ctypes.data_as(C.c_void_p)))
                L.check(lib.lh264_parser_frame_info(ps, i, b.ctypes.data_as(C.c_void_p)))
                assert a.tobytes() == b.tobytes(), (path, i)
                mbs, ns = int(a[0]["mb_w"]) * int(a[0]["mb_h"]), int(a[0]["n_slices"])
                assert C.string_at(lib.lh264_parser_frame_mbs(pd, i), mbs * 128) == C.string_at(lib.lh264_parser_frame_mbs(ps, i), mbs * 128), (path, i)
                assert C.string_at(lib.lh264_parser_frame_slices(pd, i), ns * 232) == C.string_at(lib.lh264_parser_frame_slices(ps, i), ns * 232), (path, i)
                dense = np.frombuffer(C.string_at(lib.lh264_parser_frame_coeffs(pd, i), mbs * 768), dtype="<i2")
                assert not lib.lh264_parser_frame_coeffs(ps, i)
                cnt = C.c_size_t(0)
                ptr = lib.lh264_parser_frame_sparse_coeffs(ps, i, C.byref(cnt))
                ents = np.frombuffer(C.string_at(ptr, cnt.value * 8), dtype="<u8") if cnt.value else np.zeros(0, dtype="<u8")
                idx = (ents >> np.uint64(16)).astype(np.int64)
                val = (ents & np.uint64(0xffff)).astype(np.uint16).view(np.int16)
                assert np.all(val != 0), (path, i)
                assert np.all(np.diff(idx) > 0), (path, i)
                assert cnt.value == 0 or (idx[0] >= 0 and idx[-1] < mbs * 384), (path, i)
                got = np.zeros(mbs * 384, dtype=np.int16)
                got[idx] = val
                assert np.array_equal(got, dense), (path, i)
                n_pics += 1
                n_entries += cnt.value
        finally:
            lib.lh264_parser_destroy(pd)
            lib.lh264_parser_destroy(ps)
        n_files += 1
    print("%d files, %d pictures, %d list entries" % (n_files, n_pics, n_entries))
    assert n_files == 48


def _pack(L, lib, y, u, v, crop, fmt, dst, at):
    """y/u/v: 2-D uint8 arrays (views into padded planes, pixel (0,0) at [0,0]); packs the window into dst[at:]"""
    x0, y0, w, h = crop
    j = L.PackJob()
    j.y, j.u, j.v = y.ctypes.data, u.ctypes.data, v.ctypes.data
    j.dst = dst.ctypes.data + at
    j.stride_y, j.stride_c = y.strides[0], u.strides[0]
    assert v.strides[0] == u.strides[0]
    j.crop_x, j.crop_y, j.crop_w, j.crop_h, j.format = x0, y0, w, h, fmt
    assert lib.lh264_debug_pack_cpu(C.byref(j), 1) == 0


def _expect(y, u, v, crop, fmt):
    x0, y0, w, h = crop
    Y = y[y0:y0 + h, x0:x0 + w]
    U = u[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]
    V = v[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]
    if fmt == 0:
        return np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)])
    return np.concatenate([Y.reshape(-1), np.stack([U, V], axis=-1).reshape(-1)])


@pytest.mark.parametrize("name", ["CVFC1_Sony_C.jsv", "Static.264", "BA_MW_D.264"])
def test_pack_on_the_host_against_the_oracle(name):
    """the first 10 pictures reconstructed by the oracle, their padded pictures packed by the kernel's code on the host: I420 = the
    numpy crop of the oracle's planes, NV12 = its interleave"""
    L, lib = _lib()
    import losslessh264_amd as lh
    frames, err, _ = lh.parse_file(open(os.path.join(STREAMS, name), "rb").read())
    assert err == "" and len(frames) >= 10
    pics = {}
    if name == "CVFC1_Sony_C.jsv":
        assert (frames[0].crop_x, frames[0].crop_y, frames[0].crop_w, frames[0].crop_h) == (26, 60, 300, 168)
    if name == "Static.264":
        assert (frames[0].crop_w, frames[0].crop_h) == (152, 100)
    for f in frames[:10]:
        dst = O.HostPic(f.mb_w, f.mb_h)
        refs = [pics.get(r, dst) for r in f.ref_ids]
        O.recon_frame(f.mbs, f.coeffs, f.slices, dst, refs, 0)
        pics[f.id] = dst
        crop = (f.crop_x, f.crop_y, f.crop_w, f.crop_h)
        n = f.crop_w * f.crop_h * 3 // 2
        for fmt in (L.FMT_I420, L.FMT_NV12):
            for at in (64, 70):          # an aligned and an unaligned destination
                out = np.full(n + 192, 0xa5, dtype=np.uint8)
                _pack(L, lib, dst.plane(0), dst.plane(1), dst.plane(2), crop, fmt, out, at)
                assert np.array_equal(out[at:at + n], _expect(dst.plane(0), dst.plane(1), dst.plane(2), crop, fmt)), (name, f.id, fmt, at)
                assert np.all(out[:at] == 0xa5) and np.all(out[at + n:] == 0xa5)


@pytest.mark.parametrize("crop_x", [0, 2, 6, 18])
@pytest.mark.parametrize("crop_w", [2, 14, 16, 18, 174, 1918])
def test_pack_on_the_host_synthetic_geometries(crop_x, crop_w):
    """windows that start off the 16-byte grid and rows shorter than, equal to and longer than a piece, both formats, several
    destination alignments, guard bytes around the destination"""
    L, lib = _lib()
    rng = np.random.default_rng(1000 * crop_x + crop_w)
    mb_w = (crop_x + crop_w + 15) // 16
    for crop_y, crop_h, mb_h in ((0, 2, 1), (4, 22, 2), (2, 46, 3)):
        sy, sc, oy, ou, ov, total = O.pic_geometry(mb_w, mb_h)
        pic = O.HostPic(mb_w, mb_h)
        pic.buf[:] = rng.integers(0, 256, total, dtype=np.uint8)
        crop = (crop_x, crop_y, crop_w, crop_h)
        n = crop_w * crop_h * 3 // 2
        for fmt in (L.FMT_I420, L.FMT_NV12):
            for at in (64, 66, 78):
                out = np.full(n + 192, 0x3c, dtype=np.uint8)
                _pack(L, lib, pic.plane(0), pic.plane(1), pic.plane(2), crop, fmt, out, at)
                assert np.array_equal(out[at:at + n], _expect(pic.plane(0), pic.plane(1), pic.plane(2), crop, fmt)), (crop, fmt, at)
                assert np.all(out[:at] == 0x3c) and np.all(out[at + n:] == 0x3c), (crop, fmt, at)


def test_pack_rejects_bad_jobs():
    L, lib = _lib()
    assert lib.lh264_debug_pack_cpu(None, 1) == L.E_ARG
    j = L.PackJob()
    assert lib.lh264_debug_pack_cpu(C.byref(j), 1) == L.E_ARG
