"""Decoding the pictures asked for by number (decode_batch (select=)) on the device.  The yardstick is exact and the project's own:
every delivered picture is byte for byte that picture of the call without select, which the other decode tests hold to the reference.
One full call over the committed streams and one host-mode selected call over the parity batch are computed once per module; every
other call is held to them.  What is new on the device - runs as chains of their own, pictures that are reconstructed only, streams
that end early - is held by the bytes, by parsed_slices and chain_pictures, and by lh264_decode_last_chains."""
import collections
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scale_ref
import select_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK = 0
BA, MIDR, LOST = "streams/BA_MW_D.264", "streams/MIDR_MW_D.264", "streams/BA_MW_D_IDR_LOST.264"
# the parity batch: (stream, its selection)
BATCH = [(BA, [0]), (BA, [29]), (BA, [30]), (BA, [31, 59]), (BA, [5, 35, 65, 95]), (BA, [99]), (BA, [98, 99, 100, 500]), (BA, None),
         (MIDR, [45]), (MIDR, [60]), (MIDR, [89, 91]), (LOST, [10]), (LOST, [27]), ("streams/MR1_BT_A.h264", [7, 40]),
         ("streams/CVFC1_Sony_C.jsv", [12]), ("streams/test_qcif_cabac.264", slice(0, None, 9)), ("cabac_edge/cabac_skip.264", [2, 4])]
NAMES = sorted(set(name for name, _ in BATCH))

R = collections.namedtuple("R", "status error pics data src index parsed chain psha ssha")
_cache = {}


def _read(name):
    if name not in _cache:
        _cache[name] = open(os.path.join(GOLDEN, name), "rb").read()
    return _cache[name]


def _result(b, n, data=None, sha=True):
    out = []
    for i in range(n):
        out.append(R(b.status(i), b.error(i), b.pictures(i), data[i] if data is not None else b.data(i), b.source_sizes(i), b.picture_indices(i),
                     b.parsed_slices(i), b.chain_pictures(i), b.picture_sha1(i) if sha else None, b.stream_sha1(i) if sha else None))
    b.free()
    return out


def _full(fmt="i420"):
    """ONE call without select over the streams of the batch per format, with both digests: name -> R"""
    if ("full", fmt) not in _cache:
        import losslessh264_amd as lh
        _cache[("full", fmt)] = dict(zip(NAMES, _result(lh.decode_batch([_read(n) for n in NAMES], fmt=fmt, sha1="both"), len(NAMES))))
    return _cache[("full", fmt)]


def _selected(**kw):
    import losslessh264_amd as lh
    return _result(lh.decode_batch([_read(n) for n, _ in BATCH], select=[s for _, s in BATCH], sha1="both", **kw), len(BATCH))


def _host():
    """ONE host-mode selected call over the parity batch, shared by the tests"""
    if "host" not in _cache:
        _cache["host"] = _selected()
    return _cache["host"]


def _plan(name, sel):
    """(needed, delivered) by the model, from where the header walk finds the IDR pictures"""
    import losslessh264_amd as lh
    key = ("idr", name)
    if key not in _cache:
        _cache[key] = (lh.pick(_read(name), "idr"), len(lh.pick(_read(name), "all")))
    return select_model.model(_cache[key][0], _cache[key][1], sel)


def _slice_counts(name):
    if ("slices", name) not in _cache:
        import losslessh264_amd as lh
        _cache[("slices", name)] = [len(f.slices) for f in lh.parse_file(_read(name))[0]]
    return _cache[("slices", name)]


def _cut_from(full, index):
    """the pictures `index` of a full call's result -> (records with offsets of their own, bytes, source sizes, picture digests)"""
    pics, data, off = [], [], 0
    for k in index:
        w, h, fn, idr, o, n = full.pics[k]
        pics.append((w, h, fn, idr, off, n))
        data.append(full.data[o:o + n])
        off += n
    return pics, b"".join(data), [full.src[k] for k in index], [full.psha[k] for k in index]


def _check(got, full, index, what, digests=True, data=True):
    pics, bytes_, src, psha = _cut_from(full, index)
    assert got.index == index, (what, got.index)
    assert got.pics == pics and got.src == src, what
    if data:
        assert got.data == bytes_, what
    if digests:
        assert got.psha == psha and got.ssha == hashlib.sha1(bytes_).digest(), what


# ---- 1: parity ------------------------------------------------------------------------------------------------------------------------------
def test_selected_pictures_are_the_full_call_s():
    """host mode, I420: bytes, records, source sizes, per-picture SHA-1 and picture_indices are the full call's at the numbers asked for;
    the stream SHA-1 is hashlib's of the delivered bytes; chain_pictures counts the needed pictures, parsed_slices their slices"""
    full, got = _full(), _host()
    for name in NAMES:
        assert full[name].status == OK and full[name].index == list(range(len(full[name].pics))), (name, full[name].error)
    for (name, sel), g in zip(BATCH, got):
        needed, delivered = _plan(name, sel)
        what = (name, sel)
        assert delivered and (g.status, g.error) == (OK, ""), (what, g.error)
        _check(g, full[name], delivered, what)
        assert g.ssha == hashlib.sha1(g.data).digest(), what
        assert g.chain == len(needed), (what, g.chain)
        assert g.parsed == sum(_slice_counts(name)[k] for k in needed), (what, g.parsed)
    by = {(n, str(s)): g for (n, s), g in zip(BATCH, got)}
    assert by[(BA, "[31, 59]")].chain == 30 and by[(BA, "[98, 99, 100, 500]")].index == [98, 99] and by[(BA, "[98, 99, 100, 500]")].chain == 10
    assert by[(MIDR, "[45]")].chain == 46 and by[(MIDR, "[60]")].chain == 1 and by[(MIDR, "[89, 91]")].chain == 32
    assert by[(LOST, "[10]")].chain == 11 and by[(LOST, "[27]")].chain == 1
    assert by[(BA, "None")] == full[BA]._replace(chain=100)
    assert full[BA].chain == 100
    assert [p[:2] for p in by[("cabac_edge/cabac_skip.264", "[2, 4]")].pics] == [full["cabac_edge/cabac_skip.264"].pics[2][:2], (16, 16)]      # a change of size at an IDR picture


# ---- 2: damage ------------------------------------------------------------------------------------------------------------------------------
def _cut_slice(data, picture):
    """BA_MW_D.264 (one slice per picture) with the slice NAL unit of `picture` cut to half its payload, its header kept"""
    starts = [m.start() for m in re.finditer(b"\x00\x00\x01", data)]
    slices = [s for s in starts if data[s + 3] & 31 in (1, 5)]
    assert len(slices) == 100
    at = slices[picture]
    nxt = min(s for s in starts + [len(data)] if s > at)
    if nxt < len(data) and data[nxt - 1] == 0:
        nxt -= 1                                          # (a four-byte start code)
    payload = nxt - (at + 4)
    assert payload > 16
    return data[:at + 4 + payload // 2] + data[nxt:]


def _header_failure_stream():
    """BA_MW_D.264 with the slice of picture 45 turned into a B slice: the header walk fails with 44 pictures complete"""
    data = _read(BA)
    starts = [m.start() for m in re.finditer(b"\x00\x00\x01", data)]
    slices = [s for s in starts if data[s + 3] & 31 in (1, 5)]
    at = slices[45]
    return data[:at + 4] + b"\xa8" + data[at + 5:]


@pytest.mark.parametrize("kw", [dict(), dict(parse="device")], ids=["host", "device"])
def test_damage_where_nothing_is_needed_is_not_seen(kw):
    """a slice cut short in a picture that is not needed, or behind the last requested one, does not show; in a needed picture it stops
    the stream with the full call's text, the requested pictures in front of it delivered; the same for a slice header that fails"""
    import losslessh264_amd as lh
    clean = _full()[BA]
    cut10, cut50, hdr = _cut_slice(_read(BA), 10), _cut_slice(_read(BA), 50), _header_failure_stream()
    f10, f50, fh = _result(lh.decode_batch([cut10, cut50, hdr], sha1="both"), 3)
    assert f10.error.startswith("picture 10: ") and f50.error.startswith("picture 50: ") and fh.error.startswith("picture 44: ") and len(fh.pics) == 44
    datas = [cut10, cut50, cut50, hdr, hdr, hdr]
    sels = [[35], [35], [35, 55], [35], [65], [43]]
    got = _result(lh.decode_batch(datas, select=sels, sha1="both", **kw), len(datas))
    for k in (0, 1, 3):
        assert (got[k].status, got[k].error) == (OK, ""), (k, got[k].error)
        _check(got[k], clean, [35], k)
        assert got[k].chain == 6 and got[k].parsed == 6
    assert (got[2].status, got[2].error) == (f50.status, f50.error)
    _check(got[2], clean, [35], "picture 50 cut, [35, 55]")
    assert (got[4].status, got[4].error) == (fh.status, fh.error) and got[4].index == [] and got[4].chain == 0
    assert (got[5].status, got[5].error) == (OK, "")          # (picture 43 ends where picture 44 begins, in front of the failure)
    _check(got[5], clean, [43], "[43]")


# ---- 3: cuts and routes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(parse="device"), dict(parse="device+cabac"), dict(round_pictures=1), dict(round_pictures=3), dict(round_pictures=8),
                                dict(group_mbs=600), dict(threads=1)], ids=lambda kw: ",".join("%s=%s" % kv for kv in sorted(kw.items())))
def test_the_cuts_of_the_work_and_the_routes_do_not_show(kw):
    """the parity batch under the device parse routes, round_pictures 1, 3 and 8, a group_mbs that makes streams wait, one thread: the
    host-mode result, digests and counts included"""
    res, want = _selected(**kw), _host()
    for (name, sel), g, w in zip(BATCH, res, want):
        assert g == w, (kw, name, sel, g.error)


# ---- 4: modes -------------------------------------------------------------------------------------------------------------------------------
def test_nv12_and_a_reduced_size():
    """NV12: the selected pictures of the NV12 full call.  scale 2: tests/scale_ref.py applied to the selected full-size bytes"""
    full, got = _full("nv12"), _selected(fmt="nv12")
    for (name, sel), g in zip(BATCH, got):
        assert (g.status, g.error) == (OK, "")
        _check(g, full[name], _plan(name, sel)[1], ("nv12", name, sel))
    assert any(g.data != h.data for g, h in zip(got, _host()))
    res = _selected(scale=2)
    for (name, sel), g, base in zip(BATCH, res, _host()):
        data, pics = scale_ref.scale_packed(base.data, base.pics, "i420", 2)
        assert (g.status, g.error, g.index, g.src, g.chain, g.parsed) == (OK, "", base.index, base.src, base.chain, base.parsed), (name, sel)
        assert g.pics == pics and g.data == data, (name, sel)
        assert g.ssha == hashlib.sha1(data).digest() and g.psha == [hashlib.sha1(data[p[4]:p[4] + p[5]]).digest() for p in pics], (name, sel)


def test_clips_as_float_tensors():
    """size, cover, RGB, float16, device_out and four pictures per stream in one call: frames (i) is the call without select indexed at
    the numbers, and the batch stacks to (N, T, H, W, 3)"""
    import torch
    import losslessh264_amd as lh
    names = [BA, MIDR, "streams/MR1_BT_A.h264", "streams/CVFC1_Sony_C.jsv"]
    sels = [[4, 29, 54, 91], slice(10, 50, 10), [0, 1, 30, 61], slice(46, None)]
    datas = [_read(n) for n in names]
    kw = dict(size=(64, 48), fit="cover", colour="rgb24", dtype="float16", mul=(1 / 255.0,) * 3, add=(-0.5, 0.25, 0.0), device_out=True)
    full = lh.decode_batch(datas, **kw)
    got = lh.decode_batch(datas, select=sels, **kw)
    clips = []
    for i, (name, sel) in enumerate(zip(names, sels)):
        idx = _plan(name, sel)[1]
        assert len(idx) == 4 and got.status(i) == OK and got.picture_indices(i) == idx, (name, got.error(i))
        f = got.frames(i)
        assert f.dtype == torch.float16 and tuple(f.shape) == (4, 48, 64, 3)
        assert torch.equal(f.view(torch.int16), full.frames(i)[idx].view(torch.int16)), name
        assert got.views(i) == [full.views(i)[k] for k in idx] and got.colours(i) == [full.colours(i)[k] for k in idx]
        clips.append(f)
    assert tuple(torch.stack(clips).shape) == (4, 4, 48, 64, 3)
    full.free()
    got.free()


def test_a_sink_and_digests_only():
    """a sink: runs of consecutive delivered pictures, first_picture counts delivered pictures.  pictures=False with both digests"""
    import losslessh264_amd as lh
    n = len(BATCH)
    datas, sels = [_read(nm) for nm, _ in BATCH], [s for _, s in BATCH]
    seen, recs = [[] for _ in range(n)], [[] for _ in range(n)]

    def sink(stream, first, pics, data):
        assert first == len(recs[stream]) and len(pics) >= 1 and len(data) == sum(p[5] for p in pics)
        seen[stream].append(data)
        recs[stream] += pics
        return 0
    b = lh.decode_batch(datas, select=sels, sink=sink, round_pictures=2, sha1="both")
    assert [b.data(i) for i in range(n)] == [b""] * n
    res = _result(b, n, [b"".join(x) for x in seen])
    assert res == _host() and [r.pics for r in res] == recs
    res = _result(lh.decode_batch(datas, select=sels, sha1="both", pictures=False), n)
    assert all(r.data == b"" for r in res)
    assert [r._replace(data=None) for r in res] == [r._replace(data=None) for r in _host()]
    b = lh.decode_batch(datas, select=sels, device_out=True, sha1="both")
    assert _result(b, n, [b.tensor(i).cpu().numpy().tobytes() for i in range(n)]) == _host()


# ---- 5: fields ------------------------------------------------------------------------------------------------------------------------------
def test_fields_of_selected_pictures():
    """motion=True: motion (i) and mb_info (i) are the full call's at the numbers, `back` - which counts pictures of the stream -
    included; the motion-only call gives the same fields and launches no reconstruct kernel"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    datas, sels = [_read(BA), _read(BA), _read("streams/MR1_BT_A.h264")], [[31, 59], [5, 35], [7, 40]]
    full = lh.decode_batch(datas[1:], motion=True)
    want = [([full.motion(i)[k] for k in s], [full.mb_info(i)[k] for k in s]) for i, s in ((0, sels[0]), (0, sels[1]), (1, sels[2]))]
    want_data = [b"".join(full.data(i)[full.pictures(i)[k][4]:full.pictures(i)[k][4] + full.pictures(i)[k][5]] for k in s) for i, s in ((0, sels[0]), (0, sels[1]), (1, sels[2]))]
    assert int(want[0][0][0][2].max()) >= 1 and int(want[2][0][1][2].max()) >= 1      # P pictures: some block predicts from a picture back
    v = (C.c_longlong * 3)()
    for kw in (dict(), dict(pictures=False), dict(parse="device"), dict(pictures=False, round_pictures=3)):
        got = lh.decode_batch(datas, select=sels, motion=True, **kw)
        assert L.lib().lh264_decode_last_chains(v) == OK
        for i, s in enumerate(sels):
            assert got.status(i) == OK and got.picture_indices(i) == s, (kw, got.error(i))
            mot, mbi = got.motion(i), got.mb_info(i)
            assert len(mot) == len(s) and all(np.array_equal(a, b) for a, b in zip(mot, want[i][0])), (kw, i)
            assert len(mbi) == len(s) and all(np.array_equal(a, b) for a, b in zip(mbi, want[i][1])), (kw, i)
            assert got.data(i) == (b"" if "pictures" in kw else want_data[i]), (kw, i)
        if "pictures" in kw:
            assert tuple(v) == (0, 0, 0) and [got.chain_pictures(i) for i in range(3)] == [0, 0, 0]
        else:
            assert tuple(v)[0] >= 1 and [got.chain_pictures(i) for i in range(3)] == [30, 12, 41]
        got.free()
    full.free()


# ---- 6: the launch shape --------------------------------------------------------------------------------------------------------------------
def test_a_chain_per_run():
    """BA_MW_D.264 alone, [1, 31, 61, 91], round_pictures 8: one round, four runs of two pictures, each a chain of its own.  Without
    select the stream is one chain per round, as ever"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    v = (C.c_longlong * 3)()
    r = _result(lh.decode_batch([_read(BA)], select=[1, 31, 61, 91], round_pictures=8, sha1="both"), 1)[0]
    assert L.lib().lh264_decode_last_chains(v) == OK and tuple(v) == (1, 4, 8)
    _check(r, _full()[BA], [1, 31, 61, 91], "runs")
    assert r.chain == 8 and r.parsed == 8
    r = _result(lh.decode_batch([_read(BA)], round_pictures=8, sha1="both"), 1)[0]
    assert L.lib().lh264_decode_last_chains(v) == OK and tuple(v) == (13, 13, 100)
    assert r == _full()[BA]
    # a run that spans rounds goes on as the stream's chain: 30..35 in rounds of four is 30..33 then 34, 35
    r = _result(lh.decode_batch([_read(BA)], select=[35], round_pictures=4, sha1="both"), 1)[0]
    assert L.lib().lh264_decode_last_chains(v) == OK and tuple(v) == (2, 2, 6)
    _check(r, _full()[BA], [35], "a run over two rounds")


# ---- 7: the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_ex5_without_a_selection_is_ex4():
    """lh264_decode_batch_ex5 with select = NULL and with n_selects = 0: the results and the launch shape of lh264_decode_batch_ex4"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    lib = L.lib()
    datas = [_read(n) for n in NAMES]
    n = len(datas)
    ptrs, lens = (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas])
    o = L.DecodeOptsV6()
    o.struct_bytes, o.flags = C.sizeof(L.DecodeOptsV6), L.DECODE_SHA1_PICTURES | L.DECODE_SHA1_STREAM
    none = L.DecodeSelect()
    none.struct_bytes = C.sizeof(L.DecodeSelect)
    v = (C.c_longlong * 3)()
    shapes, results = [], []
    for sel in ("ex4", None, none):
        outs = (C.c_void_p * n)()
        if sel == "ex4":
            assert lib.lh264_decode_batch_ex4(ptrs, lens, n, 0, C.byref(o), None, None, None, None, outs) == OK
        else:
            assert lib.lh264_decode_batch_ex5(ptrs, lens, n, 0, C.byref(o), None, None, None, None, C.byref(sel) if sel is not None else None, outs) == OK
        assert lib.lh264_decode_last_chains(v) == OK
        shapes.append(tuple(v))
        results.append(_result(lh.DecodedBatch(lib, [outs[i] for i in range(n)], False), n))
    assert shapes[0] == shapes[1] == shapes[2] and shapes[0][1] >= n
    assert results[0] == results[1] == results[2] == [_full()[nm] for nm in NAMES]


# ---- 8: the command lines -------------------------------------------------------------------------------------------------------------------
def test_the_command_lines_take_at(tmp_path):
    """lh264dec --decode --sha1 --at 5,35,65,95 and the Python module write identical .sha1 files whose index column is 5 35 65 95;
    --at 0::25 without --sha1 writes the selected bytes"""
    src = os.path.join(GOLDEN, BA)
    full = _full()[BA]
    pics, data, _src, psha = _cut_from(full, [5, 35, 65, 95])
    texts = []
    for k, cmd in enumerate(([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"])):
        d = tmp_path / str(k)
        d.mkdir()
        r = subprocess.run(cmd + ["--decode", "--sha1", "--at", "5,35,65,95", str(d), src], capture_output=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
        texts.append(open(str(d / (os.path.basename(src) + ".sha1"))).read())
        lines = texts[-1].split("\n")
        assert lines[-1] == "" and lines[-2] == "stream " + hashlib.sha1(data).hexdigest() and len(lines) == 6
        for line, idx, p, dig in zip(lines, [5, 35, 65, 95], pics, psha):
            assert line.split() == [str(idx), str(p[0]), str(p[1]), str(p[2]), str(p[3]), dig.hex()]
        d = tmp_path / ("yuv%d" % k)
        d.mkdir()
        r = subprocess.run(cmd + ["--decode", "--at", "0::25", str(d), src], capture_output=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
        assert open(str(d / (os.path.basename(src) + ".yuv")), "rb").read() == _cut_from(full, [0, 25, 50, 75])[1]
    assert texts[0] == texts[1]
