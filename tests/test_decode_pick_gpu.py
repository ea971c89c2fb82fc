"""Picking the pictures a decode call decodes (decode_batch (pick="intra" | "idr")) on the device.  The yardstick is exact: a picture
whose slices are all I slices depends on no other picture, so decoded alone it is byte for byte that picture of the full decode.  One
pick="all" call, one "intra" and one "idr" over the small committed streams are computed once per module; every other call is held
to them.  What the device sees that is new - a chain per picture, task lists of the selected pictures only - is held by the bytes, by
parsed_slices (skipped, not decoded and dropped) and by lh264_decode_last_chains."""
import collections
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import pytest

import scale_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK = 0
STREAMS = ["streams/MIDR_MW_D.264", "streams/MR1_BT_A.h264", "streams/CVFC1_Sony_C.jsv", "streams/BA1_Sony_D.jsv", "streams/syn720p_allI_4slices_8f.264",
           "streams/BA_MW_D_IDR_LOST.264", "streams/Error_I_P.264", "streams/test_qcif_cabac.264", "streams/QCIF_2P_I_allIPCM.264",
           "cabac_edge/cabac_qp.264", "cabac_edge/cabac_mixed.264", "cabac_edge/cabac_pcm.264", "cabac_edge/cabac_skip.264",
           "streams/BA_MW_D.264", "streams/BA_MW_D.264+streams/Error_I_P.264"]
# the full call stops these at the picture named (macroblocks no slice covers in Error_I_P's first picture); both pictures are IDR
# pictures, so a picked call selects them and stops there too
STOPPED = {"streams/Error_I_P.264": 0, "streams/BA_MW_D.264+streams/Error_I_P.264": 100}
PICKS = ("intra", "idr")

R = collections.namedtuple("R", "status error pics data src index parsed psha ssha path dslices")
_cache = {}


def _read(name):
    return b"".join(open(os.path.join(GOLDEN, part), "rb").read() for part in name.split("+"))


def _datas():
    if "datas" not in _cache:
        _cache["datas"] = [_read(n) for n in STREAMS]
    return _cache["datas"]


def _result(b, n, data=None, sha=True):
    out = []
    for i in range(n):
        out.append(R(b.status(i), b.error(i), b.pictures(i), data[i] if data is not None else b.data(i), b.source_sizes(i), b.picture_indices(i),
                     b.parsed_slices(i), b.picture_sha1(i) if sha else None, b.stream_sha1(i) if sha else None, b.parse_path(i), b.device_slices(i)))
    b.free()
    return out


def _call(pick, fmt="i420"):
    """ONE host-mode decode_batch over STREAMS per (pick, format), with both digests, shared by the tests"""
    if (pick, fmt) not in _cache:
        import losslessh264_amd as lh
        _cache[(pick, fmt)] = _result(lh.decode_batch(_datas(), fmt=fmt, pick=pick, sha1="both"), len(STREAMS))
    return _cache[(pick, fmt)]


def _slice_counts(i):
    """slices per picture of stream i, from the full parse on the host"""
    if ("slices", i) not in _cache:
        import losslessh264_amd as lh
        _cache[("slices", i)] = [len(f.slices) for f in lh.parse_file(_datas()[i])[0]]
    return _cache[("slices", i)]


def _selected(i, pick):
    """the indices the header walk selects (lh264_parser_pick: held to the full parse by tests/test_decode_pick.py)"""
    if ("sel", i, pick) not in _cache:
        import losslessh264_amd as lh
        _cache[("sel", i, pick)] = lh.pick(_datas()[i], pick)
    return _cache[("sel", i, pick)]


def _cut_from(full, index):
    """the pictures `index` (positions in the full call's result, which delivers every picture up to where it stops) of a full call's
    result -> (picture records with offsets of their own, bytes, source sizes, picture digests)"""
    pics, data, off = [], [], 0
    for k in index:
        w, h, fn, idr, o, n = full.pics[k]
        pics.append((w, h, fn, idr, off, n))
        data.append(full.data[o:o + n])
        off += n
    return pics, b"".join(data), [full.src[k] for k in index], [full.psha[k] for k in index]


def _check_against_full(got, full, i, pick, what, digests=True, data=True):
    """stream i of a picked call against the full call: the selected pictures in front of where the full call stops, and its end"""
    name = STREAMS[i]
    assert full.index == list(range(len(full.pics))), name
    want_idx = [k for k in _selected(i, pick) if k < len(full.pics)]
    assert got.index == want_idx, (what, name, got.index)
    pics, bytes_, src, psha = _cut_from(full, want_idx)
    assert got.pics == pics and got.src == src, (what, name)
    if data:
        assert got.data == bytes_, (what, name)
    if digests:
        assert got.psha == psha, (what, name)
        assert got.ssha == hashlib.sha1(bytes_).digest(), (what, name)
    assert (got.status, got.error) == (full.status, full.error), (what, name, got.error)


# ---- 1: parity ------------------------------------------------------------------------------------------------------------------------------
def test_the_full_call_is_what_the_table_says():
    """not vacuous: every stream is LH264_OK in the full call except the two that Error_I_P's bytes stop, the index of a full call counts
    the pictures, and each picked call has something to select on every stream"""
    full = _call("all")
    for i, name in enumerate(STREAMS):
        f = full[i]
        assert (f.status == OK) == (name not in STOPPED), (name, f.error)
        if name in STOPPED:
            assert f.error.startswith("picture %d: " % STOPPED[name]) and len(f.pics) == STOPPED[name], (name, f.error)
        assert f.index == list(range(len(f.pics))) and len(f.data) == sum(p[5] for p in f.pics)
        assert f.ssha == hashlib.sha1(f.data).digest()
        if name not in STOPPED:
            assert f.parsed == sum(_slice_counts(i)) and f.path == "host" and f.dslices == 0, name
        for pick in PICKS:
            assert len(_selected(i, pick)) >= 1, (name, pick)


@pytest.mark.parametrize("pick", PICKS)
def test_picked_pictures_are_the_full_call_s(pick):
    """host mode, I420: for every stream the picked call's pictures are the slices of the full call's bytes at picture_indices - bytes,
    (width, height, frame_num, idr), source sizes, per-picture SHA-1 - and the stream SHA-1 is hashlib's of the delivered bytes"""
    full, got = _call("all"), _call(pick)
    for i, name in enumerate(STREAMS):
        _check_against_full(got[i], full[i], i, pick, pick)
        assert got[i].ssha == hashlib.sha1(got[i].data).digest(), name
    by = dict(zip(STREAMS, got))
    e = by["streams/Error_I_P.264"]
    assert e.index == [] and e.data == b"" and e.status != OK and e.error.startswith("picture 0: ")
    e = by["streams/BA_MW_D.264+streams/Error_I_P.264"]
    assert e.index == [0, 30, 60, 90] and e.status != OK and e.error.startswith("picture 100: ")
    e = by["streams/BA_MW_D_IDR_LOST.264"]
    assert e.index == [27, 57, 87] and e.status == OK
    assert by["streams/MIDR_MW_D.264"].index == ([0, 30, 60, 90] if pick == "intra" else [0, 60])
    assert by["cabac_edge/cabac_mixed.264"].index == [0]


# ---- 2: skipped, not dropped ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parse", ["host", "device+cabac"])
def test_unselected_pictures_are_not_parsed(parse):
    """parsed_slices is the sum of the slice counts of the selected pictures (from parse_file), on both parse routes; on the device
    route device_slices is at most parsed_slices and equals it for a stream that stayed on that route (no round waits in this batch)"""
    import losslessh264_amd as lh
    n = len(STREAMS)
    res = {"all": _call("all")} if parse == "host" else {"all": _result(lh.decode_batch(_datas(), parse=parse, sha1="both"), n)}
    for pick in PICKS:
        res[pick] = _call(pick) if parse == "host" else _result(lh.decode_batch(_datas(), parse=parse, pick=pick, sha1="both"), n)
    for i, name in enumerate(STREAMS):
        counts = _slice_counts(i)
        for pick in ("all",) + PICKS:
            r = res[pick][i]
            sel = list(range(len(counts))) if pick == "all" else _selected(i, pick)
            if name in STOPPED:
                # (how many pictures behind the stop were parsed with the round that held it follows round_pictures, not the stream)
                assert sum(counts[k] for k in sel if k <= STOPPED[name]) <= r.parsed <= sum(counts[k] for k in sel), (parse, pick, name, r.parsed)
                continue
            assert r.parsed == sum(counts[k] for k in sel), (parse, pick, name, r.parsed)
            assert r.dslices <= r.parsed, (parse, pick, name)
            if parse != "host" and r.path == "device":
                assert r.dslices == r.parsed, (parse, pick, name)
            if parse != "host":
                assert r.data == _call(pick)[i].data and r.index == _call(pick)[i].index, (parse, pick, name)
    by = {pick: dict(zip(STREAMS, res[pick])) for pick in res}
    assert [by[p]["streams/MIDR_MW_D.264"].parsed for p in ("all", "intra", "idr")] == [100, 4, 2]
    i = STREAMS.index("streams/MR1_BT_A.h264")
    assert sum(_slice_counts(i)) == 171 and by["intra"]["streams/MR1_BT_A.h264"].parsed == sum(_slice_counts(i)[k] for k in (0, 10, 31, 41, 51)) < 171
    if parse != "host":
        assert by["intra"]["streams/MIDR_MW_D.264"].path == "device" and by["intra"]["streams/test_qcif_cabac.264"].path == "device"
        assert by["intra"]["streams/MIDR_MW_D.264"].dslices == 4


# ---- 3: damage in an unselected picture ----------------------------------------------------------------------------------------------------
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


def test_damage_in_an_unselected_picture_is_not_seen():
    """the slice of picture 10 cut short: the full call stops at picture 10, the picked call is LH264_OK and delivers 0, 30, 60, 90 of the
    undamaged stream.  The same cut in picture 30 stops the picked call at picture 30 with the full call's text, picture 0 delivered"""
    import losslessh264_amd as lh
    i = STREAMS.index("streams/BA_MW_D.264")
    clean, want = _datas()[i], _call("intra")[i]
    assert want.index == [0, 30, 60, 90] and want.status == OK
    cut10, cut30 = _cut_slice(clean, 10), _cut_slice(clean, 30)
    full10, full30 = _result(lh.decode_batch([cut10, cut30], sha1="both"), 2)
    assert full10.status != OK and full10.error.startswith("picture 10: ") and len(full10.pics) == 10
    assert full30.status != OK and full30.error.startswith("picture 30: ") and len(full30.pics) == 30
    for kw in (dict(), dict(parse="device")):
        got10, got30 = _result(lh.decode_batch([cut10, cut30], pick="intra", sha1="both", **kw), 2)
        assert got10.status == OK and got10.error == "" and got10.index == [0, 30, 60, 90], kw
        assert (got10.pics, got10.data, got10.psha, got10.ssha) == (want.pics, want.data, want.psha, want.ssha), kw
        assert got10.parsed == 4
        assert (got30.status, got30.error) == (full30.status, full30.error) and got30.index == [0], kw
        assert got30.data == want.data[:want.pics[0][5]] and got30.pics == want.pics[:1], kw


# ---- 4: routes and modes -------------------------------------------------------------------------------------------------------------------
def _same(res, pick, what, data=True, digests=True):
    want = _call(pick)
    for i, name in enumerate(STREAMS):
        g, w = res[i], want[i]
        assert (g.status, g.error, g.pics, g.src, g.index) == (w.status, w.error, w.pics, w.src, w.index), (what, name, g.error)
        if data:
            assert g.data == w.data, (what, name)
        if digests:
            assert (g.psha, g.ssha) == (w.psha, w.ssha), (what, name)


@pytest.mark.parametrize("pick", PICKS)
@pytest.mark.parametrize("kw", [dict(parse="device"), dict(round_pictures=1), dict(round_pictures=8), dict(group_mbs=600, threads=4),
                                dict(group_mbs=600, parse="device+cabac"), dict(threads=1), dict(round_pictures=3, group_mbs=5000, parse="device")],
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in sorted(kw.items())))
def test_the_cuts_of_the_work_and_the_routes_do_not_show(pick, kw):
    """the parse routes, round_pictures 1 and 8, a group_mbs that makes streams wait (600 macroblocks: less than two QCIF streams'
    rounds), one thread: the picked result of the host-mode call, digests included; parse_path as the rules give it"""
    import losslessh264_amd as lh
    res = _result(lh.decode_batch(_datas(), pick=pick, sha1="both", **kw), len(STREAMS))
    _same(res, pick, kw)
    for i, name in enumerate(STREAMS):
        r = res[i]
        if "parse" not in kw:
            assert r.path == "host" and r.dslices == 0, name
            continue
        cabac_first = name.startswith("cabac_edge/") or name == "streams/test_qcif_cabac.264"
        if kw["parse"] == "device" and cabac_first:
            assert r.path == "host" and r.dslices == 0, name      # a CABAC picture is the host's without the flag
        elif cabac_first or name in ("streams/MIDR_MW_D.264", "streams/BA_MW_D.264", "streams/BA_MW_D_IDR_LOST.264"):
            assert r.path == "device" and r.dslices >= r.parsed >= 1, name      # (CAVLC streams, and CABAC ones with the flag)
        if name not in STOPPED:
            assert r.parsed == _call(pick)[i].parsed, (kw, name)      # distinct slices: a picture that waited counts once


@pytest.mark.parametrize("pick", PICKS)
def test_nv12_and_reduced_sizes(pick):
    """NV12: the selected pictures of the NV12 full call.  scale 1 and 3: tests/scale_ref.py applied to the picked full-size bytes"""
    import losslessh264_amd as lh
    n = len(STREAMS)
    full, got = _call("all", "nv12"), _call(pick, "nv12")
    for i in range(n):
        _check_against_full(got[i], full[i], i, pick, "nv12")
    assert any(got[i].data != _call(pick)[i].data for i in range(n))
    for fmt, s in (("i420", 1), ("i420", 3), ("nv12", 3)):
        res = _result(lh.decode_batch(_datas(), fmt=fmt, pick=pick, scale=s, sha1="both"), n)
        for i, name in enumerate(STREAMS):
            base = _call(pick, fmt)[i]
            data, pics = scale_ref.scale_packed(base.data, base.pics, fmt, s)
            g = res[i]
            assert (g.status, g.error, g.index, g.src) == (base.status, base.error, base.index, base.src), (fmt, s, name)
            assert g.pics == pics and g.data == data, (fmt, s, name)
            assert g.ssha == hashlib.sha1(data).digest() and g.psha == [hashlib.sha1(data[p[4]:p[4] + p[5]]).digest() for p in pics], (fmt, s, name)


@pytest.mark.parametrize("pick", PICKS)
def test_output_modes(pick):
    """device_out, a sink (runs of consecutive delivered pictures, first_picture counts delivered pictures), pictures=False with both
    digests"""
    import losslessh264_amd as lh
    datas, n = _datas(), len(STREAMS)
    b = lh.decode_batch(datas, pick=pick, device_out=True, sha1="both")
    _same(_result(b, n, [b.tensor(i).cpu().numpy().tobytes() for i in range(n)]), pick, "device_out")
    seen, recs, calls = [[] for _ in range(n)], [[] for _ in range(n)], [0] * n

    def sink(stream, first, pics, data):
        assert first == len(recs[stream]) and len(pics) >= 1 and len(data) == sum(p[5] for p in pics)
        assert [p[4] for p in pics] == [sum(q[5] for q in recs[stream]) + sum(q[5] for q in pics[:k]) for k in range(len(pics))]
        seen[stream].append(data)
        recs[stream] += pics
        calls[stream] += 1
        return 0
    b = lh.decode_batch(datas, pick=pick, sink=sink, round_pictures=2, sha1="both")
    assert [b.data(i) for i in range(n)] == [b""] * n
    res = _result(b, n, [b"".join(x) for x in seen])
    _same(res, pick, "sink")
    assert [r.pics for r in res] == recs
    assert calls[STREAMS.index("streams/BA1_Sony_D.jsv")] == (9 if pick == "intra" else 1)      # 17 pictures two by two; one IDR picture
    res = _result(lh.decode_batch(datas, pick=pick, sha1="both", pictures=False), n)
    _same(res, pick, "pictures=False", data=False)
    assert all(r.data == b"" for r in res)


def test_the_64_byte_struct_is_the_call_of_before():
    """struct_bytes 64 with `pick` words behind it that say idr: every picture is decoded, as by the library before"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    lib = L.lib()
    datas = _datas()
    n = len(datas)
    ptrs, lens = (C.c_char_p * n)(*datas), (C.c_size_t * n)(*[len(d) for d in datas])
    o = L.DecodeOptsV5()
    o.struct_bytes, o.pick, o.reserved3 = 64, 2, 7
    o.flags = L.DECODE_SHA1_PICTURES | L.DECODE_SHA1_STREAM
    outs = (C.c_void_p * n)()
    assert lib.lh264_decode_batch(ptrs, lens, n, 0, C.byref(o), outs) == OK
    res = _result(lh.DecodedBatch(lib, [outs[i] for i in range(n)], False), n)
    want = _call("all")
    for i, name in enumerate(STREAMS):
        assert res[i] == want[i], name


# ---- 5: a change of resolution -------------------------------------------------------------------------------------------------------------
def test_idr_pictures_of_two_sizes():
    """cabac_skip.264 with pick="idr": pictures 0 and 3, the second one of the 1 x 1-macroblock pictures, alone in a call"""
    import losslessh264_amd as lh
    i = STREAMS.index("cabac_edge/cabac_skip.264")
    full = _call("all")[i]
    got = _result(lh.decode_batch([_datas()[i]], pick="idr", sha1="both"), 1)[0]
    assert got.index == [0, 3] and got.status == OK
    assert [(p[0], p[1]) for p in got.pics] == [full.pics[0][:2], (16, 16)] and full.pics[0][:2] != (16, 16)
    _check_against_full(got, full, i, "idr", "alone")


# ---- 6: the launch shape -------------------------------------------------------------------------------------------------------------------
def test_a_chain_per_selected_picture():
    """BA1_Sony_D.jsv alone, 17 intra pictures, round_pictures 8: three rounds; with pick="intra" every picture is a chain of its own
    (jobs == chains == 17), with pick="all" the stream is one chain per round.  The bytes are the same"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    i = STREAMS.index("streams/BA1_Sony_D.jsv")
    v = (C.c_longlong * 3)()
    shapes = {}
    for pick in ("intra", "all"):
        r = _result(lh.decode_batch([_datas()[i]], pick=pick, round_pictures=8, sha1="both"), 1)[0]
        assert L.lib().lh264_decode_last_chains(v) == OK
        shapes[pick] = tuple(v)
        assert r.index == list(range(17)) and r.data == _call("all")[i].data and r.ssha == _call("all")[i].ssha, pick
    assert shapes["intra"] == (3, 17, 17) and shapes["all"] == (3, 3, 17)
    r = _result(lh.decode_batch([_datas()[i]], pick="idr", round_pictures=8, sha1="both"), 1)[0]
    assert L.lib().lh264_decode_last_chains(v) == OK and tuple(v) == (1, 1, 1) and r.index == [0]


# ---- 7: the command lines ------------------------------------------------------------------------------------------------------------------
def test_the_command_lines_take_pick(tmp_path):
    """lh264dec --decode --sha1 --pick intra on two streams: the index column of the .sha1 files is picture_indices, the digests are
    those of the picked call; python -m losslessh264_amd writes the same files; --pick idr without --sha1 writes the picked bytes"""
    names = ["streams/MIDR_MW_D.264", "streams/MR1_BT_A.h264"]
    srcs = [os.path.join(GOLDEN, s) for s in names]
    want = [_call("intra")[STREAMS.index(s)] for s in names]
    texts = []
    for k, cmd in enumerate(([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"])):
        d = tmp_path / str(k)
        d.mkdir()
        r = subprocess.run(cmd + ["--decode", "--sha1", "--pick", "intra", str(d)] + srcs, capture_output=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
        texts.append([open(str(d / (os.path.basename(s) + ".sha1"))).read() for s in srcs])
        for text, w in zip(texts[-1], want):
            lines = text.split("\n")
            assert lines[-1] == "" and lines[-2] == "stream " + w.ssha.hex() and len(lines) == len(w.pics) + 2
            for line, idx, p, dig in zip(lines, w.index, w.pics, w.psha):
                assert line.split() == [str(idx), str(p[0]), str(p[1]), str(p[2]), str(p[3]), dig.hex()]
    assert texts[0] == texts[1]
    assert [int(x.split()[0]) for x in texts[0][0].split("\n")[:-2]] == [0, 30, 60, 90]
    d = tmp_path / "yuv"
    d.mkdir()
    r = subprocess.run([os.path.join(ROOT, "losslessh264_amd", "lh264dec"), "--decode", "--device-parse", "--scale", "0", "--pick", "idr", str(d), srcs[0]],
                       capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
    assert open(str(d / (os.path.basename(srcs[0]) + ".yuv")), "rb").read() == _call("idr")[STREAMS.index(names[0])].data
