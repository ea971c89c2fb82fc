"""slice_parse_kernel against the CPU form of the same code (csrc/lh264_slice.h): byte for byte the records, coefficient planes,
slice tables and results, with the guard bytes behind every buffer intact.  tests/test_slice_parse.py holds the CPU form against the
host parser; a damaged input goes to the device only after the CPU form has been through it."""
import pytest

import slice_parse_cases as K
from losslessh264_amd import slice_parse as SP
from test_slice_parse import cpu_form_against_host

pytestmark = pytest.mark.gpu

# the edge streams, the synthetic ones, and corpus streams that between them reach every branch test_slice_parse.py counts: slices
# that start mid-row, every partition shape, up to 7 references, I_PCM, the 8x8 transform (the stream's first pictures) and scaling lists
SET = ([n for n, _ in K.committed() if n.startswith(("edge/", "slice_parse/"))] +
       ["streams/SVA_Base_B.264", "streams/MR1_BT_A.h264", "streams/CVPCMNL1_SVA_C.264", "streams/CVFC1_Sony_C.jsv", "streams/test_scalinglist_jm.264",
        "streams/tibby8x8cavlc.264"])


def same_dump(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x.mb_w, x.mb_h, x.n_deferred) == (y.mb_w, y.mb_h, y.n_deferred)
        assert (x.results == y.results).all(), "picture %d: results differ" % i
        for k in ("mbs", "coeffs", "slices"):
            assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), "picture %d: %s differs" % (i, k)


@pytest.mark.parametrize("name", SET)
def test_kernel_equals_cpu_form(name):
    data = K.read(name)
    if name == "streams/tibby8x8cavlc.264":
        data = K.head(data, 14)
    cpu, g0, e0 = SP.slice_parse(data, threads=4)
    assert g0 and sum(p.n_deferred for p in cpu) > 0
    assert all((p.results[:, 1] == 0).all() for p in cpu)
    dev, g1, e1 = SP.slice_parse(data, on_device=True)
    assert g1, "guard bytes were overwritten on the device"
    assert e0 == e1
    same_dump(cpu, dev)


def test_kernel_on_damaged_streams():
    """the 20 damaged streams, Error_I_P.264 and the overrun: each through the host parser and the CPU form first (statuses as
    test_slice_parse.py asks), then through the kernel: the same statuses, the same bytes, no guard touched"""
    cases = K.damaged_cases() + [("Error_I_P", K.read("streams/Error_I_P.264"))]
    statuses = set()
    for label, data in cases:
        b = SP.parse_file_plain(data, deferred=True)
        cpu, g0, _ = SP.slice_parse(data, threads=4)
        cpu_form_against_host(b, cpu, g0)
        dev, g1, _ = SP.slice_parse(data, on_device=True)
        assert g1, label
        same_dump(cpu, dev)
        for p in dev:
            statuses |= set(int(s) for s in p.results[:, 1])
    assert 1 in statuses and 0 in statuses
    data = K.head(K.read("streams/SVA_Base_B.264"), 6)
    for limit in (32, 1, 0):
        cpu, g0, _ = SP.slice_parse(data, tweak=(0, 0, limit))
        assert g0 and int(cpu[0].results[0][1]) == (2 if limit else 3)
        dev, g1, _ = SP.slice_parse(data, on_device=True, tweak=(0, 0, limit))
        assert g1
        same_dump(cpu, dev)


# ---- 7: decode_batch (parse="device") against parse="host" -----------------------------------------------------------------------
import hashlib
import json
import os

import losslessh264_amd as lh


def _decode(datas, **kw):
    """-> per stream (status, error, pictures, bytes, stream digest, route)"""
    b = lh.decode_batch(datas, sha1="stream", **kw)
    out = [(b.status(i), b.error(i), b.pictures(i), b.data(i), b.stream_sha1(i), b.parse_path(i), b.device_slices(i)) for i in range(len(datas))]
    b.free()
    return out


def _same(host, dev):
    assert len(host) == len(dev)
    for i, (h, d) in enumerate(zip(host, dev)):
        assert h[:5] == d[:5], "stream %d: parse=device differs from parse=host (status %s / %s, %r / %r)" % (i, h[0], d[0], h[1], d[1])
        assert h[5] == "host" and h[6] == 0


_memo = {}


def _table():
    if "t" not in _memo:
        t = json.load(open(os.path.join(K.ROOT, "tests", "golden", "decoder_sha1.json")))
        t = {k: v for k, v in t.items() if not k.startswith("_")}
        names = sorted(n for n in os.listdir(os.path.join(K.GOLDEN, "streams")) if n in t)
        datas = [K.read("streams/" + n) for n in names]
        _memo["t"] = (names, t, datas, _decode(datas), _decode(datas, parse="device"))
    return _memo["t"]


def test_call_a_the_reference_table():
    names, sha, datas, host, dev = _table()
    assert len(names) == 36
    _same(host, dev)
    routes = {}
    for n, data, d in zip(names, datas, dev):
        if d[0] == 0:
            assert d[4].hex() == sha[n], n
        cavlc = any(SP.parse_file_plain(K.head(data, 12), deferred=True).deferred)
        routes[n] = d[5]
        if cavlc and d[0] == 0:
            assert d[5] == "device", n
        if not cavlc:
            assert d[5] == "host", n
    assert sum(1 for r in routes.values() if r == "device") >= 25


def test_call_b_edge_and_synthetic_streams():
    datas = [K.read(n) for n, _ in K.committed() if n.startswith(("edge/", "slice_parse/"))]
    dev = _decode(datas, parse="device")
    _same(_decode(datas), dev)
    assert all(d[5] == "device" for d in dev)
    for data, d in zip(datas, dev):
        if d[0] == 0:
            assert d[6] == sum(len(x) for x in SP.parse_file_plain(data, deferred=True).deferred)


def test_call_c_leaves_the_device_at_a_cabac_picture():
    """a stream is on the device route until its first picture of CABAC slices and with the host parser from there on, CAVLC pictures
    behind it included: a CAVLC stream with a CABAC stream behind it reports DEVICE, a stream that begins with CABAC reports HOST"""
    joined = K.read("edge/qp_edges.264") + K.read("cabac_edge/cabac_skip.264") + K.read("edge/qp_edges.264")
    datas = [K.read("cabac_edge/cabac_mixed.264"), K.read("cabac_edge/cabac_skip.264"), joined]
    first_is_cavlc = [bool(SP.parse_file_plain(d, deferred=True).deferred[0]) for d in datas]
    assert first_is_cavlc[1:] == [False, True]
    for r in (1, 8):
        dev = _decode(datas, parse="device", round_pictures=r)
        _same(_decode(datas, round_pictures=r), dev)
        assert [d[5] for d in dev] == ["device" if c else "host" for c in first_is_cavlc]
        assert len(dev[0][2]) == 6 and len(dev[2][2]) == 2 + 5 + 2 and all(d[0] == 0 for d in dev)
        # the kernel parsed the CAVLC slices in front of the first CABAC picture and none behind it: the host parsed those
        in_front = sum(len(d) for d in SP.parse_file_plain(K.read("edge/qp_edges.264"), deferred=True).deferred)
        assert in_front == 2 and [d[6] for d in dev] == [0, 0, in_front]


def test_call_d_damaged_streams_stop_where_the_host_stops():
    cases = dict(K.damaged_cases())
    cuts = [d for l, d in K.damaged_cases() if l.startswith("cut")][:2]
    fails = [d for l, d in K.damaged_cases() if SP.parse_file_plain(d, deferred=True).error][:2]
    datas = [K.read("streams/Error_I_P.264"), K.read("streams/BA_MW_D_IDR_LOST.264")] + cuts + fails
    host, dev = _decode(datas), _decode(datas, parse="device")
    _same(host, dev)
    assert any(h[0] != 0 for h in host)
    assert all(d[5] in ("device", "fallback") for d in dev) and any(d[5] == "fallback" for d in dev)
    assert cases


def test_call_e_conceal_keeps_the_host_route():
    datas = [K.read("streams/BA_MW_D_P_LOST.264"), K.read("streams/Error_I_P.264")]
    dev = _decode(datas, parse="device", conceal="mv_copy")
    host = _decode(datas, conceal="mv_copy")
    _same(host, dev)
    assert all(d[5] == "host" for d in dev)


def test_call_f_cuts_of_the_work_and_output_modes():
    names = ["streams/SVA_Base_B.264", "streams/MR1_BT_A.h264", "streams/CVFC1_Sony_C.jsv", "streams/SVA_BA2_D.264", "edge/levels_ext.264"]
    datas = [K.read(n) for n in names]
    host = _decode(datas)
    for kw in (dict(round_pictures=1), dict(round_pictures=8, threads=1), dict(group_mbs=600, threads=4), dict(round_pictures=3, group_mbs=5000)):
        dev = _decode(datas, parse="device", **kw)
        _same(host, dev)
        assert all(d[5] == "device" for d in dev), kw
    b = lh.decode_batch(datas, parse="device", device_out=True, sha1="both")
    for i, h in enumerate(host):
        assert bytes(b.tensor(i).cpu().numpy().tobytes()) == h[3] and b.stream_sha1(i) == h[4]
    b.free()
    b = lh.decode_batch(datas, parse="device", sha1="both", pictures=False)
    for i, h in enumerate(host):
        assert b.stream_sha1(i) == h[4] and b.pictures(i) == h[2] and b.data(i) == b""
        assert b.picture_sha1(i) == [hashlib.sha1(h[3][p[4]:p[4] + p[5]]).digest() for p in h[2]]
    b.free()


def test_call_g_forced_fallback(monkeypatch):
    data = K.read("streams/BA_MW_D.264")
    host = _decode([data, data])
    monkeypatch.setenv("LH264_SLICE_PARSE_FAIL", "3")
    dev = _decode([data, data], parse="device")
    monkeypatch.delenv("LH264_SLICE_PARSE_FAIL")
    _same(host, dev)
    assert sorted(d[5] for d in dev) == ["device", "fallback"]
