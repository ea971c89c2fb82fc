"""slice_parse_cabac_kernel against the CPU form of the same code (csrc/lh264_slice_cabac.h): byte for byte the records, coefficient
planes, slice tables and results, with the guard bytes behind every buffer intact; and lh264_decode_batch with CABAC slice data parsed on
the device against the host route.  tests/test_slice_parse_cabac.py holds the CPU form against the host parser; a damaged input goes to
the device only after the CPU form has been through it."""
import hashlib

import pytest

import losslessh264_amd as lh
import slice_parse_cabac_cases as KC
import slice_parse_cases as K
from losslessh264_amd import slice_parse as SP
from test_slice_parse import cpu_form_against_host
from test_slice_parse_gpu import _decode, _same, _table, same_dump

pytestmark = pytest.mark.gpu

SET = ([(n, 0) for n, _ in K.committed() if n.startswith("cabac_edge/")] + [("slice_parse_cabac/cabac_i8.264", 0), ("slice_parse_cabac/cabac_wide.264", 0)] +
       [("streams/test_qcif_cabac.264", 0), ("streams/QCIF_2P_I_allIPCM.264", 0), ("streams/tibbycabac.264", 14), ("streams/test_cif_P_CABAC_slice.264", 60),
        ("streams/test_cif_I_CABAC_slice.264", 30)])


@pytest.mark.parametrize("name,nals", SET, ids=[n for n, _ in SET])
def test_kernel_equals_cpu_form(name, nals):
    data = K.read(name)
    if nals:
        data = K.head(data, nals)
    cpu, g0, e0 = SP.slice_parse(data, threads=4, cabac=True)
    assert g0 and sum(p.n_deferred for p in cpu) > 0
    assert all((p.results[:, 1] == 0).all() for p in cpu)
    assert any(SP.parse_file_plain(data, deferred=True, cabac=True).deferred_cabac)
    dev, g1, e1 = SP.slice_parse(data, on_device=True, cabac=True)
    assert g1, "guard bytes were overwritten on the device"
    assert e0 == e1
    same_dump(cpu, dev)


def test_kernel_on_damaged_streams():
    """the 20 damaged streams and the overrun / inconsistent-task tweaks: each through the host parser and the CPU form first (statuses as
    test_slice_parse_cabac.py asks), then through the kernel: the same statuses, the same bytes, no guard touched"""
    statuses = set()
    for label, data in KC.damaged_cases():
        b = SP.parse_file_plain(data, deferred=True, cabac=True)
        cpu, g0, _ = SP.slice_parse(data, threads=4, cabac=True)
        cpu_form_against_host(b, cpu, g0)
        dev, g1, _ = SP.slice_parse(data, on_device=True, cabac=True)
        assert g1, label
        same_dump(cpu, dev)
        for p in dev:
            statuses |= set(int(s) for s in p.results[:, 1])
    assert 1 in statuses and 0 in statuses
    data = KC.overrun_input()
    first1 = int(SP.slice_parse(data, cabac=True)[0][0].slices[1]["first_mb"])
    for tweak, want in (((0, 0, first1 - 1), 2), ((0, 0, first1 - 7), 2), ((0, 0, 1), 2), ((0, 0, 0), 3), ((0, 0, first1, 0x83), 3), ((0, 0, first1, 0), 3)):
        cpu, g0, _ = SP.slice_parse(data, tweak=tweak, cabac=True)
        assert g0 and int(cpu[0].results[0][1]) == want
        dev, g1, _ = SP.slice_parse(data, on_device=True, tweak=tweak, cabac=True)
        assert g1
        same_dump(cpu, dev)


# ---- decode_batch (parse="device+cabac") against parse="host" -----------------------------------------------------------------------
def _decode_c(datas, **kw):
    """-> per stream (status, error, pictures, bytes, stream digest, route, device slices, of them CABAC)"""
    b = lh.decode_batch(datas, sha1="stream", parse="device+cabac", **kw)
    out = [(b.status(i), b.error(i), b.pictures(i), b.data(i), b.stream_sha1(i), b.parse_path(i), b.device_slices(i), b.device_cabac_slices(i)) for i in range(len(datas))]
    b.free()
    return out


def _counts(data):
    """-> (deferred slices of both kinds, the CABAC ones) of a stream that parses"""
    r = SP.parse_file_plain(data, deferred=True, cabac=True)
    return sum(len(d) for d in r.deferred), sum(sum(m) for m in r.deferred_cabac)


def test_the_reference_table():
    names, sha, datas, host, _ = _table()
    assert len(names) == 36
    dev = _decode_c(datas)
    _same(host, dev)
    n_cabac = 0
    for n, data, d in zip(names, datas, dev):
        if d[0] == 0:
            assert d[4].hex() == sha[n], n
        r = KC.deferred_both("streams/" + n)                    # the whole stream: its first slice may come late
        if d[0] == 0 and KC.has_cabac(r):
            assert d[5] == "device" and d[7] > 0, n
            n_cabac += 1
        if d[5] == "host":
            assert not any(r.deferred), n
    # the CABAC streams of the corpus that the table lists and that decode: all of them went through slice_parse_cabac_kernel
    corpus = ("test_qcif_cabac.264", "tibbycabac.264", "test_cif_I_CABAC_slice.264", "test_cif_P_CABAC_slice.264", "QCIF_2P_I_allIPCM.264")
    assert n_cabac == sum(1 for n, d in zip(names, dev) if n in corpus and d[0] == 0) > 0


STREAMS_C = ("cabac_edge/cabac_mixed.264", "cabac_edge/cabac_skip.264")


def test_streams_stay_on_the_device_through_cabac_pictures():
    joined = K.read("edge/qp_edges.264") + K.read("cabac_edge/cabac_skip.264") + K.read("edge/qp_edges.264")
    datas = [K.read(n) for n in STREAMS_C] + [joined]
    counts = [_counts(d) for d in datas]
    assert all(c[1] > 0 for c in counts) and counts[2][0] > counts[2][1]
    for r in (1, 8):
        host = _decode(datas, round_pictures=r)
        dev = _decode_c(datas, round_pictures=r)
        _same(host, dev)
        assert all(d[0] == 0 and d[5] == "device" for d in dev)
        assert [(d[6], d[7]) for d in dev] == counts
        # without the flag: what tests/test_slice_parse_gpu.py::test_call_c_leaves_the_device_at_a_cabac_picture asserts
        old = _decode(datas, parse="device", round_pictures=r)
        _same(host, old)
        assert [d[5] for d in old] == ["host", "host", "device"] and [d[6] for d in old] == [0, 0, 2]


def test_a_change_of_resolution_ends_the_round_on_the_cavlc_device_route():
    """CAVLC pictures of 4 x 4, 3 x 3 and 4 x 4 macroblocks in one stream, parse="device" without the flag: a round ends in front of a
    picture of another size before that picture is examined - on the device route its slice data is not parsed yet when the round's
    pictures are chosen, and the picture was refused as not covered.  With round_pictures 8 a round would hold pictures of both sizes"""
    parts = [K.read("edge/qp_edges.264"), K.read("slice_parse/i8_first.264"), K.read("edge/qp_edges.264")]
    sizes = [{(f.mb_w, f.mb_h) for f in SP.parse_file_plain(d).frames} for d in parts]
    assert sizes == [{(4, 4)}, {(3, 3)}, {(4, 4)}]
    datas = [b"".join(parts)]
    slices = sum(len(d) for d in SP.parse_file_plain(datas[0], deferred=True).deferred)
    for r in (1, 8):
        host = _decode(datas, round_pictures=r)
        for dev in (_decode(datas, parse="device", round_pictures=r), _decode_c(datas, round_pictures=r)):
            _same(host, dev)
            assert dev[0][0] == 0 and len(dev[0][2]) == 6 and dev[0][5] == "device" and dev[0][6] == slices


def test_i8_picture():
    """I8x8 macroblocks under CABAC in I and P slices, through the whole decode call"""
    datas = [K.read("slice_parse_cabac/cabac_i8.264")]
    for r in (1, 8):
        dev = _decode_c(datas, round_pictures=r)
        _same(_decode(datas, round_pictures=r), dev)
        assert dev[0][0] == 0 and len(dev[0][2]) == 3 and dev[0][5] == "device" and (dev[0][6], dev[0][7]) == _counts(datas[0]) == (4, 4)


def test_wide_picture():
    """257 macroblocks wide: the line of neighbour state lies in device memory, not in LDS"""
    datas = [K.read("slice_parse_cabac/cabac_wide.264")]
    for r in (1, 8):
        dev = _decode_c(datas, round_pictures=r)
        _same(_decode(datas, round_pictures=r), dev)
        assert dev[0][0] == 0 and len(dev[0][2]) == 3 and dev[0][5] == "device" and (dev[0][6], dev[0][7]) == _counts(datas[0]) == (5, 5)


def test_forced_fallback(monkeypatch):
    data = K.read("streams/test_qcif_cabac.264")
    host = _decode([data, data])
    monkeypatch.setenv("LH264_SLICE_PARSE_FAIL_CABAC", "3")
    dev = _decode_c([data, data])
    monkeypatch.delenv("LH264_SLICE_PARSE_FAIL_CABAC")
    _same(host, dev)
    assert sorted(d[5] for d in dev) == ["device", "fallback"]


def test_damaged_streams_conceal_and_output_modes():
    cases = KC.damaged_cases()
    fails = [d for _, d in cases if SP.parse_file_plain(d, deferred=True, cabac=True).error][:3]
    cuts = [d for l, d in cases if l.startswith("cut")][:2]
    datas = fails + cuts + [KC.multi_slice()]
    for d in datas:                                          # the CPU form first
        cpu, g0, _ = SP.slice_parse(d, threads=4, cabac=True)
        assert g0
    host = _decode(datas)
    dev = _decode_c(datas)
    _same(host, dev)
    assert any(h[0] != 0 for h in host) and all(d[5] in ("device", "fallback") for d in dev) and any(d[5] == "fallback" for d in dev)
    conc = _decode_c(datas, conceal="mv_copy")
    _same(_decode(datas, conceal="mv_copy"), conc)
    assert all(d[5] == "host" and d[6] == 0 for d in conc)
    b = lh.decode_batch(datas, parse="device+cabac", device_out=True, sha1="both")
    for i, h in enumerate(host):
        assert bytes(b.tensor(i).cpu().numpy().tobytes()) == h[3] and b.stream_sha1(i) == h[4]
    b.free()
    b = lh.decode_batch(datas, parse="device+cabac", sha1="both", pictures=False)
    for i, h in enumerate(host):
        assert b.stream_sha1(i) == h[4] and b.pictures(i) == h[2] and b.data(i) == b""
        assert b.picture_sha1(i) == [hashlib.sha1(h[3][p[4]:p[4] + p[5]]).digest() for p in h[2]]
    b.free()
