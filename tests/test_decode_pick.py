"""Picking the pictures a decode call decodes (lh264_decode_batch, opts->pick) where no device is present: the layout of the 72-byte
options struct, the arguments of the call, and lh264_parser_pick - the header walk's choice - on every committed stream of the table
in the issue, against a choice the test makes itself from the records of the full parse (parse_file)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# stream -> (pictures, all-I pictures, IDR pictures, pictures that mix I and P slices)
TABLE = {
    "streams/MIDR_MW_D.264": (100, 4, 2, 0),
    "streams/MR1_BT_A.h264": (62, 5, 1, 0),
    "streams/CVFC1_Sony_C.jsv": (50, 4, 1, 0),
    "streams/BA1_Sony_D.jsv": (17, 17, 1, 0),
    "streams/syn720p_allI_4slices_8f.264": (8, 8, 8, 0),
    "streams/BA_MW_D_IDR_LOST.264": (97, 3, 3, 0),
    "streams/Error_I_P.264": (6, 3, 3, 0),
    "streams/test_qcif_cabac.264": (30, 1, 1, 0),
    "streams/QCIF_2P_I_allIPCM.264": (2, 1, 1, 0),
    "cabac_edge/cabac_qp.264": (4, 2, 1, 0),
    "cabac_edge/cabac_mixed.264": (6, 1, 1, 2),
    "cabac_edge/cabac_pcm.264": (3, 1, 1, 1),
    "cabac_edge/cabac_skip.264": (5, 2, 2, 0),
}
# ... and the index lists the issue spells out
INTRA_AT = {
    "streams/MIDR_MW_D.264": [0, 30, 60, 90],
    "streams/MR1_BT_A.h264": [0, 10, 31, 41, 51],
    "streams/BA_MW_D_IDR_LOST.264": [27, 57, 87],
    "streams/Error_I_P.264": [0, 2, 4],
    "cabac_edge/cabac_qp.264": [0, 2],
}
IDR_AT = {"cabac_edge/cabac_skip.264": [0, 3], "streams/BA_MW_D_IDR_LOST.264": [27, 57, 87]}


def _lib():
    import __graft_entry__ as g
    g.build()
    from losslessh264_amd import _lib as L
    return L, L.lib()


def _read(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def test_layout_of_the_options_struct():
    """sizeof 72, pick at 64, reserved3 at 68, the 64-byte struct named V4; the header carries the two fields in that order behind
    reserved2, the values of pick and the new entry points"""
    L, lib = _lib()
    assert C.sizeof(L.DecodeOptsV5) == 72 and L.DecodeOptsV5.pick.offset == 64 and L.DecodeOptsV5.reserved3.offset == 68
    assert L.DECODE_OPTS_BYTES_V4 == 64 and C.sizeof(L.DecodeOptsV4) == 64
    assert L.PICK == {"all": 0, "intra": 1, "idr": 2}
    txt = open(os.path.join(ROOT, "include", "lh264.h")).read()
    assert re.search(r"uint32_t scale_log2;[^}]*uint32_t reserved2;[^}]*uint32_t pick;[^}]*uint32_t reserved3;[^}]*\} lh264_decode_opts_t;", txt, flags=re.S)
    assert re.search(r"#define LH264_DECODE_OPTS_BYTES_V4 64u", txt)
    for name, value in (("ALL", 0), ("INTRA", 1), ("IDR", 2)):
        assert re.search(r"#define LH264_PICK_%s\s+%du" % (name, value), txt)
    for decl in ("int lh264_decoded_picture_index (const lh264_decoded_t* d, int idx);", "long long lh264_decoded_parsed_slices (const lh264_decoded_t* d);",
                 "int lh264_decode_last_chains (long long v[3]);", "int lh264_parser_pick (const uint8_t* data, size_t len, uint32_t pick, int32_t* idx, int cap, int* n);"):
        assert decl in txt, decl
    assert "NEITHER SEEN NOR REPORTED" in txt      # damage inside an unselected picture: the header says so


def test_arguments_are_checked_before_the_device():
    """every LH264_E_ARG case of pick is reported on a machine without a device (none becomes LH264_E_NODEVICE) and leaves `out` alone;
    a valid pick is accepted (LH264_E_NODEVICE where there is no device); the 64-byte struct does not read what lies behind it"""
    L, lib = _lib()
    data = _read("streams/BA1_Sony_D.jsv")
    ptrs, lens = (C.c_char_p * 1)(data), (C.c_size_t * 1)(len(data))
    outs = (C.c_void_p * 1)()
    sentinel = 0x1234

    def call(o):
        outs[0] = sentinel
        rc = lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(o), outs)
        if rc == 0:
            lib.lh264_decoded_free(outs[0])
        else:
            assert outs[0] == sentinel
        return rc
    import torch
    accepted = 0 if torch.cuda.is_available() else L.E_NODEVICE
    o = L.DecodeOptsV5()
    o.struct_bytes = 72
    for bad in (3, 4, 0x80000000, 0xffffffff):
        o.pick, o.reserved3 = bad, 0
        assert call(o) == L.E_ARG, bad
    for pick in (0, 1, 2):
        o.pick, o.reserved3 = pick, 1
        assert call(o) == L.E_ARG, pick
        o.reserved3 = 0xffffffff
        assert call(o) == L.E_ARG, pick
    o.reserved3 = 0
    for pick in (1, 2):
        for method in sorted(set(L.CONCEAL.values()) - {0}):
            o.pick, o.conceal = pick, method
            assert call(o) == L.E_ARG, (pick, method)
    o.pick, o.conceal, o.reserved2 = 1, 0, 1          # the 64-byte struct's rule holds in the 72-byte struct
    assert call(o) == L.E_ARG
    o.reserved2 = 0
    for pick in (0, 1, 2):
        o.pick = pick
        assert call(o) == accepted, pick
    o.pick, o.conceal = 0, L.CONCEAL["slice_copy"]    # concealment with every picture decoded: as ever
    assert call(o) == accepted
    o.conceal = 0
    # struct_bytes 64 (and 56, 48, 40) with garbage behind: accepted, the new words are not read
    o.pick, o.reserved3 = 0xdeadbeef, 0xdeadbeef
    for nbytes in (64, 56, 48, 40):
        o.struct_bytes = nbytes
        assert call(o) == accepted, nbytes
    o.struct_bytes, o.conceal = 64, L.CONCEAL["slice_copy"]
    o.pick = 1
    assert call(o) == accepted                        # (pick is not read there: no clash with conceal)
    o.conceal = 0
    for nbytes in (68, 76, 80, 0):
        o.struct_bytes, o.pick, o.reserved3 = nbytes, 0, 0
        assert call(o) == L.E_ARG, nbytes
    import losslessh264_amd as lh
    for bad in ("p", 1, None, "IDR"):
        with pytest.raises(ValueError):
            lh.decode_batch([data], pick=bad)
    with pytest.raises(ValueError):
        lh.decode_batch([data], pick="intra", conceal="slice_copy")
    with pytest.raises(ValueError):
        lh.pick(data, "p")
    assert lib.lh264_decoded_picture_index(None, 0) == L.E_ARG and lib.lh264_decoded_parsed_slices(None) == 0
    assert lib.lh264_decode_last_chains(None) == L.E_ARG
    n = C.c_int(-1)
    assert lib.lh264_parser_pick(data, len(data), 3, None, 0, C.byref(n)) == L.E_ARG and n.value == -1
    assert lib.lh264_parser_pick(data, len(data), 1, None, 0, None) == L.E_ARG
    assert lib.lh264_parser_pick(data, len(data), 1, None, 4, C.byref(n)) == L.E_ARG
    assert lib.lh264_parser_pick(data, len(data), 1, None, -1, C.byref(n)) == L.E_ARG


@pytest.mark.parametrize("name", sorted(TABLE))
def test_parser_pick_against_the_full_parse(name):
    """lh264_parser_pick (headers only) selects what the records of the full parse say: every slice an I slice for intra, idr for idr,
    every index for all; the counts and the index lists are those of the table"""
    import __graft_entry__ as g
    g.build()
    import losslessh264_amd as lh
    data = _read(name)
    frames, err, _main = lh.parse_file(data)
    assert err == ""
    intra = [i for i, f in enumerate(frames) if len(f.slices) >= 1 and all(int(t) == 2 for t in f.slices["slice_type"])]
    idr = [i for i, f in enumerate(frames) if f.idr]
    mixed = [i for i, f in enumerate(frames) if len(set(int(t) for t in f.slices["slice_type"])) > 1]
    assert (len(frames), len(intra), len(idr), len(mixed)) == TABLE[name]
    assert lh.pick(data, "intra") == intra and lh.pick(data, "idr") == idr and lh.pick(data, "all") == list(range(len(frames)))
    assert set(idr) <= set(intra) and not set(mixed) & set(intra)
    if name in INTRA_AT:
        assert intra == INTRA_AT[name]
    if name in IDR_AT:
        assert idr == IDR_AT[name]


def test_parser_pick_reports_the_count_when_cap_is_small():
    """cap below the count: the first cap indices are written, nothing behind them, and *n is the count"""
    L, lib = _lib()
    data = _read("streams/MIDR_MW_D.264")
    n = C.c_int(0)
    idx = (C.c_int32 * 8)(*([-7] * 8))
    assert lib.lh264_parser_pick(data, len(data), L.PICK["intra"], idx, 2, C.byref(n)) == 0
    assert n.value == 4 and list(idx) == [0, 30, -7, -7, -7, -7, -7, -7]
    assert lib.lh264_parser_pick(data, len(data), L.PICK["intra"], None, 0, C.byref(n)) == 0 and n.value == 4
    assert lib.lh264_parser_pick(data, len(data), L.PICK["idr"], idx, 8, C.byref(n)) == 0 and n.value == 2 and list(idx)[:3] == [0, 60, -7]
    assert lib.lh264_parser_pick(data, len(data), L.PICK["all"], None, 0, C.byref(n)) == 0 and n.value == 100
    assert lib.lh264_parser_pick(None, 0, L.PICK["all"], None, 0, C.byref(n)) == 0 and n.value == 0      # no stream: no picture


def header_failure_stream():
    """BA_MW_D.264 with the slice of picture 45 turned into a B slice (first_mb_in_slice 0, slice_type 1): the header walk fails there.
    Picture 44 is still in progress then, so 44 pictures were complete (lh264_parser_error_pictures) and the decode call stops at 44"""
    data = _read("streams/BA_MW_D.264")
    starts = [m.start() for m in re.finditer(b"\x00\x00\x01", data)]
    slices = [s for s in starts if data[s + 3] & 31 in (1, 5)]
    assert len(slices) == 100
    at = slices[45]
    return data[:at + 4] + b"\xa8" + data[at + 5:]


def test_parser_pick_stops_at_a_header_failure():
    """a slice header that does not parse ends the choice where the decode call ends the stream: the pictures complete in front of it"""
    import __graft_entry__ as g
    g.build()
    import losslessh264_amd as lh
    cut = header_failure_stream()
    frames, err, _main = lh.parse_file(cut)
    assert err == "only I and P slices are supported"
    assert lh.pick(cut, "intra") == [0, 30] and lh.pick(cut, "idr") == [0, 30] and lh.pick(cut, "all") == list(range(44))


def test_the_command_lines_refuse_pick_with_conceal(tmp_path):
    """--pick takes intra | idr; --pick with --conceal is the usage error: both end the command lines with the usage code before a
    stream is read or a device looked for"""
    src = os.path.join(GOLDEN, "streams", "BA_MW_D.264")
    _lib()
    for cmd in ([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"]):
        for args in (["--pick", "all"], ["--pick", "x"], ["--pick", "intra", "--conceal", "slice_copy"], ["--conceal", "mv_copy", "--sha1", "--pick", "idr"]):
            r = subprocess.run(cmd + ["--decode"] + args + [str(tmp_path), src], capture_output=True, timeout=120, cwd=ROOT)
            assert r.returncode == 2, (cmd, args, r.stdout, r.stderr)
            assert os.listdir(str(tmp_path)) == []
