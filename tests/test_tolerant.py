"""LH264_COMPRESS_TOLERANT on the CPU (include/lh264.h): the default stream keeps the payload of every NAL unit that is no slice, so
that the restorers - untouched - write it back; what cannot be carried has a text; streams without such units get the default stream
they always got.  The tagged streams of the modified streams are those of the unmodified ones (tests/golden/cli_*.npz): units that
are no slices reach no model."""
import ctypes as C
import os

import numpy as np
import pytest

import golden_io
import tolerant_cases as T
import losslessh264_amd as lh
from losslessh264_amd import _lib as L

R = __import__("sys").modules["losslessh264_amd.restore"]


def _golden_tags(base):
    z = np.load(os.path.join(golden_io.GOLDEN_DIR, "cli_%s.npz" % base))
    return z["main"].tobytes(), {int(k[4:]): z[k].tobytes() for k in z.files if k.startswith("tag_")}


CASES = [(b, c) for b in T.BASES for c in T.EXTRA]


@pytest.mark.parametrize("base,case", CASES)
def test_default_stream_with_the_flag_restores_through_every_host_path(base, case):
    """the test that fails without the flag: restore (default stream, tags of the unmodified stream) is the modified stream"""
    data, units = T.extra(base, case)
    main0, tags = _golden_tags(base)
    assert lh.parse_file(T.data(base))[2] == main0                 # (the fixture is this stream's)
    frames, err, main = lh.parse_file(data, tolerant=True)
    assert err == "" and lh.not_carried(data) == ""
    assert lh.restore(main, tags) == data
    assert R.restore_batch([(main, tags)]) == [data]
    for cabac_device in (False, True):
        outs, paths = R.restore_batch_cpu_check([(main, tags)], cabac_device=cabac_device)
        assert outs == [data], (cabac_device, paths)


@pytest.mark.parametrize("base,case", CASES)
def test_without_the_flag_exactly_the_payload_bytes_are_missing(base, case):
    data, units = T.extra(base, case)
    main_on = lh.parse_file(data, tolerant=True)[2]
    main_off = lh.parse_file(data)[2]
    assert main_off == T.without_payloads(main_on, units)
    payload = sum(len(u) - len(k) for u, k in units)
    assert len(main_on) - len(main_off) == payload
    first = next((u for u, k in units if len(u) > len(k)), None)
    text = lh.not_kept(data)
    if first is None:                                              # (types 10 and 11: a header byte and nothing else)
        assert payload == 0 and text == "" and main_on == main_off
        assert lh.restore(main_off, _golden_tags(base)[1]) == data
    else:
        at = data.index(first) + len(T.SC)
        assert "nal_unit_type %d, header byte at offset %d)" % (first[len(T.SC)] & 31, at) in text, text
        assert text.startswith("NAL unit %d " % (data[:at].count(b"\x00\x00\x01") - 1)), text
        # ... and without the flag the result is not the input (what LH264_OK stood for before)
        try:
            assert lh.restore(main_off, _golden_tags(base)[1]) != data
        except RuntimeError:
            pass


@pytest.mark.parametrize("base", T.BASES)
def test_what_cannot_be_carried_has_a_text(base):
    data, _ = T.extra(base, "slice_first")
    text = lh.not_carried(data)
    assert text.startswith("NAL unit 0 (nal_unit_type 5, header byte at offset 4): a slice in front of its parameter sets") and "cannot be carried" in text
    assert lh.not_kept(data).startswith("NAL unit 0 (nal_unit_type 5")
    data, units = T.extra(base, "forbidden")
    text = lh.not_carried(data)
    at = data.index(units[0][0]) + len(T.SC)
    assert "(nal_unit_type 9, header byte at offset %d): the forbidden_zero_bit is set" % at in text and "cannot be carried" in text
    assert lh.not_kept(data) != ""
    # a stream whose PPS never comes: its first slice is named.  A slice whose header names a PPS other than the one that came: the
    # parser's own text, with the flag and without
    plain = T.data(base)
    pps = next(u for u in T.nal_units(plain) if u[2] == 8)
    assert lh.not_carried(plain[:pps[0]] + plain[pps[1]:]).startswith("NAL unit 1 (nal_unit_type 5")
    s = T.Synth(2, 2)
    s.picture([dict(first_mb=0, type="I", qp=26, pps=1, mbs=[T._intra(k, 0) for k in range(4)])], idr=True)
    for tolerant in (False, True):
        assert "missing PPS" in lh.parse_file(s.bytes(), tolerant=tolerant)[1]
    for b in (plain,) + tuple(T.extra(base, c)[0] for c in T.EXTRA):
        assert lh.not_carried(b) == ""


def test_all_44_streams_get_the_same_default_stream_with_the_flag():
    """no shipped stream holds a unit whose bytes the default stream drops; the flag changes nothing for them"""
    import test_sweep
    named = {}
    for name in test_sweep.STREAMS:
        d = test_sweep._data(name)
        f0, e0, m0 = lh.parse_file(d)
        f1, e1, m1 = lh.parse_file(d, tolerant=True)
        assert (e0, m0, len(f0)) == (e1, m1, len(f1)), name
        if lh.not_kept(d) or lh.not_carried(d):
            named[name] = lh.not_kept(d) or lh.not_carried(d)
    assert len(test_sweep.STREAMS) == 44 and named == {}, named


def test_the_flag_must_be_set_before_the_first_byte():
    lib = L.lib()
    p = lib.lh264_parser_create()
    try:
        d = T.data("BA_MW_D.264")
        assert lib.lh264_parser_set_tolerant(p, 1) == 0 and lib.lh264_parser_set_tolerant(p, 0) == 0
        lib.lh264_parser_feed_file(p, d, len(d))
        assert lib.lh264_parser_set_tolerant(p, 1) == -2           # LH264_E_ARG
        assert lib.lh264_parser_not_kept(p) == b"" and lib.lh264_parser_not_carried(p) == b""
    finally:
        lib.lh264_parser_destroy(p)
    assert lib.lh264_parser_set_tolerant(None, 1) == -2 and lib.lh264_parser_not_kept(None) == b""


def test_options_struct_rejects_unknown_bits_as_before():
    """bit 1 is LH264_COMPRESS_TOLERANT now; every other unknown bit, alone or beside the known ones, is LH264_E_ARG before anything
    is looked at (no device is needed for the answer)"""
    lib = L.lib()
    assert L.COMPRESS_ESCAPES == 1 and L.COMPRESS_TOLERANT == 2 and lib.lh264_abi_version() == 3
    d = b""
    ptrs, lens, outs = (C.c_char_p * 1)(d), (C.c_size_t * 1)(0), (C.c_void_p * 1)()
    devs = (C.c_int * 1)(0)
    for flags in (4, 8, 1 << 31, 2 | 4, 1 | 2 | 4, 0xfffffffc):
        opts = L.CompressOpts(C.sizeof(L.CompressOpts), flags, 0)
        assert lib.lh264_compress_batch_opts(ptrs, lens, 1, 1, C.byref(opts), outs) == -2, flags
        assert lib.lh264_compress_batch_devices_opts(ptrs, lens, 1, 1, devs, 1, C.byref(opts), outs) == -2, flags
    hdr = open(os.path.join(os.path.dirname(golden_io.GOLDEN_DIR), "..", "include", "lh264.h")).read()
    assert "#define LH264_COMPRESS_TOLERANT 2u" in hdr and "#define LH264_ABI_VERSION 3" in hdr


@pytest.mark.parametrize("name", T.SYNTHETIC)
def test_synthetic_lost_slice_streams_lose_what_they_are_named_after(name):
    """the front end parses them without an error, and the macroblocks no slice covers are the ones the case stands for"""
    frames, err, main = lh.parse_file(T.lost(name), tolerant=True)
    assert err == ""
    got = {i: [int(k) for k in np.flatnonzero(f.covered == 0)] for i, f in enumerate(frames) if not f.covered.all()}
    assert got == T.UNCOVERED[name]
    for i, f in enumerate(frames):
        assert (f.mbs["mb_type"][f.covered == 0] == 0).all() and (f.mbs["mb_type"][f.covered != 0] != 0).all(), i
    if name == "nonref":
        assert [f.frame_num for f in frames] == [0, 1, 1, 2, 2] and [f.is_ref for f in frames] == [True, False, True, False, True]
    if name == "resize":
        assert [(f.mb_w, f.mb_h) for f in frames] == [(4, 3)] * 3 + [(5, 3)] * 3
    # P_Skip in every P picture that kept the slice with it, and a residual in every coded macroblock
    assert sum(int((f.mbs["mb_type"] == 0x100).sum()) for f in frames) >= 3          # LH264_MB_SKIP
    for f in frames:
        coded = (f.covered != 0) & (f.mbs["mb_type"] != 0x100)
        assert (np.abs(f.levels[coded]).sum(axis=1) > 0).all()


@pytest.mark.parametrize("name", T.SYNTHETIC)
def test_keep_rule_restores_on_the_cpu(name):
    """the rule restated on the host (tolerant_cases.cpu_compress: a cell no slice writes keeps the entry of the picture that held its
    buffer before) gives files that the restorers - the host restore and the kernel's code stepped on the host - turn back into the
    input.  tests/test_tolerant_gpu.py holds the kernels to these bytes"""
    d = T.lost(name)
    main, tags = T.cpu_compress(d)
    assert lh.restore(main, tags) == d
    outs, paths = R.restore_batch_cpu_check([(main, tags)])
    assert outs == [d], paths
    assert len(main) + sum(len(b) for b in tags.values()) < len(d)


def test_keep_policy_names_the_buffers_previous_picture():
    class F:
        def __init__(self, fn, w=4, h=3):
            self.frame_num, self.mb_w, self.mb_h = fn, w, h
    # every picture a reference picture: KEEP is two flips back
    assert T.keep_policy([F(0), F(1), F(2), F(3)]) == ([None, 0, 1, 2], [None, None, 0, 1])
    # frame_num repeats behind a non-reference picture: KEEP is the picture directly before, PAST stays
    assert T.keep_policy([F(0), F(1), F(1), F(2), F(2)]) == ([None, 0, 0, 2, 2], [None, None, 1, 0, 3])
    # a change of size: both buffers start again
    assert T.keep_policy([F(0), F(1), F(2), F(0, 5), F(1, 5), F(2, 5)]) == ([None, 0, 1, None, 3, 4], [None, None, 0, None, None, 3])
