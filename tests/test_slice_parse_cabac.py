"""CABAC slice data apart from the header walk, without a device: with both defer switches on the parser gives what the plain parser
gives, and the code that parses CABAC slice data for the device (csrc/lh264_slice_cabac.h), stepped on the host by
lh264_debug_slice_parse_opts, gives the host parser's records, coefficients, n_mbs and stop positions - and a status instead of them
exactly where the host parser fails."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import slice_parse_cabac_cases as KC
import slice_parse_cases as K
from losslessh264_amd import _lib as L
from losslessh264_amd import slice_parse as SP
from test_slice_parse import MB, cpu_form_against_host, same_as_plain

FIXTURES = [("slice_parse_cabac/" + f, os.path.join(K.GOLDEN, "slice_parse_cabac", f)) for f in sorted(os.listdir(os.path.join(K.GOLDEN, "slice_parse_cabac")))]
COMMITTED = K.committed() + FIXTURES
CABAC_CORPUS = ("streams/test_qcif_cabac.264", "streams/tibbycabac.264", "streams/test_cif_I_CABAC_slice.264", "streams/test_cif_P_CABAC_slice.264",
                "streams/QCIF_2P_I_allIPCM.264")


@pytest.mark.parametrize("name,path", COMMITTED, ids=[n for n, _ in COMMITTED])
def test_committed_stream(name, path):
    """1: deferred mode is invisible, with both switches and with the old one alone, under which a CABAC stream defers nothing.
    2: the CPU form equals the host parser for every CABAC slice, all 128 bytes of every record, guards intact"""
    a, b, c = KC.parsed(name)
    same_as_plain(a, b)
    same_as_plain(a, c)
    assert not KC.has_cabac(c)
    assert [len(d) for d in b.deferred] == [len(f.slices) for f in b.frames] or b.error
    if name.startswith(("cabac_edge/", "slice_parse_cabac/")) or name in CABAC_CORPUS:
        assert KC.has_cabac(b)
        # the old switch: only the CAVLC slices (cabac_mixed.264 has some), never a CABAC one
        assert sum(len(d) for d in c.deferred) == sum(len(d) - sum(m) for d, m in zip(b.deferred, b.deferred_cabac))
    if not KC.has_cabac(b):
        return
    pics, guards, _ = SP.slice_parse(K.read(name), threads=4, cabac=True)
    assert cpu_form_against_host(b, pics, guards) > 0
    # ... and at least one of the slices compared was a CABAC one that the host parses
    assert any(ok and m for d, ms in zip(b.deferred, b.deferred_cabac) for (_, ok, _), m in zip(d, ms))


def test_old_entry_defers_no_cabac_slice():
    """lh264_debug_slice_parse is unchanged in effect: a CABAC stream defers nothing"""
    pics, guards, _ = SP.slice_parse(K.read("cabac_edge/cabac_skip.264"))
    assert guards and pics and all(p.n_deferred == 0 for p in pics)
    lib = L.lib()
    h = C.c_void_p()
    data = K.read("cabac_edge/cabac_skip.264")
    assert lib.lh264_debug_slice_parse(data, len(data), 0, 1, None, C.byref(h)) == 0
    assert sum(_info(lib, h, i)[3] for i in range(lib.lh264_slice_dump_pictures(h))) == 0
    lib.lh264_slice_dump_free(h)
    assert lib.lh264_debug_slice_parse_opts(data, len(data), 4, 1, None, C.byref(h)) == L.E_ARG


def _info(lib, h, i):
    info = (C.c_int32 * 4)()
    L.check(lib.lh264_slice_dump_picture(h, i, info))
    return [int(x) for x in info]


# ---- 3: what the committed CABAC pictures reach ----------------------------------------------------------------------------------------
COVER = CABAC_CORPUS + tuple(n for n, _ in COMMITTED if n.startswith(("cabac_edge/", "slice_parse_cabac/")))


@functools.lru_cache(maxsize=None)
def coverage():
    seen = set()
    for name in COVER:
        _, r, _ = KC.parsed(name)
        data = K.read(name)
        spans = [e - a for a, e in K.nal_spans(data) if data[a] & 31 in (1, 5)]
        for f, d, marks in zip(r.frames, r.deferred, r.deferred_cabac):
            if not d or not all(marks):
                continue                                # only pictures the CABAC layer parsed count
            m, cov = f.mbs, f.covered != 0
            t = m["mb_type"]
            for key, bit in MB.items():
                if ((t == bit) & cov).any():
                    seen.add(key)
            for key, bit in (("I4", 1), ("I16", 2), ("I8", 4)):
                for av in np.unique(m[(t == bit) & cov]["intra_avail"] & 5):
                    seen.add((key, "L" if av & 4 else "-", "T" if av & 1 else "-"))
            seen |= i8_syntax(f, cov)
            for s in np.unique(m[(t == 0x40) & cov]["sub_type"]):
                seen.add("sub%d" % s)
            for nr in f.slices["n_refs"][f.slices["slice_type"] == 0]:
                seen.add("nref2" if nr == 2 else "nref>2" if nr > 2 else "nref1")
            if (((m["flags"] & 1) != 0) & ((t & 0xf8) != 0) & cov).any():
                seen.add("t8_inter")
            if len(f.slices) > 1:
                seen.add("multi_slice")
            if (f.slices["first_mb"] % f.mb_w != 0).any():
                seen.add("mid_row")
            if f.mb_w > 256:
                seen.add("wider_than_256")
                # both neighbours in the slice at the columns where the line index passes 255
                for col in (255, 256):
                    k = f.mb_w + col
                    if cov[k] and m["slice_id"][k] == m["slice_id"][k - 1] == m["slice_id"][k - f.mb_w]:
                        seen.add(("wide_both_neighbours", col))
        if has_long_payload(spans, r):
            seen.add("payload>4096")
    return seen


RAW_MODE = {9: 2, 10: 2, 11: 2, 12: 3, 13: 7}                   # the availability-resolved modes of a record back to Intra8x8PredMode


def i8_syntax(f, cov):
    """what the syntax of the I8x8 macroblocks of a picture must have held, from the records: ("I8_first",) for one that starts a slice,
    ("I8_t8_inc", n) and ("I8_mb_type_inc", n) for the ctxIdxInc of its transform_size_8x8_flag and (I slices) of its mb_type,
    ("I8_prev", flag) per 8x8 block from the prediction of 8.3.2.1, ("I8_pred_from", "left" or "top") where the neighbouring macroblock's
    mode was the smaller one"""
    seen = set()
    m, w = f.mbs, f.mb_w
    first = {int(x) for x in f.slices["first_mb"]}

    def raw(k, blk):
        if m["mb_type"][k] not in (1, 4):
            return 2
        v = int(m["intra_mode"][k][(blk >> 1) * 8 + (blk & 1) * 2])
        return RAW_MODE.get(v, v)
    for k in np.flatnonzero((m["mb_type"] == 4) & cov):
        k = int(k)
        sid = m["slice_id"][k]
        A = k - 1 if k % w and cov[k - 1] and m["slice_id"][k - 1] == sid else None
        B = k - w if k >= w and cov[k - w] and m["slice_id"][k - w] == sid else None
        if k in first:
            seen.add(("I8_first",))
        seen.add(("I8_t8_inc", sum(1 for N in (A, B) if N is not None and m["flags"][N] & 1)))
        if f.slices["slice_type"][sid] == 2:
            seen.add(("I8_mb_type_inc", sum(1 for N in (A, B) if N is not None and m["mb_type"][N] not in (1, 4))))
        assert m["mb_type"][[N for N in (A, B) if N is not None]].tolist().count(1) == 0         # (an I4x4 neighbour's modes: not needed so far)
        for blk in range(4):
            bx, by = blk & 1, blk >> 1
            if not ((bx or A is not None) and (by or B is not None)):
                pred = 2
            else:
                ma = raw(k, blk - 1) if bx else raw(A, blk + 1)
                mb = raw(k, blk - 2) if by else raw(B, blk + 2)
                pred = min(ma, mb)
                if not bx and ma < mb:
                    seen.add(("I8_pred_from", "left"))
                if not by and mb < ma:
                    seen.add(("I8_pred_from", "top"))
            seen.add(("I8_prev", int(raw(k, blk) == pred)))
    return seen


def has_long_payload(spans, r):
    return KC.has_cabac(r) and max(spans) > 4096


WANT = ["I4", "I16", "IPCM", "P16x16", "P16x8", "P8x16", "P8x8", "SKIP", "sub1", "sub2", "sub4", "sub8", "nref1", "nref2", "nref>2", "t8_inter",
        "multi_slice", "mid_row", "payload>4096", "wider_than_256", ("wide_both_neighbours", 255), ("wide_both_neighbours", 256)] + [(k, l, t) for k in ("I4", "I16", "I8") for l in "L-" for t in "T-"] + \
       [("I8_first",), ("I8_prev", 0), ("I8_prev", 1), ("I8_pred_from", "left"), ("I8_pred_from", "top")] + [(k, n) for k in ("I8_t8_inc", "I8_mb_type_inc") for n in (0, 1, 2)]


@pytest.mark.parametrize("what", WANT, ids=[str(w) for w in WANT])
def test_coverage(what):
    assert what in coverage()


# ---- 4: statuses ------------------------------------------------------------------------------------------------------------------
DAMAGED = KC.damaged_cases()


@pytest.mark.parametrize("label,data", DAMAGED, ids=[l for l, _ in DAMAGED])
def test_damaged_slice(label, data):
    a, b = SP.parse_file_plain(data), SP.parse_file_plain(data, deferred=True, cabac=True)
    same_as_plain(a, b)
    pics, guards, _ = SP.slice_parse(data, threads=2, cabac=True)
    cpu_form_against_host(b, pics, guards)


def test_damaged_cases_fail_and_pass():
    """the 20 cases are not all of one kind: some make the host fail (counted when the cases were chosen: 9, "CABAC error"), some leave
    a stream that still parses"""
    failed = [bool(SP.parse_file_plain(d, deferred=True, cabac=True).error) for _, d in DAMAGED]
    assert any(failed) and not all(failed)


def test_multi_slice_pictures():
    data = KC.multi_slice()
    a, b = SP.parse_file_plain(data), SP.parse_file_plain(data, deferred=True, cabac=True)
    same_as_plain(a, b)
    assert any(len(d) > 1 for d in b.deferred) and KC.has_cabac(b) and not b.error
    pics, guards, _ = SP.slice_parse(data, threads=4, cabac=True)
    assert cpu_form_against_host(b, pics, guards) == sum(len(d) for d in b.deferred)


def test_overrun_and_inconsistent_tasks():
    """a CABAC slice whose limit lies in front of where its data ends: OVERRUN, and nothing at or beyond the limit is written; limit 0
    and a task whose entropy-mode byte names an undefined cabac_init_idc (or no CABAC at all): BAD_TASK, nothing touched"""
    data = KC.overrun_input()
    ref, guards, _ = SP.slice_parse(data, cabac=True)
    assert guards and len(ref) == 1 and len(ref[0].slices) >= 2 and (ref[0].results[:, 0] == 1).all() and (ref[0].results[:, 1] == 0).all()
    first1 = int(ref[0].slices[1]["first_mb"])
    assert int(ref[0].slices[0]["n_mbs"]) == first1 > 8
    for limit in (first1 - 1, first1 - 7, 1):
        pics, guards, _ = SP.slice_parse(data, tweak=(0, 0, limit), cabac=True)
        q = pics[0]
        assert guards
        assert int(q.results[0][1]) == L.SLICE_OVERRUN and int(q.results[0][2]) <= limit
        assert q.mbs[:int(q.results[0][2])].tobytes() == ref[0].mbs[:int(q.results[0][2])].tobytes()
        assert not q.mbs[limit:first1].tobytes().strip(b"\0") and not q.coeffs[limit:first1].any()
        assert q.mbs[first1:].tobytes() == ref[0].mbs[first1:].tobytes() and (q.results[1:] == ref[0].results[1:]).all()
    for tweak in ((0, 0, 0), (0, 0, first1, 0x83), (0, 0, first1, 0x84), (0, 0, first1, 0x40), (0, 0, first1, 0)):
        pics, guards, _ = SP.slice_parse(data, tweak=tweak, cabac=True)
        assert guards and int(pics[0].results[0][1]) == L.SLICE_BAD_TASK and not pics[0].mbs[:first1].tobytes().strip(b"\0"), tweak
        assert pics[0].mbs[first1:].tobytes() == ref[0].mbs[first1:].tobytes()
    # the byte as the entry fills it in is accepted when it is written back unchanged
    idc = [d for d in (0x80, 0x81, 0x82) if SP.slice_parse(data, tweak=(0, 0, first1, d), cabac=True)[0][0].results[0][1] == 0]
    assert len(idc) >= 1


# ---- 6: the arguments of the decode call --------------------------------------------------------------------------------------------
def test_decode_opts_parse_flags_argument():
    """parse_flags: an undefined bit, or the CABAC flag with parse = host, is LH264_E_ARG; struct_bytes 40 and 48 do not read the field -
    all of it before a device is looked for (on a machine without one an accepted call answers LH264_E_NODEVICE)"""
    lib = L.lib()
    data = K.read("cabac_edge/cabac_skip.264")
    ptrs, lens, outs = (C.c_char_p * 1)(data), (C.c_size_t * 1)(len(data)), (C.c_void_p * 1)()

    def call(struct_bytes, parse, parse_flags):
        o = L.DecodeOptsV3()
        o.struct_bytes, o.parse, o.parse_flags = struct_bytes, parse, parse_flags
        rc = lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(o), outs)
        if rc == 0:
            lib.lh264_decoded_free(outs[0])
        return rc
    assert C.sizeof(L.DecodeOptsV3) == 56 and L.DecodeOptsV3.parse_flags.offset == 52 and L.PARSE == {"host": 0, "device": 1}
    for bad in (2, 3, 0x80000001, 0xffffffff):
        assert call(56, 1, bad) == L.E_ARG and call(56, 0, bad) == L.E_ARG
        assert call(48, 1, bad) in (0, L.E_NODEVICE) and call(40, 0, bad) in (0, L.E_NODEVICE)
    assert call(56, 0, 1) == L.E_ARG
    assert call(56, 1, 1) in (0, L.E_NODEVICE) and call(56, 1, 0) in (0, L.E_NODEVICE) and call(56, 0, 0) in (0, L.E_NODEVICE)
    assert call(48, 0, 1) in (0, L.E_NODEVICE) and call(40, 0, 1) in (0, L.E_NODEVICE)
    import losslessh264_amd as lh
    with pytest.raises(ValueError):
        lh.decode_batch([data], parse="device+gpu")
    assert lib.lh264_decoded_device_cabac_slices(None) == 0


# ---- 7: the generator -----------------------------------------------------------------------------------------------------------------
def test_synthetic_streams_are_the_generator_s_and_decode_as_the_reference_decodes_them():
    """tests/golden/slice_parse_cabac/: the files are what tests/golden/make_slice_parse_cabac_streams.py writes, its counters show what
    it reached, and the host parser's records reconstruct, through the oracle, to the pictures the unmodified reference wrote
    (tests/golden/slice_parse_cabac_ref.json; a file the reference refused is held to its return code only)"""
    import hashlib
    import importlib.util
    import json
    import oracle_lib as O
    spec = importlib.util.spec_from_file_location("make_slice_parse_cabac_streams", os.path.join(K.GOLDEN, "make_slice_parse_cabac_streams.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ref = json.load(open(os.path.join(K.GOLDEN, "slice_parse_cabac_ref.json")))
    made = gen.build()
    assert sorted(made) == sorted(ref) == sorted(f[:-4] for f in os.listdir(os.path.join(K.GOLDEN, "slice_parse_cabac")))
    for name, (data, count) in made.items():
        assert data == K.read("slice_parse_cabac/%s.264" % name)
        assert (len(data), hashlib.sha1(data).hexdigest()) == (ref[name]["bytes"], ref[name]["sha1"])
        r = SP.parse_file_plain(data)
        assert r.error == ""
        if ref[name].get("decode_rc") != 0:
            continue
        h, pics, total = hashlib.sha1(), {}, 0
        for f in r.frames:
            dst = O.HostPic(f.mb_w, f.mb_h)
            O.recon_frame(f.mbs, f.coeffs, f.slices, dst, [pics[q] for q in f.ref_ids], 0)
            pics[f.id] = dst
            for p in range(3):
                b = np.ascontiguousarray(dst.plane(p)).tobytes()
                h.update(b)
                total += len(b)
        assert (total, h.hexdigest()) == (ref[name]["yuv_bytes"], ref[name]["yuv_sha1"])
    count = made["cabac_i8"][1]
    i8 = count["i8"]
    assert i8["avail"] == {(l, t) for l in "L-" for t in "T-"} and i8["first"] == {0, 6} and i8["slice"] == {"I", "P"}
    assert set(count["t8_inc"]) == {0, 1, 2} and {n for kind, n in count["mb_type_inc"] if kind == "i8"} == {0, 1, 2}
    assert i8["prev"][0] > 0 and i8["prev"][1] > 0 and i8["pred"] == {0, 1, 2} and i8["from_left"] and i8["from_top"] and {0, 7} <= i8["rem"]
    assert {c for c, _ in count["last_pos"]} >= {3, 4, 5} and (5, 63) in count["last_pos"] and max(v for (c, v) in count["abs_level"] if c == 5) >= 14
    count = made["cabac_wide"][1]
    assert count["pictures"] == 3 and len(count["pcm_phase"]) >= 1 and count["mvd"]["max"] > 0 > count["mvd"]["min"] and set(count["skip_inc"]) == {0, 1, 2}
    assert {c for c, _ in count["cbf_pcm"]} and count["slice_qp"] >= {("I", 28), ("I", 30), (1, 28), (2, 27)}
