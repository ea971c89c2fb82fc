"""CAVLC slice data apart from the header walk, without a device: the parser's deferred mode gives what the plain parser gives, and
the one piece of code that parses slice data for the device (csrc/lh264_slice.h), stepped on the host by lh264_debug_slice_parse,
gives the host parser's records, coefficients, n_mbs and stop positions - and a status instead of them exactly where the host
parser fails."""
import functools

import numpy as np
import pytest

import slice_parse_cases as K
from losslessh264_amd import _lib as L
from losslessh264_amd import slice_parse as SP

COMMITTED = K.committed()


def same_as_plain(a, b):
    """the deferred parser with every slice run through parse_deferred (b) against the plain parser (a)"""
    assert (b.error, b.status, b.error_pictures, len(b.frames)) == (a.error, a.status, a.error_pictures, len(a.frames))
    for i, (x, y) in enumerate(zip(a.frames, b.frames)):
        assert (x.id, x.mb_w, x.mb_h, x.frame_num, x.is_ref, x.idr, x.ref_ids) == (y.id, y.mb_w, y.mb_h, y.frame_num, y.is_ref, y.idr, y.ref_ids), i
        for k in ("mbs", "coeffs", "slices", "covered"):
            assert getattr(x, k).tobytes() == getattr(y, k).tobytes(), "picture %d: %s differs" % (i, k)
        # (a slice that failed has no entry in the slice syntax table: the table is short, and only whole tables are read)
        if all(ok for _, ok, _ in b.deferred[i]):
            assert x.slice_syn.tobytes() == y.slice_syn.tobytes(), "picture %d: slice syntax differs" % i


def cpu_form_against_host(b, pics, guards):
    """the CPU form's dump against the deferred parser's pictures after parse_deferred (b): a status exactly where the host fails,
    the host's bytes wherever it does not.  -> the number of slices compared"""
    assert guards, "guard bytes were overwritten"
    assert len(pics) == len(b.frames)
    n = 0
    for i, (y, q) in enumerate(zip(b.frames, pics)):
        assert q.n_deferred == len(b.deferred[i])
        for sid, ok, stop in b.deferred[i]:
            deferred, status, n_mbs, stop_bit = [int(v) for v in q.results[sid]]
            assert deferred == 1
            assert (status == 0) == ok, "picture %d slice %d: status %d, the host %s" % (i, sid, status, "parses" if ok else "fails")
            if not ok:
                assert status == L.SLICE_SYNTAX
                continue
            n += 1
            first = int(y.slices[sid]["first_mb"])
            assert (n_mbs, stop_bit) == (int(y.slices[sid]["n_mbs"]), stop), (i, sid)
            assert q.slices[sid].tobytes() == y.slices[sid].tobytes(), (i, sid)
            # a later slice of a damaged picture may overwrite the host's records where this one ran on; the range it owns is its own
            last = first + n_mbs
            if sid + 1 < len(y.slices):
                last = min(last, int(y.slices[sid + 1]["first_mb"]))
            assert q.mbs[first:last].tobytes() == y.mbs[first:last].tobytes(), "picture %d slice %d: records differ" % (i, sid)
            assert q.coeffs[first:last].tobytes() == y.coeffs[first:last].tobytes(), "picture %d slice %d: coefficients differ" % (i, sid)
        if b.deferred[i] and all(ok for _, ok, _ in b.deferred[i]):
            assert q.mbs.tobytes() == y.mbs.tobytes() and q.coeffs.tobytes() == y.coeffs.tobytes() and q.slices.tobytes() == y.slices.tobytes(), i
    return n


@pytest.mark.parametrize("name,path", COMMITTED, ids=[n for n, _ in COMMITTED])
def test_committed_stream(name, path):
    """1: deferred mode is invisible.  2: the CPU form equals the host parser, all 128 bytes of every record, guards intact"""
    data = open(path, "rb").read()
    a, b = SP.parse_file_plain(data), SP.parse_file_plain(data, deferred=True)
    same_as_plain(a, b)
    if not any(b.deferred):
        return                                   # a CABAC stream: nothing was deferred
    pics, guards, _ = SP.slice_parse(data, threads=4)
    assert cpu_form_against_host(b, pics, guards) > 0


def test_deferred_mode_off_by_default():
    data = K.read("streams/SVA_BA2_D.264")
    a = SP.parse_file_plain(data)
    assert not any(a.deferred) and all(f.covered.all() for f in a.frames)


# ---- 3: what the committed CAVLC streams reach -------------------------------------------------------------------------------------
COVER = ("streams/BA_MW_D.264", "streams/SVA_Base_B.264", "streams/CVFC1_Sony_C.jsv", "streams/MR1_BT_A.h264", "streams/CVPCMNL1_SVA_C.264",
         "streams/tibby8x8cavlc.264", "streams/test_scalinglist_jm.264", "streams/BASQP1_Sony_C.jsv", "edge/qp_edges.264", "edge/nref_2_3_15.264", "slice_parse/i8_first.264")
MB = dict(I4=0x1, I16=0x2, I8=0x4, P16x16=0x8, P16x8=0x10, P8x16=0x20, P8x8=0x40, P8x8REF0=0x80, SKIP=0x100, IPCM=0x200)


@functools.lru_cache(maxsize=None)
def coverage():
    seen = set()
    for name in COVER:
        r = SP.parse_file_plain(K.read(name), deferred=True)
        for f, d in zip(r.frames, r.deferred):
            if not d:
                continue                                # only what the CAVLC layer parsed counts
            m, cov = f.mbs, f.covered != 0
            t = m["mb_type"]
            for key, bit in (("I4", 1), ("I16", 2), ("I8", 4)):
                sel = m[(t == bit) & cov]
                for av in np.unique(sel["intra_avail"] & 5):       # LH264_AVAIL_T | LH264_AVAIL_L
                    seen.add((key, "L" if av & 4 else "-", "T" if av & 1 else "-"))
                # with the upper neighbour there, the upper-right one decides the DDL / VL remaps (finalize_intra_modes) of the NxN types
                if key != "I16":
                    for av in np.unique(sel["intra_avail"][(sel["intra_avail"] & 1) != 0] & 8):
                        seen.add((key, "T", "TR" if av else "noTR"))
                    for mode, name in ((12, "ddl_top"), (13, "vl_top")):
                        if (sel["intra_mode"] == mode).any():
                            seen.add((key, name))
            for key, bit in MB.items():
                if ((t == bit) & cov).any():
                    seen.add(key)
            p8 = m[((t == 0x40) | (t == 0x80)) & cov]
            for s in np.unique(p8["sub_type"]):
                seen.add("sub%d" % s)
            sk = m[(t == 0x100) & cov]
            if len(sk):
                moved = (sk["mv"].reshape(len(sk), -1) != 0).any(axis=1)
                seen.add("skip_inferred") if moved.any() else None
                seen.add("skip_zero") if (~moved).any() else None
            for nr in f.slices["n_refs"][f.slices["slice_type"] == 0]:
                seen.add("nref2" if nr == 2 else "nref>2" if nr > 2 else "nref1")
            if ((m["flags"] & 1) != 0).any():
                seen.add("t8")
                # under a PPS with transform_8x8_mode_flag 1 (a macroblock of the picture has the flag): an inter macroblock without
                # luma coefficients, whose flag is not transmitted
                if ((t & 0xf8) != 0)[((m["cbp"] & 15) == 0) & ((m["flags"] & 1) == 0) & cov].any():
                    seen.add("inter_t8_absent")
            if ((t == 4) & (m["cbp"] == 0) & cov).any():
                seen.add(("I8", "cbp0"))                 # no mb_qp_delta: the QP is the one carried from the macroblock before
            if (f.slices["luma_dc_weight"] != 16).any():
                seen.add("scaling")
            if len(f.slices) > 1:
                seen.add("multi_slice")
            if (f.slices["first_mb"] % f.mb_w != 0).any():
                seen.add("mid_row")
            coded = f.syn[f.syn["have"] == 1]
            # mb_qp_delta lies in -26..25: a QP further than that from the QP before it went round the end of 0..51
            d = coded["luma_qp"].astype(int) - coded["last_mb_qp"]
            if ((np.abs(d) > 26) & (coded["mb_type"] != 0x200)).any():
                seen.add("qp_wrap")
    return seen


WANT = ([(k, l, t) for k in ("I4", "I16", "I8") for l in "L-" for t in "T-"] + [(k, "T", r) for k in ("I4", "I8") for r in ("TR", "noTR")] +
        [(k, m) for k in ("I4", "I8") for m in ("ddl_top", "vl_top")] + list(MB) + ["sub1", "sub2", "sub4", "sub8", "skip_inferred", "skip_zero",
        "nref2", "nref>2", "t8", "scaling", "multi_slice", "mid_row", "qp_wrap", ("I8", "cbp0"), "inter_t8_absent"])


@pytest.mark.parametrize("what", WANT, ids=[str(w) for w in WANT])
def test_coverage(what):
    assert what in coverage()


def test_synthetic_stream_is_the_generator_s_and_decodes_as_the_reference_decodes_it():
    """tests/golden/slice_parse/i8_first.264 (I8x8 as a slice's first macroblock: no committed CAVLC stream had one): the file is what
    tests/golden/make_slice_parse_streams.py writes, and the host parser's records reconstruct, through the oracle, to the pictures the
    unmodified reference wrote for it (tests/golden/slice_parse_ref.json)"""
    import hashlib
    import importlib.util
    import json
    import os
    import oracle_lib as O
    spec = importlib.util.spec_from_file_location("make_slice_parse_streams", os.path.join(K.GOLDEN, "make_slice_parse_streams.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    ref = json.load(open(os.path.join(K.GOLDEN, "slice_parse_ref.json")))
    made = gen.build()
    assert sorted(made) == sorted(ref) == sorted(f[:-4] for f in os.listdir(os.path.join(K.GOLDEN, "slice_parse")))
    for name, (data, _) in made.items():
        assert data == K.read("slice_parse/%s.264" % name)
        assert (len(data), hashlib.sha1(data).hexdigest()) == (ref[name]["bytes"], ref[name]["sha1"]) and ref[name]["decode_rc"] == 0
        r = SP.parse_file_plain(data)
        assert r.error == ""
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


# ---- 4: statuses ------------------------------------------------------------------------------------------------------------------
DAMAGED = K.damaged_cases()


@pytest.mark.parametrize("label,data", DAMAGED, ids=[l for l, _ in DAMAGED])
def test_damaged_slice(label, data):
    a, b = SP.parse_file_plain(data), SP.parse_file_plain(data, deferred=True)
    same_as_plain(a, b)
    pics, guards, _ = SP.slice_parse(data, threads=2)
    cpu_form_against_host(b, pics, guards)


def test_damaged_cases_fail_and_pass():
    """the 20 cases are not all of one kind: some make the host fail, some leave a stream that still parses"""
    failed = [bool(SP.parse_file_plain(d, deferred=True).error) for _, d in DAMAGED]
    assert any(failed) and not all(failed)


def test_error_stream():
    data = K.read("streams/Error_I_P.264")
    a, b = SP.parse_file_plain(data), SP.parse_file_plain(data, deferred=True)
    same_as_plain(a, b)
    pics, guards, _ = SP.slice_parse(data, threads=2)
    cpu_form_against_host(b, pics, guards)


def test_overrun():
    """a slice whose limit lies in front of where its data ends: OVERRUN, and nothing at or beyond the limit is written"""
    data = K.head(K.read("streams/SVA_Base_B.264"), 6)
    ref, guards, _ = SP.slice_parse(data)
    assert guards and len(ref[0].slices) >= 2 and (ref[0].results[:, 1] == 0).all()
    first1 = int(ref[0].slices[1]["first_mb"])
    assert int(ref[0].slices[0]["n_mbs"]) == first1
    for limit in (first1 - 1, first1 - 7, 1):
        pics, guards, _ = SP.slice_parse(data, tweak=(0, 0, limit))
        q = pics[0]
        assert guards
        assert int(q.results[0][1]) == L.SLICE_OVERRUN and int(q.results[0][2]) <= limit
        assert not q.mbs[limit:first1].tobytes().strip(b"\0") and not q.coeffs[limit:first1].any()
        # the other slices are what they were
        assert q.mbs[first1:].tobytes() == ref[0].mbs[first1:].tobytes() and (q.results[1:] == ref[0].results[1:]).all()
    # a limit that is no limit at all is an inconsistent task: a status, nothing touched
    pics, guards, _ = SP.slice_parse(data, tweak=(0, 0, 0))
    assert guards and int(pics[0].results[0][1]) == L.SLICE_BAD_TASK and not pics[0].mbs[:first1].tobytes().strip(b"\0")


# ---- 5: the arguments of the decode call --------------------------------------------------------------------------------------------
def test_decode_opts_parse_argument():
    """parse 2 is LH264_E_ARG, struct_bytes 40 and 48 are accepted and mean host - all of it before a device is looked for (on a
    machine without one an accepted call answers LH264_E_NODEVICE, never LH264_E_ARG)"""
    import ctypes as C
    lib = L.lib()
    data = K.read("streams/SVA_BA2_D.264")
    ptrs, lens, outs = (C.c_char_p * 1)(data), (C.c_size_t * 1)(len(data)), (C.c_void_p * 1)()

    def call(struct_bytes, parse, conceal=0):
        o = L.DecodeOptsV3()
        o.struct_bytes, o.parse, o.conceal = struct_bytes, parse, conceal
        o.reserved0 = 0xdeadbeef                             # what was tail padding: never read
        rc = lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(o), outs)
        if rc == 0:
            lib.lh264_decoded_free(outs[0])
        return rc
    assert C.sizeof(L.DecodeOptsV3) == 56 and C.sizeof(L.DecodeOpts) == L.DECODE_OPTS_BYTES_V2 == 48 and L.DECODE_OPTS_BYTES_V1 == 40
    assert L.DecodeOptsV3.parse.offset == 48
    for bad in (2, 3, 0xffffffff):
        assert call(56, bad) == L.E_ARG
        assert call(48, bad) in (0, L.E_NODEVICE) and call(40, bad) in (0, L.E_NODEVICE)       # the old structs: the field is not read
    for ok in (0, 1):
        assert call(56, ok) in (0, L.E_NODEVICE) and call(56, ok, conceal=6) in (0, L.E_NODEVICE)
    assert call(52, 0) == L.E_ARG and call(60, 0) == L.E_ARG and call(44, 0) == L.E_ARG
    for flag in (2, 16):                                     # still not defined
        o = L.DecodeOptsV3()
        o.struct_bytes, o.flags, o.parse = 56, flag, 1
        assert lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(o), outs) == L.E_ARG
    import losslessh264_amd as lh
    with pytest.raises(ValueError):
        lh.decode_batch([data], parse="gpu")
    assert lib.lh264_decoded_parse_path(None) == L.E_ARG
