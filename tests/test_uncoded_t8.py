"""Macroblocks that code nothing under the 8x8 transform, without a device: I_NxN with transform_size_8x8_flag 1 and
coded_block_pattern 0 - the one macroblock that carries the flag and has no mb_qp_delta, so that its QP is the one carried from the
macroblock before (7.4.5) - and the inter macroblocks of a PPS with transform_8x8_mode_flag 1 whose flag is not transmitted.  The
streams of tests/golden/uncoded_t8/ (tests/golden/make_uncoded_t8_streams.py) through the host parser, the oracle's reconstruction,
the CPU forms of the device parsers, the compress direction and every restore path, against the unmodified reference's recorded verdict
(tests/golden/uncoded_t8_ref.json).  Every comparison is bytes against bytes.

One stream, i8_cbp0_cavlc_i_stale, is decoded otherwise by the reference, and the tests say exactly how: its CAVLC reader of I slices
leaves the QP entries of such a macroblock as the picture before wrote them."""
import os
import sys

import numpy as np
import pytest

import losslessh264_amd as lh
import uncoded_t8_cases as U
from losslessh264_amd import slice_parse as SP
from test_slice_parse import cpu_form_against_host, same_as_plain

R = sys.modules["losslessh264_amd.restore"]
TYPE_OF = dict(i8=U.MB_I8, i8u=U.MB_I8, i4=U.MB_I4, i16=U.MB_I16, pcm=U.MB_IPCM, skip=U.MB_SKIP, p16=U.MB_P16x16, p16t8=U.MB_P16x16, p16x8=U.MB_P16x8, p8x16=U.MB_P8x16,
               p8x8=U.MB_P8x8)
# the QP the reference's filter read for the I8x8 macroblock without coefficients of a first picture: what its allocator left there
REFERENCE_FIRST_PICTURE_QP = 0
# tags of the compress direction's files that differ from the reference's: 6 is the stream whose prior reads the luma QP of the
# macroblock, which in the reference is the same entry that the picture before left
FILES_DIFFER = {U.STALE: {6}}


def test_the_set():
    assert U.NAMES == sorted(["i8_cbp0_cavlc_p", "i8_cbp0_cabac", "i8_cbp0_cavlc_i_same", "i8_cbp0_cavlc_i_stale", "inter_t8_absent_cavlc", "inter_t8_absent_cabac"])
    assert sorted(os.listdir(U.DIR)) == [n + ".264" for n in U.NAMES]
    assert all(len(U.data(n)) < 4096 for n in U.NAMES)
    # only one stream may be exempt from equality with the reference, and the reference refused none
    assert U.NOT_AS_THE_REFERENCE == (U.STALE,)
    assert all(U.REF[n]["decode_rc"] == 0 and U.REF[n]["dump_rc"] == 0 for n in U.NAMES)


@pytest.mark.parametrize("name", U.NAMES)
def test_stream_regenerates_byte_for_byte(name):
    d = U.data(name)
    assert U.made()[name][0] == d
    assert (len(d), U.sha(d)) == (U.REF[name]["bytes"], U.REF[name]["sha1"])
    assert U.REF[name]["yuv_bytes"] == U.made()[name][1]["pictures"] * U.PIC_BYTES == len(U.REF[name]["picture_sha1"]) * U.PIC_BYTES


# ---- what the writers reached --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["i8_cbp0_cavlc_p", "i8_cbp0_cabac"])
def test_writer_reached_every_place_of_the_uncoded_i8x8_macroblock(name):
    c = U.made()[name][1]
    u = c["u8"]
    assert u["n"] == 18
    assert u["first"] == {0, 8}                                                  # the first macroblock of a slice, one of them mid-picture
    assert u["avail"] == {(l, t) for l in "L-" for t in "T-"}                    # left only and top only among them
    assert u["beside"] == {"i8", "i8u", "i4", "i16", "pcm", "p16", "p16t8", "skip"}
    assert u["pairs"] >= 2 and u["last_slice"] >= 2 and u["last_pic"] >= 1
    # the carried QP is neither the slice's nor pic_init_qp; and 0 and 51
    assert (43, 40, 28) in u["carried"] and {0, 51} <= {q for q, _, _ in u["carried"]}
    assert all(36 <= q <= 45 or q in (0, 51) for q, _, _ in u["carried"])
    assert any(d for _, d in u["behind"] if d) and {("i8", -2), ("i16", 1), ("p16", -5)} <= u["behind"]
    assert u["deblock"] == {0, 1, 2}
    assert u["slice"] == ({"I", "P"} if name.endswith("cabac") else {"P"})
    assert (c["qp_min"], c["qp_max"]) == (0, 51)
    if name.endswith("cabac"):
        i8 = c["i8"]
        assert i8["cbp0"] and all(set(luma) <= set(range(73, 77)) and 77 <= chroma <= 80 for luma, chroma in i8["cbp0"])
        assert i8["cbp_nb"] & set(range(73, 77)) and i8["cbp_nb"] & set(range(77, 85))
        assert i8["dqp_behind"] == {0} and set(c["dqp"]["inc"]) == {0}           # ... behind a macroblock with a non-zero delta in front of it
        assert i8["t8_nb"] >= {1, 2} and set(c["t8_inc"]) == {0, 1, 2}
        assert i8["first"] >= {0, 8} and i8["slice"] == {"I", "P"}


@pytest.mark.parametrize("name", ["i8_cbp0_cavlc_i_same", "i8_cbp0_cavlc_i_stale"])
def test_writer_reached_the_i_slice_cases(name):
    u = U.made()[name][1]["u8"]
    stale = name == U.STALE
    assert u["n"] == 6 + stale and u["slice"] == {"I"} and u["pairs"] == 2 and u["last_pic"] == 1
    assert {q for q, _, _ in u["carried"]} == {42, 38, 43, 36} | ({44} if stale else set())
    # the picture in front: a coded macroblock at every place under test, at the carried QP (same) or 12 below it (stale)
    log = u["log"]
    assert len(log) == 3 + stale                                                 # (the first picture,) the earlier one, the one under test, a skipped one
    early, late = log[-3], log[-2]
    under = [k for k in range(U.N) if late[k][0] == "i8u"]
    assert under == [1, 2, 5, 7, 10, 11]
    for k in under:
        assert early[k][0] == "i16" and early[k][3] == late[k][3] - (12 if stale else 0)
    if stale:
        assert [k for k in range(U.N) if log[0][k][0] == "i8u"] == [5]


@pytest.mark.parametrize("name", ["inter_t8_absent_cavlc", "inter_t8_absent_cabac"])
def test_writer_reached_the_inter_cases(name):
    c = U.made()[name][1]
    u = c["u8"]
    want = [(kind, False, cbp_c, None, None) for kind in ("p16", "p16x8", "p8x16") for cbp_c in (0, 1, 2)]       # no flag
    want += [("p8x8", True, 0, (0, 0, 0, 0), 0), ("p8x8", True, 0, (0, 0, 0, 0), 1)]                           # the flag present, 0 and 1
    assert all(w in u["between"] for w in want)
    # a sub type below 8x8 with cbp_l 15: the flag is absent
    assert any(k[0] == "p8x8" and k[1] and k[4] is None and any(k[3]) for k in u["between"])
    assert {s for k in u["inter"] if k[3] for s in k[3]} == {0, 1, 2, 3}
    assert u["i8u_between"] and u["n"] == 3 and u["slice"] == {"P"}
    if name.endswith("cabac"):
        assert set(c["t8_inc"]) == {0, 1, 2}                                     # the increments of the next flag
    else:
        assert {cls for cls, _, _, _ in c["coeff_token"]} >= {0, 1, 2}           # nC classes next to interleaved 8x8 blocks


# ---- the host parser -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.NAMES)
def test_host_parser_reads_what_was_written(name):
    """every macroblock's type, flag, coded_block_pattern and QP as the writer logged them: the macroblocks under test carry the QP of
    the macroblock before, and the macroblock behind them the QP that follows from it"""
    r = U.parsed(name)
    assert r.error == "" and r.status == 0
    log = U.made()[name][1]["u8"]["log"]
    assert len(r.frames) == len(log)
    seen = 0
    for f, pic in zip(r.frames, log):
        assert f.covered.all() and (f.mb_w, f.mb_h) == (U.MB_W, U.MB_H)
        for k, (label, t8, cbp, qp) in enumerate(pic):
            m = f.mbs[k]
            assert int(m["mb_type"]) == TYPE_OF[label], (k, label)
            assert int(m["flags"]) & 1 == t8, (k, label)
            if label == "pcm":
                assert int(m["qp_y"]) == 0
                continue
            assert int(m["qp_y"]) == qp and [int(v) for v in m["qp_c"]] == [U.CHROMA_QP[qp]] * 2, (k, label, qp)
            if label not in ("skip", "i16"):
                assert int(m["cbp"]) == cbp, (k, label)
            uncoded_under_t8 = label == "i8u" or (label in ("p16", "p16x8", "p8x16", "p8x8") and not cbp & 15)
            if uncoded_under_t8:
                assert not (cbp & 15) and not m["nzc"][:16].any() and (cbp or not m["nzc"].any())
                seen += 1
    assert seen >= 3
    assert U.i8u(r.frames) == [(i, k) for i, pic in enumerate(log) for k, e in enumerate(pic) if e[0] == "i8u"]


# ---- pictures --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in U.NAMES if n not in U.NOT_AS_THE_REFERENCE])
def test_oracle_pictures_equal_the_references(name):
    got = U.pictures(name)
    assert [U.sha(p) for p in got] == U.REF[name]["picture_sha1"]
    assert U.sha(b"".join(got)) == U.REF[name]["yuv_sha1"]
    assert U.REF[name]["dump_picture_sha1"] == U.REF[name]["picture_sha1"]
    # ... and the QP the reference held when it reconstructed is the parser's, for every macroblock
    for i, f in enumerate(U.parsed(name).frames):
        assert [int(v) for v in f.mbs["qp_y"]] == U.REF[name]["dump_qp_y"][i], i


def _stale_qps():
    """{(picture, macroblock): (qp_y, qp_c)}: for the macroblocks under test of the stale stream, what the picture decoded before holds
    at their place; for the first picture, what the reference's allocator left"""
    frames = U.parsed(U.STALE).frames
    out = {}
    for i, k in U.i8u(frames):
        if i == 0:
            out[(i, k)] = (REFERENCE_FIRST_PICTURE_QP, U.CHROMA_QP[REFERENCE_FIRST_PICTURE_QP])
        else:
            out[(i, k)] = (int(frames[i - 1].mbs["qp_y"][k]), int(frames[i - 1].mbs["qp_c"][k][0]))
    return out


def test_stale_stream_first_check_the_reference_filters_with_the_qp_of_the_picture_before():
    frames = U.parsed(U.STALE).frames
    ref = U.REF[U.STALE]
    ours = [U.sha(p) for p in U.pictures(U.STALE)]
    under = U.i8u(frames)
    assert [i for i, _ in under] == [0] + [2] * 6
    # as 7.4.5 has it, the pictures with such macroblocks differ from the reference's (and the picture that copies the last of them)
    assert [a == b for a, b in zip(ours, ref["picture_sha1"])] == [False, True, False, False]
    stale = _stale_qps()
    assert all(abs(frames[i].mbs["qp_y"][k] - qy) >= 10 for (i, k), (qy, _) in stale.items())
    # the reference's own arrays say so: at the macroblocks under test, and nowhere else, it held another QP than the parser's
    for i, f in enumerate(frames):
        for k in range(U.N):
            want = stale[(i, k)] if (i, k) in stale else (int(f.mbs["qp_y"][k]), int(f.mbs["qp_c"][k][0]))
            assert (ref["dump_qp_y"][i][k], ref["dump_qp_c"][i][k]) == want, (i, k)
    # with exactly those entries overwritten the oracle reproduces the reference's pictures byte for byte, the first picture included
    again = U.oracle_pictures(frames, stale)
    assert [U.sha(p) for p in again] == ref["picture_sha1"]
    assert b"".join(again) == open(os.path.join(U.golden_io.GOLDEN_DIR, "uncoded_t8_stale_ref.yuv"), "rb").read()


def test_stale_stream_second_check_the_difference_lies_where_those_entries_are_read():
    """the samples that differ from the reference's pictures (as its debug dump and its console application wrote them, one file) lie
    where a filter that reads those entries can write: an edge is filtered with the average of both macroblocks' QP and changes at most
    three samples on either side (8.7.2), so the macroblock under test itself (its inner edge, and its side of its four outer edges),
    three columns / rows of its right and lower neighbours (their left / upper edge) and three of its left and upper neighbours (its own
    left / upper edge, whose far side lies in them) - and the 3 x 3 corners between those, where a neighbour's other edge filters across
    the samples that its edge against the macroblock under test has just changed.  Nothing further away differs"""
    frames = U.parsed(U.STALE).frames
    theirs = open(os.path.join(U.golden_io.GOLDEN_DIR, "uncoded_t8_stale_ref.yuv"), "rb").read()
    assert len(theirs) == 4 * U.PIC_BYTES and U.sha(theirs) == U.REF[U.STALE]["yuv_sha1"]
    assert [U.sha(theirs[i:i + U.PIC_BYTES]) for i in range(0, len(theirs), U.PIC_BYTES)] == U.REF[U.STALE]["dump_picture_sha1"]
    under = U.i8u(frames)
    for i in (0, 2):
        diff = [a != b for a, b in zip(U.planes(U.pictures(U.STALE)[i]), U.planes(theirs[i * U.PIC_BYTES:(i + 1) * U.PIC_BYTES]))]
        assert diff[0].any() and diff[1].any()                                   # luma and chroma
        for p, d in enumerate(diff):
            s = 8 if p else 16
            allowed = np.zeros_like(d)
            for _, k in (u for u in under if u[0] == i):
                x, y = (k % U.MB_W) * s, (k // U.MB_W) * s
                allowed[max(y - 3, 0):y + s + 3, max(x - 3, 0):x + s + 3] = True
            assert not (d & ~allowed).any(), (i, p, np.argwhere(d & ~allowed)[:4])
            # every macroblock under test shows it
            if p == 0:
                for _, k in (u for u in under if u[0] == i):
                    x, y = (k % U.MB_W) * s, (k // U.MB_W) * s
                    assert d[y:y + s, x:x + s].any(), (i, k)


# ---- the CPU forms of the device parsers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.NAMES)
def test_cpu_forms_of_the_device_parsers(name):
    data = U.data(name)
    cabac = name in U.CABAC
    a, b = SP.parse_file_plain(data), SP.parse_file_plain(data, deferred=True, cabac=cabac)
    same_as_plain(a, b)
    slices = sum(len(f.slices) for f in b.frames)
    assert sum(len(d) for d in b.deferred) == slices and all(ok for d in b.deferred for _, ok, _ in d)
    pics, guards, _ = SP.slice_parse(data, threads=4, cabac=cabac)
    assert cpu_form_against_host(b, pics, guards) == slices
    assert all(int(q.results[s][1]) == 0 for q in pics for s in range(q.n_deferred))
    if not cabac:
        # the entry with the CABAC switch on parses a CAVLC stream the same
        pics, guards, _ = SP.slice_parse(data, threads=4, cabac=True)
        assert cpu_form_against_host(SP.parse_file_plain(data, deferred=True, cabac=True), pics, guards) == slices


# ---- compress and restore ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.NAMES)
def test_compress_on_the_cpu_and_every_restore_returns_the_input(name):
    """host symbols + the oracle's coefficient symbols through the oracle's coder; lh264_pip_restore; the restore kernels' code stepped
    on the host with the CAVLC writer alone (a CABAC stream is then the host's) and with both writers"""
    main, tags = U.cpu_compress(name)
    d = U.data(name)
    assert lh.out_of_range(d) == ""
    assert lh.restore(main, tags) == d
    outs, paths, st = R.restore_batch_cpu_check([(main, tags)], 1, None, statuses=True)
    assert st[0][0] == 0 and outs == [d] and paths == [R.PATH_HOST if name in U.CABAC else R.PATH_DEVICE]
    outs, paths, st = R.restore_batch_cpu_check([(main, tags)], 1, None, statuses=True, cabac_device=True)
    assert st[0][0] == 0 and outs == [d] and paths == [R.PATH_DEVICE]


def test_all_streams_restore_in_one_call():
    items = [U.cpu_compress(n) for n in U.NAMES]
    outs, paths = R.restore_batch_cpu_check(items, 4, None, cabac_device=True)
    assert outs == [U.data(n) for n in U.NAMES] and paths == [R.PATH_DEVICE] * len(U.NAMES)


@pytest.mark.parametrize("name", U.NAMES)
def test_files_against_the_references(name):
    """the compress direction's files against those the reference wrote.  What was found: they are the reference's byte for byte, but
    for tag 6 of the stale stream - the stream of mb_qp_delta, whose prior reads the luma QP of macroblocks decoded before: the
    reference's entry for an I8x8 macroblock without coefficients in a CAVLC I slice is the stale one there too.  (Its own restore
    returns three of the six streams; every restore of this code returns all six.)"""
    main, tags = U.cpu_compress(name)
    ref = U.REF[name]["files"]
    ours = {t: b for t, b in tags.items() if t != U.E.TAG_PCM and b}
    assert {str(t) for t in ours} == {k for k in ref if k != "main"}
    assert U.sha(main) == ref["main"][1]
    assert {t for t in ours if U.sha(ours[t]) != ref[str(t)][1]} == FILES_DIFFER.get(name, set())
    assert U.REF[name]["reference_roundtrip"] == (name in ("i8_cbp0_cavlc_i_same", "i8_cbp0_cavlc_i_stale", "inter_t8_absent_cabac"))
