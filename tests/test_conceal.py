"""Concealment of lost slices, the host side: the records the front end writes for macroblocks no slice covered, the freeze and
delivery flags against the reference (tests/golden/conceal/ref.json), the option checks, and that nothing changes without the option.
No device is needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import losslessh264_amd as lh
from losslessh264_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "conceal")
REF = json.load(open(os.path.join(DIR, "ref.json")))
METHODS = ["slice_copy", "slice_copy_cross_idr", "slice_copy_cross_idr_freeze", "mv_copy", "mv_copy_freeze"]
NAMES = sorted(n for n in REF if n != "error_i_p")


def stream(name):
    return open(os.path.join(DIR, name + ".264"), "rb").read()


def sizes(m):
    """[w, h] per delivered picture of a ref.json method entry (`size` where they are all alike)"""
    return m["sizes"] if "sizes" in m else [m["size"]] * len(m["sha1"])


def cdiv(a, b):
    """C integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def i16(v):
    return ((v + 0x8000) & 0xffff) - 0x8000


def mean_vector(f):
    """GetAvilInfoFromCorrectMb (error_concealment.cpp:246-362) for ref_idx 0, restated over the parser's own records"""
    sx = sy = n = 0
    for k in np.flatnonzero(f.covered):
        m = f.mbs[k]
        t = int(m["mb_type"])
        if t in (0x0100, 0x0008):
            parts = [(0, 0)]
        elif t == 0x0010:
            parts = [(0, 0), (2, 8)]
        elif t == 0x0020:
            parts = [(0, 0), (1, 2)]
        elif t in (0x0040, 0x0080):
            parts = []
            for i in range(4):
                b = ((i >> 1) << 3) + ((i & 1) << 1)
                parts += [(i, b + o) for o in {1: [0], 2: [0, 4], 4: [0, 1], 8: [0, 1, 4, 5]}.get(int(m["sub_type"][i]), [])]
        else:
            continue
        for quad, blk in parts:
            if int(m["ref_idx"][quad]) == 0:
                sx += int(m["mv"][blk][0]); sy += int(m["mv"][blk][1]); n += 1
    return (cdiv(sx, n), cdiv(sy, n), n) if n else (0, 0, 0)


def clamp(f, k, vec):
    """DoMbECMvCopy's window arithmetic (error_concealment.cpp:207-240), the top offset twice as there"""
    px, py = (k % f.mb_w) * 16, (k // f.mb_w) * 16
    left, right, top, bottom = f.crop_x, f.crop_x + f.crop_w, f.crop_y, f.mb_h * 16 - f.crop_y
    fx, fy = (px << 2) + vec[0], (py << 2) + vec[1]
    if fx < (left + 2) << 2:
        fx = max(left, (fx >> 2) << 2)
    elif fx > (right - 19) << 2:
        fx = min((right - 17) << 2, (fx >> 2) << 2)
    if fy < (top + 2) << 2:
        fy = max(top, (fy >> 2) << 2)
    elif fy > (bottom - 19) << 2:
        fy = min((bottom - 17) << 2, (fy >> 2) << 2)
    return fx - (px << 2), fy - (py << 2)


@pytest.mark.parametrize("method", ["slice_copy", "slice_copy_cross_idr", "mv_copy"])
@pytest.mark.parametrize("name", NAMES)
def test_concealment_records(name, method):
    frames, err, _ = lh.parse_file(stream(name), conceal=method)
    plain = lh.parse_file(stream(name))[0]
    assert err == "" and len(frames) == len(plain)
    lost = {int(k): v for k, v in REF[name]["lost"].items()}
    mv_copy = method == "mv_copy"
    for i, (f, g) in enumerate(zip(frames, plain)):
        assert f.concealed == lost.get(i, 0) == int((f.covered == 0).sum()), i
        assert np.array_equal(f.covered, g.covered)
        rec = f.covered != 0
        assert np.array_equal(f.mbs[rec], g.mbs[rec]), "received macroblocks keep their records"
        if not f.concealed:
            assert len(f.slices) == len(g.slices) and np.array_equal(f.mbs, g.mbs)
            continue
        # the source: the picture decoded before this one, or 128s (no such picture; an IDR picture under plain slice copy)
        want_src = -1 if i == 0 or (method == "slice_copy" and f.idr) else frames[i - 1].id
        assert f.conceal_src == want_src
        assert len(f.slices) == len(g.slices) + 1
        sl = f.slices[-1]
        assert sl["deblock_idc"] == 1 and sl["weighted_pred"] == 0 and sl["slice_type"] == 0 and sl["n_mbs"] == f.concealed
        slot = int(sl["ref_slot"][0])
        assert 0 <= slot < 16
        assert (f.ref_ids[slot] == want_src) if want_src >= 0 else slot >= len(f.ref_ids)
        # the vector: mean of ref_idx 0, scaled by the POC distances where list entry 0 is not the source, clamped per macroblock
        # Which of the three it is, and the POCs, come from the frames: entry 0 of list 0 of the picture's last P slice through that
        # slice's ref_slot and the picture's ref_ids, every picture's POC from its own record (lh264_parser_frame_conceal [11])
        info = [int(x) for x in f.conceal_info]
        mx, my, n = mean_vector(f)
        vec = (0, 0)
        if mv_copy:
            assert (info[3], info[4]) == (mx, my)
        poc = {q.id: q.poc for q in frames}
        p_slices = [s for s in f.slices[:-1] if s["slice_type"] == 0]
        l0 = -1
        if p_slices and 0 <= int(p_slices[-1]["ref_slot"][0]) < len(f.ref_ids):
            l0 = f.ref_ids[int(p_slices[-1]["ref_slot"][0])]
        mode = 0 if not (mv_copy and want_src >= 0 and not f.idr and n and l0 >= 0) else 1 if l0 == want_src else 2
        assert info[10] == mode, (i, info, l0, want_src)
        if mode:
            assert (info[7], info[8], info[9]) == (f.poc, poc[l0], poc[want_src])
            if mode == 1:
                vec = (i16(mx), i16(my))
            else:
                s0, s1 = poc[l0] - f.poc, poc[want_src] - f.poc
                vec = (0, 0) if s0 == 0 else (i16(cdiv(mx * s1, s0)), i16(cdiv(my * s1, s0)))
            assert (info[5], info[6]) == vec
        for k in np.flatnonzero(f.covered == 0):
            m = f.mbs[k]
            assert int(m["mb_type"]) == 0x0408 and int(m["cbp"]) == 0 and int(m["slice_id"]) == len(f.slices) - 1
            assert list(m["ref_idx"]) == [0, 0, 0, 0]
            want = clamp(f, int(k), vec) if info[10] else (0, 0)
            assert all((int(m["mv"][b][0]), int(m["mv"][b][1])) == want for b in range(16)), (i, int(k), want)
        # the picture is held one picture longer than its marking says: the next picture may need it as a source
        if i + 1 < len(frames) and frames[i + 1].concealed:
            assert frames[i + 1].conceal_src == f.id


def test_mean_scaling_and_clamp_are_reached():
    """the fixtures reach every branch of the vector: a non-zero mean, the crop window's clamp, the POC scaling"""
    modes, clamped = set(), False
    for name in ("sva_tail5", "cvfc1_tail", "mr1bt_tail"):
        for f in lh.parse_file(stream(name), conceal="mv_copy")[0]:
            if f.concealed:
                info = [int(x) for x in f.conceal_info]
                modes.add(info[10])
                mvs = {(int(m["mv"][0][0]), int(m["mv"][0][1])) for m in f.mbs[f.covered == 0]}
                clamped |= any(v != (info[5], info[6]) for v in mvs)
    assert modes == {1, 2} and clamped


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", NAMES + ["error_i_p"])
def test_freeze_and_delivery_flags(name, method):
    data = stream(name) if name != "error_i_p" else open(os.path.join(HERE, "golden", "streams", "Error_I_P.264"), "rb").read()
    frames = lh.parse_file(data, conceal=method)[0]
    ref = REF[name]["methods"][method]
    delivered = [f for f in frames if not f.frozen]
    if "freeze" not in method:
        assert len(delivered) == len(frames)
    if name == "error_i_p":
        # The stream's last picture is damaged.  At the end of a stream the reference's drain does not conceal and does not deliver
        # such a picture; the front end conceals it like any other.  Under the freeze methods it is withheld anyway:
        # nothing before the first whole IDR picture (the third), and nothing again from the damaged IDR picture that changes the size
        assert [f.frozen for f in frames] == ([True, True, False, False, True, True] if "freeze" in method else [False] * 6)
        if "freeze" not in method:
            assert frames[-1].concealed
            delivered = delivered[:-1]
    assert len(delivered) == len(ref["sha1"])
    assert [[f.crop_w, f.crop_h] for f in delivered] == sizes(ref)
    # a picture we conceal is one the reference reports as concealed (its flag also covers pictures that only reference one)
    for f, st in zip(delivered, ref["states"]):
        assert not f.concealed or st & 0x20


def test_option_checks():
    lib = L.lib()
    data = stream("sva_tail5")
    ptrs = (C.c_char_p * 1)(data)
    lens = (C.c_size_t * 1)(len(data))
    outs = (C.c_void_p * 1)()

    def call(struct_bytes, conceal):
        o = L.DecodeOpts()
        o.struct_bytes, o.conceal = struct_bytes, conceal
        rc = lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(o), outs)
        if rc == 0:
            lib.lh264_decoded_free(outs[0])
        return rc
    assert C.sizeof(L.DecodeOpts) == 48 and L.DECODE_OPTS_BYTES_V1 == 40
    for bad in (1, 3, 8, 0xffffffff):                  # FRAME_COPY, FRAME_COPY_CROSS_IDR, no method at all
        assert call(48, bad) == L.E_ARG
        assert call(40, bad) != L.E_ARG                # the old struct: the field is not read
    assert call(44, 0) == L.E_ARG and call(52, 0) == L.E_ARG
    for ok in (0, 2, 4, 5, 6, 7):
        assert call(48, ok) in (0, L.E_NODEVICE)
    p = lib.lh264_parser_create()
    try:
        assert lib.lh264_parser_set_conceal(p, 1) == L.E_ARG and lib.lh264_parser_set_conceal(p, 3) == L.E_ARG
        assert lib.lh264_parser_set_conceal(p, 6) == 0
    finally:
        lib.lh264_parser_destroy(p)
    with pytest.raises(ValueError):
        lh.parse_file(data, conceal="frame_copy")
    with pytest.raises(ValueError):
        lh.decode_batch([data], conceal="frame_copy")


def test_off_is_todays_parse():
    """without a method the records of a damaged picture are what they were: type 0 where no slice covered, no extra slice, and the
    picture's marking alone decides what is held"""
    for name in ("sva_tail5", "sva_idr_tail"):
        frames, err, _ = lh.parse_file(stream(name))
        assert err == ""
        k = int(next(iter(REF[name]["lost"])))
        f = frames[k]
        assert f.concealed == 0 and f.conceal_src == -1 and not f.frozen
        assert (f.covered == 0).sum() == REF[name]["lost"][str(k)]
        assert not f.mbs[f.covered == 0].tobytes().strip(b"\0")
        assert len(f.slices) == 2
