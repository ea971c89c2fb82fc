"""Streams for LH264_COMPRESS_TOLERANT (include/lh264.h), built at test time from committed ones: NAL units the default stream drops
without the flag, and pictures with lost slices.  The acceptance is the round trip, so nothing here needs the reference.

Two families:
  extra(base, case)   `base` (BA_MW_D.264, CAVLC; test_qcif_cabac.264, CABAC) with NAL units put in that are no slices and no
                      parameter sets.  -> (bytes, [(unit as inserted, what the default stream keeps of it WITHOUT the flag)])
  lost(name)          a stream with slice NAL units left out: synthetic ones of 4x3 macroblocks written with tests/h264_synth.py
                      (three slices a picture, a nonzero residual in every coded macroblock that differs from macroblock to macroblock
                      and from picture to picture - so that an nnz entry taken from the wrong picture is another entry - and some
                      P_Skip), and committed ones.  -> bytes
"""
import os
import re

import h264_synth as S

HERE = os.path.dirname(os.path.abspath(__file__))
STREAMS = os.path.join(HERE, "golden", "streams")
SC = b"\x00\x00\x00\x01"


def data(name):
    return open(os.path.join(STREAMS, name), "rb").read()


# ---- NAL units of an Annex-B stream -----------------------------------------------------------------------------------------------
def nal_units(b):
    """[(begin, end, nal_unit_type, first_mb_in_slice or None)]: begin includes the start code and its leading zero byte"""
    starts = [m.start() for m in re.finditer(b"\x00\x00\x01", b)]
    begins = [p - 1 if p > 0 and b[p - 1] == 0 else p for p in starts]
    out = []
    for i, p in enumerate(starts):
        end = begins[i + 1] if i + 1 < len(starts) else len(b)
        t = b[p + 3] & 31
        first_mb = None
        if t in (1, 5):
            bits = "".join(format(x, "08b") for x in b[p + 4:p + 12])
            z = bits.index("1")
            first_mb = int(bits[z:2 * z + 1], 2) - 1
        out.append((begins[i], end, t, first_mb))
    return out


def pictures(units):
    """indices of the slice NAL units per picture: a picture begins at a slice with first_mb_in_slice 0, or - behind a lost first
    slice - where first_mb_in_slice does not grow (true of every stream used here)"""
    pics, last = [], None
    for i, u in enumerate(units):
        if u[2] in (1, 5):
            if not pics or u[3] == 0 or u[3] <= last:
                pics.append([])
            pics[-1].append(i)
            last = u[3]
    return pics


def cut(b, n_pictures):
    """the stream up to and including its first n_pictures pictures"""
    units = nal_units(b)
    pics = pictures(units)
    return b if len(pics) <= n_pictures else b[:units[pics[n_pictures][0]][0]]


def drop(b, drops):
    """drops: [(picture, slice index within the picture; negative: from its end)] -> the stream without those NAL units"""
    units = nal_units(b)
    pics = pictures(units)
    gone = {pics[p][s % len(pics[p])] for p, s in drops}
    return b"".join(b[u[0]:u[1]] for i, u in enumerate(units) if i not in gone)


def insert(b, where):
    """where: {index of a NAL unit: bytes to put in front of it}; index len(units): behind the last one"""
    units = nal_units(b)
    out = bytearray(b[:units[0][0]])
    for i, u in enumerate(units):
        out += where.get(i, b"") + b[u[0]:u[1]]
    return bytes(out + where.get(len(units), b""))


# ---- NAL units the default stream drops --------------------------------------------------------------------------------------------
AUD = SC + b"\x09\xf0"
FILLER = SC + b"\x0c\xff\xff\x80"
# a filler whose payload needs an emulation prevention byte (FF 00 00 01 FF 80 in the RBSP) and has two trailing zero bytes behind it
FILLER_EPB = SC + b"\x0c\xff\x00\x00\x03\x01\xff\x80" + b"\x00\x00"
EXTRA = ["aud", "filler", "eos", "t14", "t24", "pps_first"]
REFUSED = ["slice_first", "forbidden"]
BASES = ["BA_MW_D.264", "test_qcif_cabac.264"]


def _kept_without_flag(unit):
    """the header byte, and the trailing zero bytes"""
    body = unit[len(SC):]
    tz = len(body) - len(body.rstrip(b"\x00"))
    return SC + body[:1] + b"\x00" * tz


def extra(base, case):
    b = data(base)
    units = nal_units(b)
    pics = pictures(units)
    slices = [i for p in pics for i in p]
    if case == "aud":                                    # a delimiter in front of every picture
        put = {p[0]: AUD for p in pics}
    elif case == "filler":                               # between slices; one with an escape inside and zero bytes behind
        put = {slices[1]: FILLER, slices[2]: FILLER_EPB, slices[5]: FILLER}
    elif case == "eos":                                  # end of sequence in the middle, end of stream at the end: no payload at all
        put = {slices[3]: SC + b"\x0a", len(units): SC + b"\x0b"}
    elif case == "t14":                                  # a prefix NAL unit with three payload bytes
        put = {slices[1]: SC + b"\x6e\x40\x80\x07"}
    elif case == "t24":
        put = {slices[2]: SC + b"\x18\xaa\xbb\xcc\xdd\xee"}
    elif case == "pps_first":                            # the stream's own PPS once more, in front of the first SPS
        sps = next(i for i, u in enumerate(units) if u[2] == 7)
        pps = next(u for u in units if u[2] == 8)
        put = {sps: SC + b[pps[0]:pps[1]].lstrip(b"\x00")[1:].rstrip(b"\x00")}
    elif case == "slice_first":                          # refused: a slice in front of the SPS
        sps = next(i for i, u in enumerate(units) if u[2] == 7)
        u = units[slices[0]]
        put = {sps: SC + b[u[0]:u[1]].lstrip(b"\x00")[1:].rstrip(b"\x00")}
    elif case == "forbidden":                            # refused: a delimiter with the forbidden bit set
        put = {slices[1]: SC + b"\x89\xf0"}
    else:
        raise KeyError(case)
    ins = [put[i] for i in sorted(put)]
    return insert(b, put), [(u, _kept_without_flag(u)) for u in ins]


def without_payloads(main_on, units):
    """the flag-on default stream minus exactly the payload bytes of the units put in (each found once, in order)"""
    out, at = bytearray(), 0
    for unit, kept in units:
        k = main_on.index(unit, at)
        out += main_on[at:k] + kept
        at = k + len(unit)
    return bytes(out + main_on[at:])


# ---- pictures with lost slices ------------------------------------------------------------------------------------------------------
class Synth(S.Synth):
    """h264_synth.Synth with non-reference pictures: nal_ref_idc 0, and frame_num does not move behind them (7.4.3)"""
    ref_idc = 3

    def _nal(self, ref_idc, typ, bits):
        S.Synth._nal(self, self.ref_idc if typ in (1, 5) else ref_idc, typ, bits)

    def _header(self, b, s, idr):
        """h264_synth's slice header without dec_ref_pic_marking where nal_ref_idc is 0 (7.3.3)"""
        if self.ref_idc:
            return S.Synth._header(self, b, s, idr)
        assert s["type"] == "P" and not idr and s.get("num_ref") is None and s.get("init_idc") is None
        b.u(8, 0)
        b.ue(s["first_mb"]); b.ue(5); b.ue(s.get("pps", 0))
        b.u(self.l2fn, self.frame_num)
        b.u(1, 0); b.u(1, 0)                                     # no override, no reordering
        b.se(s["qp"] - self.pic_init_qp)
        dis, al, be = s.get("deblock", (0, 0, 0))
        b.ue(dis)
        if dis != 1:
            b.se(al); b.se(be)
        return 1, s["qp"]

    def picture(self, slices, idr=False, ref=True):
        self.ref_idc = 3 if ref else 0
        S.Synth.picture(self, slices, idr)
        if not ref:
            self.frame_num = (self.frame_num - 1) % (1 << self.l2fn)
        self.ref_idc = 3


def _intra(k, t):
    """I16x16 whose 16 luma DC levels are nonzero where the bits of a number made of (k, t) are: the nnz entry names the macroblock"""
    v = (k * 2731 + t * 977 + 1) & 0xffff
    return S.i16(cbp_c=1, dc=[1 if v >> i & 1 else 0 for i in range(16)], cdc=[[1 + (k + t) % 2, 0, 0, 0], [0, 1, 0, 0]])


def _inter(k, t):
    """P_L0_16x16 with 1 .. 5 nonzero levels in every luma block, the count a function of (k, t, block)"""
    return S.p16(cbp_l=15, luma={blk: [1] * (1 + (k + 2 * t + blk) % 5) + [0] * (15 - (k + 2 * t + blk) % 5) for blk in range(16)})


def _picture(s, t, cuts, skips=()):
    """picture t of Synth s: slices begin at `cuts`; I in picture 0, else P with P_Skip at the positions `skips`"""
    n, sl = s.n, []
    for i, a in enumerate(cuts):
        e = cuts[i + 1] if i + 1 < len(cuts) else n
        if t == 0:
            mbs = [_intra(k, t) for k in range(a, e)]
        else:
            mbs = [S.skip(1) if k in skips else _inter(k, t) for k in range(a, e)]
        sl.append(dict(first_mb=a, type="I" if t == 0 else "P", qp=26, mbs=mbs))
    return sl


ROWS, RAGGED = (0, 4, 8), (0, 5, 9)
SKIPS = {1: (2, 9), 2: (4, 6), 3: (0, 9, 11), 4: (3, 8), 5: (1, 10)}


def _synth(w, h, cuts, n_pics, nonref=()):
    s = Synth(w, h)
    for t in range(n_pics):
        s.picture(_picture(s, t, cuts, SKIPS.get(t, ())), idr=t == 0, ref=t not in nonref)
    return s.bytes()


def lost(name):
    # --- synthetic, 4x3 macroblocks, every picture a reference picture: KEEP is two flips back
    if name == "rows":          # uncovered: row 0 with index 0 (picture 2), the last row with the last index (3), the whole middle row (4)
        return drop(_synth(4, 3, ROWS, 6), [(2, 0), (3, 2), (4, 1)])
    if name == "ragged":        # slices 0..4 | 5..8 | 9..11.  Picture 2 loses 5..8: macroblock 9 is coded with an uncovered one to its left
        # (8) and above (5), picture 3 loses 5..8 again with 9 skipped beside 8, picture 4 loses 0..4 with 6 coded under 2 and 8 skipped
        return drop(_synth(4, 3, RAGGED, 6), [(2, 1), (3, 1), (4, 0)])
    if name == "one_left":      # a picture of which one slice is left (the middle one, then the last one)
        return drop(_synth(4, 3, ROWS, 5), [(2, 0), (2, 2), (3, 0), (3, 1)])
    if name == "first":         # the first two pictures damaged: nothing has been in either buffer (no KEEP)
        return drop(_synth(4, 3, ROWS, 4), [(0, 1), (1, 2), (2, 1)])
    if name == "nonref":        # picture 1 is no reference picture: picture 2 has its frame_num and goes to the same buffer - KEEP is picture 1
        return drop(_synth(4, 3, RAGGED, 5, nonref=(1, 3)), [(2, 1), (4, 2)])
    if name == "resize":        # 4x3 with its last picture damaged, then 5x3 with its first two damaged: both buffers start again
        return drop(_synth(4, 3, ROWS, 3), [(2, 1)]) + drop(_synth(5, 3, (0, 5, 10), 3), [(0, 2), (1, 1)])
    # --- committed streams
    if name == "error_i_p":
        return data("Error_I_P.264")
    if name in ("sva_head5", "sva_mid5", "sva_tail5"):  # the cases of tests/golden/make_conceal_streams.py
        return drop(data("SVA_Base_B.264"), [(5, {"sva_head5": 0, "sva_mid5": 1, "sva_tail5": -1}[name])])
    if name == "cabac_slices":  # the CABAC writer: the first six pictures, two slices gone
        return drop(cut(data("test_cif_P_CABAC_slice.264"), 6), [(2, 1), (4, -1)])
    raise KeyError(name)


SYNTHETIC = ["rows", "ragged", "one_left", "first", "nonref", "resize"]
COMMITTED = ["error_i_p", "sva_head5", "sva_mid5", "sva_tail5", "cabac_slices"]
LOST = SYNTHETIC + COMMITTED
# which macroblocks no slice covers, per picture (pictures without a gap are left out): what the synthetic cases are named after
UNCOVERED = {
    "rows": {2: [0, 1, 2, 3], 3: [8, 9, 10, 11], 4: [4, 5, 6, 7]},
    "ragged": {2: [5, 6, 7, 8], 3: [5, 6, 7, 8], 4: [0, 1, 2, 3, 4]},
    "one_left": {2: [0, 1, 2, 3, 8, 9, 10, 11], 3: [0, 1, 2, 3, 4, 5, 6, 7]},
    "first": {0: [4, 5, 6, 7], 1: [8, 9, 10, 11], 2: [4, 5, 6, 7]},
    "nonref": {2: [5, 6, 7, 8], 4: [9, 10, 11]},
    "resize": {2: [4, 5, 6, 7], 3: [10, 11, 12, 13, 14], 4: [5, 6, 7, 8, 9]},
}


# ---- the KEEP rule restated on the host: what lh264_compress_batch_opts computes under the flag, without a device -----------------------
def keep_policy(frames):
    """-> (past, keep): per picture the index of the picture in the OTHER FreqImage buffer (PAST: what a skipped macroblock inherits)
    and of the picture that last occupied the SAME buffer (KEEP: what a cell no slice writes still holds); None: a fresh buffer.  The
    buffers flip when frame_num changes, and both start again when the size changes (decode_slice.cpp:3032-3046)"""
    cur, last_fn, slot, size, past, keep = 0, 0, [None, None], None, [], []
    for i, f in enumerate(frames):
        if f.frame_num != last_fn:
            cur ^= 1
            last_fn = f.frame_num
        if size != (f.mb_w, f.mb_h):
            slot, size = [None, None], (f.mb_w, f.mb_h)
        past.append(slot[1 - cur]); keep.append(slot[cur])
        slot[cur] = i
    return past, keep


def cpu_compress(b):
    """-> (default stream, {tag: bytes}): the host front end with the flag, the oracle's model with the nnz images made by the KEEP rule,
    the oracle's coder"""
    import ctypes as C
    import numpy as np
    import oracle_lib as O
    import losslessh264_amd as lh
    frames, err, main, pcm = lh.parse_file(b, pcm=True, tolerant=True)
    assert err == "", err
    past, keep = keep_policy(frames)
    L = O.lib()
    imgs, out = [], []
    for i, f in enumerate(frames):
        n = f.mb_w * f.mb_h
        img = np.zeros((n, 24), dtype=np.uint8)
        lv = np.ascontiguousarray(f.levels, dtype=np.int16)
        for k in range(n):
            t = int(f.mbs["mb_type"][k])
            src = past[i] if t == 0x100 else keep[i] if t == 0 else -1
            if src == -1:
                L.orc_model_nnz24(lv[k].ctypes.data_as(C.c_void_p), img[k].ctypes.data_as(C.c_void_p))
            elif src is not None:
                img[k] = imgs[src][k]
        imgs.append(img)
        ctx = O.model_frame_symbols(f, img, imgs[past[i]] if past[i] is not None else None)
        hs = f.syn_syms.astype(O.ORC_SYM_DTYPE) if f.syn_syms.dtype != O.ORC_SYM_DTYPE else f.syn_syms
        at = 0
        for k in np.flatnonzero(f.syn_syms["kind"] == 15):
            out.append(hs[at:k]); at = k + 1
            out.append(ctx[int(np.searchsorted(f.syn_off, k, side="right")) - 1])
        out.append(hs[at:])
    syms = np.ascontiguousarray(np.concatenate(out))
    L.orc_coder_new.restype = C.c_void_p
    L.orc_coder_error.restype = C.c_char_p
    c = C.c_void_p(L.orc_coder_new(0))
    assert L.orc_coder_symbols(c, syms.ctypes.data_as(C.c_void_p), C.c_long(len(syms))) == 0, L.orc_coder_error(c)
    L.orc_coder_finish(c)
    tags = {}
    for t in range(72):
        p = C.c_void_p()
        ln = L.orc_coder_tag(c, t, C.byref(p))
        if ln:
            tags[t] = bytes(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(ln,)))
    L.orc_coder_free(c)
    if pcm:
        tags[70] = pcm
    return main, tags
