"""A CABAC writer for tests, on tests/h264_synth.py: slices of a second PPS (pps_id 1: entropy_coding_mode_flag 1, transform_8x8_mode
1) beside the CAVLC slices of PPS 0, so that any value can be placed where a CABAC reader or writer changes its path: the UEG0 joint at
14 and the UEG3 joint at 9, the Exp-Golomb suffix with large values, ref_idx above 0, the mvd and mb_qp_delta context increments,
SliceQPY 0 and 51 in the context initialisation, the last position of every significance map, chains of outstanding bits, the engine
restart around I_PCM, cabac_alignment_one_bit at every header phase.

Written from ITU-T H.264 clauses 7.3 (syntax), 9.3.1 (initialisation), 9.3.2 (binarisations), 9.3.3.1 (ctxIdx assignment) and 9.3.4
(the encoder: EncodeDecision, EncodeBypass, EncodeTerminate, EncodeFlush, PutBit), not from the product's parser or restorers.  Only the
CONTENTS of the numeric tables are read from the product's sources, because the corpus pins them: the (m, n) pairs, rangeTabLPS and
the state transitions (csrc/host/h264_cabac_tables.h) and the ctxIdxInc of 8x8 blocks, Table 9-43 (the two arrays in
csrc/host/h264_parser.cpp).

The subset: I and P slices with cabac_init_idc 0..2; mb_skip_flag, end_of_slice_flag; P_L0_16x16 (ref_idx, mvd, coded_block_pattern,
transform_size_8x8_flag, mb_qp_delta, residual blocks of ctxBlockCat 1..5 - 1 through I16x16); I16x16 with DC prediction (ctxBlockCat 0
and 1, intra_chroma_pred_mode 0); I_PCM.  Neighbour availability is slice membership, as in Synth._nc.

A slice is CABAC when its description has pps=1: dict(first_mb, type, qp, mbs, pps=1, init_idc=0..2 (P), num_ref, deblock).  In a
CABAC slice every skipped macroblock is its own ("skip", 1) ... ("skip", n) stands for n flags.

Counters (Synth.count), beside the parent's:
  abs_level            {(ctxBlockCat, coeff_abs_level_minus1): count}
  gt1_eq1              {ctxBlockCat: [largest numDecodAbsLevelGt1, largest numDecodAbsLevelEq1] seen when a level was coded}
  last_pos             {(ctxBlockCat, index of the last significant coefficient)}
  mvd                  dict(min, max, inc=[{ctxIdxInc: count} for x, for y], sums=[set of absMvdComp(A) + absMvdComp(B) for x, for y])
  ref_idx              dict(top={num_ref_idx_active: highest ref_idx}, inc={ctxIdxInc: count})
  dqp                  dict(min, max, inc={ctxIdxInc: count}, after={(what came before in the slice: "first", "skip", "pcm", "cbp0",
                       "zero" or "nonzero" for a coded delta, ctxIdxInc)})
  slice_qp             {("I" or cabac_init_idc, SliceQPY)}
  cbf_inc              {(ctxBlockCat, ctxIdxInc): count}; cbf_pcm: {(ctxBlockCat, "A" or "B")} where an I_PCM neighbour set the term;
                       cbf_zero: {ctxBlockCat: blocks coded with coded_block_flag 0}
  skip_inc, t8_inc     {ctxIdxInc: count}
  outstanding_max      the longest chain of outstanding bits
  hdr_phase            {slice header bits mod 8}: 8 - that many cabac_alignment_one_bits (none at 0)
  stop_phase           {bit position of the rbsp stop bit in its byte}
  pcm_phase            (the parent's) bit phase at which pcm_alignment_zero_bits started, behind the flush
  epb, epb_arith       emulation prevention bytes; those inside arithmetic-coded data (not the header, not I_PCM samples)
  slice_bytes_min      the shortest slice_data written, in bytes
"""
import os
import re

import h264_synth as H
from h264_synth import skip, i16, pcm  # noqa: F401  (descriptions are the parent's)


def p16(t8=0, luma8=None, **kw):
    """the parent's P_L0_16x16 with transform_size_8x8_flag; luma8: {luma8x8BlkIdx: 64 levels in (frame) zigzag scan order}"""
    kind, m = H.p16(**kw)
    m["t8"], m["luma8"] = t8, luma8 or {}
    return kind, m


def _load_tables():
    txt = open(os.path.join(H._CSRC, "h264_cabac_tables.h")).read()
    num = lambda s: [int(x) for x in re.findall(r"-?\d+", s)]     # noqa: E731

    def body(src, name):
        s = src[src.index(name):]
        return s[s.index("=") + 1:s.index("};")]
    init = num(body(txt, "kCabacInit[460][4][2]"))
    assert len(init) == 460 * 8
    T = {"init": [[(init[i * 8 + 2 * c], init[i * 8 + 2 * c + 1]) for c in range(4)] for i in range(460)]}
    lps = num(body(txt, "kCabacRangeLps[64][4]"))
    T["range_lps"] = [lps[i * 4:i * 4 + 4] for i in range(64)]
    T["next_lps"], T["next_mps"] = num(body(txt, "kCabacNextLps[64]")), num(body(txt, "kCabacNextMps[64]"))
    par = open(os.path.join(H._CSRC, "h264_parser.cpp")).read()
    T["sig8"], T["last8"] = num(body(par, "kSig8x8[63]")), num(body(par, "kLast8x8[63]"))
    assert [len(T[k]) for k in ("range_lps", "next_lps", "next_mps", "sig8", "last8")] == [64, 64, 64, 63, 63]
    return T


TABLES = _load_tables()
CAT_CBF, CAT_MAP, CAT_ABS = (0, 4, 8, 12, 16), (0, 15, 29, 44, 47, 0), (0, 10, 20, 30, 39, 0)
SIG_BASE, LAST_BASE, ABS_BASE = (105,) * 5 + (402,), (166,) * 5 + (417,), (227,) * 5 + (426,)


class Enc:
    """the arithmetic encoder of 9.3.4.2 .. 9.3.4.5 over a Bits"""

    def __init__(self, bits, count, qp, column):
        self.b, self.C = bits.b, count
        self.ctx = []
        for m, n in (row[column] for row in TABLES["init"]):     # 9.3.1.1
            pre = min(126, max(1, ((m * min(51, max(0, qp))) >> 4) + n))
            self.ctx.append([63 - pre, 0] if pre <= 63 else [pre - 64, 1])
        self.start()

    def start(self):
        self.low, self.range, self.first, self.out = 0, 510, True, 0

    def _put(self, bit):
        if self.first:
            self.first = False
        else:
            self.b.append(bit)
        while self.out:
            self.b.append(1 - bit); self.out -= 1

    def _wait(self):
        self.out += 1
        self.C["outstanding_max"] = max(self.C["outstanding_max"], self.out)

    def _renorm(self):
        while self.range < 256:
            if self.low < 256:
                self._put(0)
            elif self.low >= 512:
                self.low -= 512; self._put(1)
            else:
                self.low -= 256; self._wait()
            self.range <<= 1; self.low <<= 1

    def decision(self, idx, bin_):
        st = self.ctx[idx]
        lps = TABLES["range_lps"][st[0]][(self.range >> 6) & 3]
        self.range -= lps
        if bin_ != st[1]:
            self.low += self.range; self.range = lps
            if st[0] == 0:
                st[1] = 1 - st[1]
            st[0] = TABLES["next_lps"][st[0]]
        else:
            st[0] = TABLES["next_mps"][st[0]]
        self._renorm()

    def bypass(self, bin_):
        self.low <<= 1
        if bin_:
            self.low += self.range
        if self.low >= 1024:
            self._put(1); self.low -= 1024
        elif self.low < 512:
            self._put(0)
        else:
            self.low -= 512; self._wait()

    def terminate(self, bin_):
        self.range -= 2
        if bin_:
            self.low += self.range
            self.range = 2                                       # EncodeFlush
            self._renorm()
            self._put((self.low >> 9) & 1)
            v = ((self.low >> 7) & 3) | 1
            self.b.append(v >> 1); self.b.append(v & 1)
        else:
            self._renorm()

    def unary(self, v, ctxs):
        """U binarisation: v ones and a zero; bin i with ctxs[min(i, last)]"""
        for i in range(v + 1):
            self.decision(ctxs[min(i, len(ctxs) - 1)], 1 if i < v else 0)

    def exp_golomb(self, v, k):
        """the UEGk suffix (9.3.2.3), in bypass"""
        while v >= (1 << k):
            self.bypass(1); v -= 1 << k; k += 1
        self.bypass(0)
        while k:
            k -= 1
            self.bypass((v >> k) & 1)


def escape_positions(rbsp):
    """the rbsp byte indices in front of which 7.4.1 inserts an emulation prevention byte"""
    at, zeros = [], 0
    for i, c in enumerate(rbsp):
        if zeros >= 2 and c <= 3:
            at.append(i); zeros = 0
        zeros = zeros + 1 if c == 0 else 0
    return at


class CabacSynth(H.Synth):
    def __init__(self, mb_w, mb_h, profile=100, t8=1, **kw):
        assert profile in (77, 100) and (profile == 100 or not t8)
        H.Synth.__init__(self, mb_w, mb_h, profile=profile, **kw)
        self._pps(1, 1, t8)
        self.t8_mode = t8
        self.count.update(abs_level={}, gt1_eq1={}, last_pos=set(), mvd=dict(min=0, max=0, inc=[{}, {}], sums=[set(), set()]),
                          ref_idx=dict(top={}, inc={}), dqp=dict(min=0, max=0, inc={}, after=set()), slice_qp=set(), cbf_inc={}, cbf_pcm=set(), cbf_zero={}, skip_inc={}, t8_inc={},
                          outstanding_max=0, hdr_phase=set(), stop_phase=set(), epb_arith=0, slice_bytes_min=1 << 30)
        self.written = []                                        # per picture, per macroblock: what a reader must find

    def picture(self, slices, idr=False):
        self.info = [None] * self.n                              # per macroblock of a CABAC slice: what its neighbours' increments read
        self.cbf = [[0] * 27 for _ in range(self.n)]             # 16 luma 4x4 (raster), Intra16x16 DC, Cb DC, Cr DC, 4 Cb AC, 4 Cr AC
        self.written.append([None] * self.n)
        H.Synth.picture(self, slices, idr)

    # ---- neighbours --------------------------------------------------------------------------------------------------------------
    def _left(self, k):
        return k - 1 if k % self.mb_w and self.slice_of[k - 1] == self.slice_of[k] else None

    def _up(self, k):
        return k - self.mb_w if k >= self.mb_w and self.slice_of[k - self.mb_w] == self.slice_of[k] else None

    @staticmethod
    def _bump(d, key):
        d[key] = d.get(key, 0) + 1

    # ---- a CABAC slice -----------------------------------------------------------------------------------------------------------
    def _slice(self, si, s, idr):
        if not s.get("pps"):
            return H.Synth._slice(self, si, s, idr)
        C = self.count
        is_p = s["type"] == "P"
        if is_p:
            s = dict(s, init_idc=s.get("init_idc", 0))
        b = H.Bits()
        num_ref, qp = self._header(b, s, idr)
        C["hdr_phase"].add(len(b) % 8)
        C["slice_qp"].add((s["init_idc"] if is_p else "I", qp))
        while len(b) % 8:
            b.u(1, 1)                                            # cabac_alignment_one_bit
        data_at = len(b) // 8
        e = Enc(b, C, qp, 1 + s["init_idc"] if is_p else 0)
        mbs = []
        for kind, m in s["mbs"]:
            mbs += [("skip", 1)] * m if kind == "skip" else [(kind, m)]
        k = s["first_mb"]
        self.prev_dqp, self.prev_kind = 0, "first"
        samples = []                                             # rbsp byte ranges of I_PCM samples
        for j, (kind, m) in enumerate(mbs):
            self.slice_of[k] = si
            A, B = self._left(k), self._up(k)
            rec = self.written[-1][k] = dict(kind=kind, qp=qp)
            if is_p:
                inc = sum(1 for N in (A, B) if N is not None and self.info[N]["kind"] != "skip")
                e.decision(11 + inc, 1 if kind == "skip" else 0)
                self._bump(C["skip_inc"], inc)
            if kind == "skip":
                self.info[k] = dict(kind="skip", cbp_l=0, cbp_c=0, t8=0, mvd=(0, 0), ref=0)
                self.prev_dqp = 0
                self._qp_seen(qp)
            else:
                if kind == "pcm":
                    self._mb_type_intra(e, k, is_p, None)
                    C["pcm_phase"].add(len(b) % 8)
                    while len(b) % 8:
                        b.u(1, 0)
                    samples.append((len(b) // 8, len(b) // 8 + 384))
                    for c in m:
                        b.u(8, c)
                    e.start()                                    # 9.3.1.2: the engine alone, the contexts stay
                    self.info[k] = dict(kind="pcm", cbp_l=15, cbp_c=2, t8=0, mvd=(0, 0), ref=0)
                    self.cbf[k] = [1] * 27
                    self.prev_dqp = 0                            # no mb_qp_delta: QPY stays QPY,PRED for the next macroblock (7.4.5);
                    rec.update(qp=0, pcm=bytes(m))               # the macroblock's own qp, which the deblocking filter reads, is 0 (8.7.2)
                elif kind == "p16":
                    qp = self._p16(e, k, m, num_ref, qp)
                else:
                    qp = self._i16(e, k, m, is_p, qp)
                if kind != "pcm":
                    rec["qp"] = qp
            self.prev_kind = kind if kind in ("skip", "pcm") else "cbp0" if kind == "p16" and not (m["cbp_l"] or m["cbp_c"]) else \
                "nonzero" if self.prev_dqp else "zero"
            k += 1
            e.terminate(1 if j == len(mbs) - 1 else 0)           # end_of_slice_flag
        C["stop_phase"].add((len(b) - 1) % 8)
        while len(b) % 8:
            b.u(1, 0)
        self.last_align = (0, 0)
        b.b = b.b[8:]
        rbsp = b.bytes()
        data_at -= 1
        C["slice_bytes_min"] = min(C["slice_bytes_min"], len(rbsp) - data_at)
        C["epb_arith"] += sum(1 for i in escape_positions(rbsp) if i >= data_at and not any(a - 1 <= i <= z - 1 for a, z in samples))
        self._nal(3, 5 if idr else 1, b)

    # ---- mb_type (9.3.2.5, Table 9-36; ctxIdx: 9.3.3.1.1.3, 9.3.3.1.2) -----------------------------------------------------------
    def _mb_type_intra(self, e, k, is_p, m):
        """m None: I_PCM; else the I16x16 description"""
        if is_p:
            e.decision(14, 1)                                    # the prefix: not a P type
            c0, cac, cc0, cc1, cp0, cp1 = 17, 18, 19, 19, 20, 20
        else:
            inc = sum(1 for N in (self._left(k), self._up(k)) if N is not None)      # no neighbour here is I_NxN
            c0, cac, cc0, cc1, cp0, cp1 = 3 + inc, 6, 7, 8, 9, 10
        e.decision(c0, 1)
        if m is None:
            e.terminate(1)
            return
        e.terminate(0)
        e.decision(cac, 1 if m["cbp_l"] else 0)
        e.decision(cc0, 1 if m["cbp_c"] else 0)
        if m["cbp_c"]:
            e.decision(cc1, 1 if m["cbp_c"] == 2 else 0)
        e.decision(cp0, 1); e.decision(cp1, 0)                   # Intra16x16PredMode 2, DC

    # ---- macroblocks -------------------------------------------------------------------------------------------------------------
    def _dqp_cabac(self, e, qp, dqp):
        C = self.count["dqp"]
        assert -26 <= dqp <= 25
        inc = 1 if self.prev_dqp else 0
        self._bump(C["inc"], inc)
        C["after"].add((self.prev_kind, inc))
        e.unary(2 * dqp - 1 if dqp > 0 else -2 * dqp, [60 + inc, 62, 63])
        C["min"], C["max"] = min(C["min"], dqp), max(C["max"], dqp)
        self.count["dqp_min"], self.count["dqp_max"] = min(self.count["dqp_min"], dqp), max(self.count["dqp_max"], dqp)
        self.prev_dqp = dqp
        qp = (qp + dqp + 52) % 52
        self._qp_seen(qp)
        return qp

    def _i16(self, e, k, m, is_p, qp):
        self._mb_type_intra(e, k, is_p, m)
        e.decision(64, 0)                                        # intra_chroma_pred_mode 0; every neighbour has 0 too, or is not intra
        self.info[k] = dict(kind="i16", cbp_l=m["cbp_l"], cbp_c=m["cbp_c"], t8=0, mvd=(0, 0), ref=0)
        qp = self._dqp_cabac(e, qp, m["dqp"])
        self.written[-1][k].update(levels=self._levels_of(m, True))
        self._residual_cabac(e, k, 0, 16, m["dc"], 16)
        if m["cbp_l"]:
            for blk in range(16):
                self._residual_cabac(e, k, 1, self._raster(blk), m["ac"].get(blk, [0] * 15), 15)
        self._chroma_cabac(e, k, m)
        return qp

    def _p16(self, e, k, m, num_ref, qp):
        C = self.count
        A, B = self._left(k), self._up(k)
        for ctx in (14, 15, 16):
            e.decision(ctx, 0)                                   # P_L0_16x16
        if num_ref > 1:
            assert 0 <= m["ref"] < num_ref
            inc = (1 if A is not None and self.info[A]["ref"] > 0 else 0) + (2 if B is not None and self.info[B]["ref"] > 0 else 0)
            self._bump(C["ref_idx"]["inc"], inc)
            e.unary(m["ref"], [54 + inc, 58, 59])
        C["ref_idx"]["top"][num_ref] = max(C["ref_idx"]["top"].get(num_ref, 0), m["ref"])
        C["num_ref_idx"][num_ref] = max(C["num_ref_idx"].get(num_ref, 0), m["ref"])
        for comp, v in enumerate(m["mvd"]):
            total = sum(self.info[N]["mvd"][comp] for N in (A, B) if N is not None)
            inc = 0 if total < 3 else 1 if total <= 32 else 2
            self._bump(C["mvd"]["inc"][comp], inc)
            C["mvd"]["sums"][comp].add(total)
            base = 40 + 7 * comp
            a = abs(v)
            for i in range(min(a, 9) + (1 if a < 9 else 0)):     # the TU prefix, cMax 9
                e.decision(base + (inc, 3, 4, 5, 6)[min(i, 4)], 1 if i < a else 0)
            if a >= 9:
                e.exp_golomb(a - 9, 3)
            if a:
                e.bypass(1 if v < 0 else 0)
            C["mvd"]["min"], C["mvd"]["max"] = min(C["mvd"]["min"], v), max(C["mvd"]["max"], v)
            C["mvd_min"], C["mvd_max"] = min(C["mvd_min"], v), max(C["mvd_max"], v)
        t8 = m.get("t8", 0)
        assert not t8 or (self.t8_mode and m["cbp_l"])
        self.info[k] = dict(kind="p16", cbp_l=m["cbp_l"], cbp_c=m["cbp_c"], t8=t8, mvd=(abs(m["mvd"][0]), abs(m["mvd"][1])), ref=m["ref"])
        self.written[-1][k].update(mvd=tuple(m["mvd"]), ref=m["ref"], levels=self._levels_of(m, False))
        # coded_block_pattern: 4 luma bins by their own neighbours, then the chroma TU
        for b8 in range(4):
            cond = []
            for N, nb8 in ((k if b8 & 1 else A, b8 ^ 1), (k if b8 & 2 else B, b8 ^ 2)):
                if N is None or self.info[N]["kind"] == "pcm":
                    cond.append(0)
                elif self.info[N]["kind"] == "skip":
                    cond.append(1)
                else:
                    cond.append(0 if self.info[N]["cbp_l"] >> nb8 & 1 else 1)
            e.decision(73 + cond[0] + 2 * cond[1], m["cbp_l"] >> b8 & 1)
        nz = [1 if N is not None and (self.info[N]["kind"] == "pcm" or (self.info[N]["kind"] != "skip" and self.info[N]["cbp_c"])) else 0 for N in (A, B)]
        e.decision(77 + nz[0] + 2 * nz[1], 1 if m["cbp_c"] else 0)
        if m["cbp_c"]:
            two = [1 if N is not None and (self.info[N]["kind"] == "pcm" or (self.info[N]["kind"] != "skip" and self.info[N]["cbp_c"] == 2)) else 0 for N in (A, B)]
            e.decision(77 + 4 + two[0] + 2 * two[1], 1 if m["cbp_c"] == 2 else 0)
        if m["cbp_l"] and self.t8_mode:
            inc = sum(1 for N in (A, B) if N is not None and self.info[N]["t8"])
            self._bump(C["t8_inc"], inc)
            e.decision(399 + inc, t8)
        if m["cbp_l"] or m["cbp_c"]:
            qp = self._dqp_cabac(e, qp, m["dqp"])
        else:
            self.prev_dqp = 0
            self._qp_seen(qp)
        for i8 in range(4):
            if not m["cbp_l"] >> i8 & 1:
                continue
            if t8:
                self._residual_cabac(e, k, 5, None, m["luma8"].get(i8, [0] * 64), 64)
                for i4 in range(4):
                    self.cbf[k][self._raster(i8 * 4 + i4)] = 1   # inferred for the 4x4 blocks of an 8x8 block (7.4.5.3.3)
            else:
                for i4 in range(4):
                    self._residual_cabac(e, k, 2, self._raster(i8 * 4 + i4), m["luma"].get(i8 * 4 + i4, [0] * 16), 16)
        self._chroma_cabac(e, k, m)
        return qp

    def _chroma_cabac(self, e, k, m):
        if m["cbp_c"]:
            for pl in range(2):
                self._residual_cabac(e, k, 3, 17 + pl, (m["cdc"] or [[0] * 4] * 2)[pl], 4)
        if m["cbp_c"] == 2:
            for pl in range(2):
                for blk in range(4):
                    self._residual_cabac(e, k, 4, 19 + 4 * pl + blk, m["cac"].get((pl, blk), [0] * 15), 15)

    @staticmethod
    def _raster(blk):
        return ((blk >> 1 & 1) + 2 * (blk >> 3)) * 4 + (blk & 1) + 2 * (blk >> 2 & 1)

    @staticmethod
    def _levels_of(m, intra):
        """every nonzero level of the macroblock that its syntax codes, sorted"""
        out = []
        if intra:
            out += m["dc"]
            if m["cbp_l"]:
                for v in m["ac"].values():
                    out += v
        else:
            for i8 in range(4):
                if m["cbp_l"] >> i8 & 1:
                    if m.get("t8"):
                        out += m["luma8"].get(i8, [])
                    else:
                        for i4 in range(4):
                            out += m["luma"].get(i8 * 4 + i4, [])
        if m["cbp_c"]:
            for v in m["cdc"] or []:
                out += v
        if m["cbp_c"] == 2:
            for v in m["cac"].values():
                out += v
        return sorted(v for v in out if v)

    # ---- residual_block_cabac (7.3.5.3.3; ctxIdx: 9.3.3.1.1.9, 9.3.3.1.3) --------------------------------------------------------
    def _cbf_of(self, k, N, cat, slot, side):
        """coded_block_flag of transBlockN for the block at `slot` of macroblock N (None: not available)"""
        if N is None:
            return 1 if self.info[k]["kind"] == "i16" else 0
        inf = self.info[N]
        if inf["kind"] == "pcm":
            self.count["cbf_pcm"].add((cat, side))
            return 1
        if inf["kind"] == "skip":
            return 0
        if cat == 0:
            return self.cbf[N][16] if inf["kind"] == "i16" else 0
        if cat in (1, 2):
            y, x = divmod(slot, 4)
            if not inf["cbp_l"] >> ((y >> 1) * 2 + (x >> 1)) & 1:
                return 0
            return 1 if inf["t8"] else self.cbf[N][slot]
        if cat == 3:
            return self.cbf[N][slot] if inf["cbp_c"] else 0
        return self.cbf[N][slot] if inf["cbp_c"] == 2 else 0

    def _cbf_inc(self, k, cat, slot):
        A, B = self._left(k), self._up(k)
        if cat in (0, 3):
            na, nb = (A, slot), (B, slot)
        elif cat in (1, 2):
            y, x = divmod(slot, 4)
            na = (k, slot - 1) if x else (A, slot + 3)
            nb = (k, slot - 4) if y else (B, slot + 12)
        else:
            base = 19 if slot < 23 else 23
            y, x = divmod(slot - base, 2)
            na = (k, slot - 1) if x else (A, slot + 1)
            nb = (k, slot - 2) if y else (B, slot + 2)
        return self._cbf_of(k, na[0], cat, na[1], "A") + 2 * self._cbf_of(k, nb[0], cat, nb[1], "B")

    def _residual_cabac(self, e, k, cat, slot, coef, maxn):
        C = self.count
        assert len(coef) == maxn
        pos = [i for i, v in enumerate(coef) if v]
        if cat != 5:                                             # 4:2:0: no coded_block_flag for an 8x8 block
            inc = self._cbf_inc(k, cat, slot)
            self._bump(C["cbf_inc"], (cat, inc))
            e.decision(85 + CAT_CBF[cat] + inc, 1 if pos else 0)
            self.cbf[k][slot] = 1 if pos else 0
            if not pos:
                self._bump(C["cbf_zero"], cat)
                return
        assert pos, "an 8x8 block of a set coded_block_pattern bit needs a coefficient (its coded_block_flag is inferred 1)"
        C["last_pos"].add((cat, pos[-1]))
        for i in range(maxn - 1):
            si = TABLES["sig8"][i] if cat == 5 else min(i, 2) if cat == 3 else i
            li = TABLES["last8"][i] if cat == 5 else min(i, 2) if cat == 3 else i
            e.decision(SIG_BASE[cat] + CAT_MAP[cat] + si, 1 if coef[i] else 0)
            if coef[i]:
                e.decision(LAST_BASE[cat] + CAT_MAP[cat] + li, 1 if i == pos[-1] else 0)
                if i == pos[-1]:
                    break
        gt1 = eq1 = 0
        g = C["gt1_eq1"].setdefault(cat, [0, 0])
        base = ABS_BASE[cat] + CAT_ABS[cat]
        for i in reversed(pos):
            v = abs(coef[i]) - 1
            self._bump(C["abs_level"], (cat, v))
            g[0], g[1] = max(g[0], gt1), max(g[1], eq1)
            C["level_min"], C["level_max"] = min(C["level_min"], coef[i]), max(C["level_max"], coef[i])
            first = 0 if gt1 else min(4, 1 + eq1)
            rest = 5 + min(4 - (1 if cat == 3 else 0), gt1)
            for j in range(min(v, 14) + (1 if v < 14 else 0)):   # the TU prefix, cMax 14
                e.decision(base + (first if j == 0 else rest), 1 if j < v else 0)
            if v >= 14:
                e.exp_golomb(v - 14, 0)
            e.bypass(1 if coef[i] < 0 else 0)
            if v:
                gt1 += 1
            else:
                eq1 += 1
