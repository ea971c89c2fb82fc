"""tests/h264_synth_cabac.py with the macroblock I_NxN under the 8x8 transform (I8x8), in I and in P slices of the CABAC PPS.  Nothing
in h264_synth_cabac.py changes; what is here is written from the same clauses: 7.3.5 / 7.3.5.1 (syntax), 8.3.2.1 (the predicted
Intra8x8PredMode), 9.3.2.5 and 9.3.3.1.1.3 (mb_type: a neighbour that is I_NxN takes its term out of ctxIdxInc), 9.3.3.1.1.10
(transform_size_8x8_flag), 9.3.3.1.2 (prev_intra8x8_pred_mode_flag: ctxIdx 68; rem_intra8x8_pred_mode: three bins of ctxIdx 69, least
significant first), 9.3.3.1.1.8 (intra_chroma_pred_mode), 9.3.3.1.1.4 (coded_block_pattern).

The description names the prediction modes themselves, not the syntax elements: the writer derives the predicted mode of every 8x8 block
from the neighbours, as a reader must, writes prev_intra8x8_pred_mode_flag 1 where the wanted mode is the predicted one and
rem_intra8x8_pred_mode elsewhere, and refuses a mode that reads samples the block does not have.

Counters (Synth.count), beside the parent's:
  i8           dict(avail={(left, top) availability of an I8x8 macroblock}, first={first_mb of slices that start with one},
               prev={prev_intra8x8_pred_mode_flag: count}, pred={the predicted mode where the flag was 1}, rem={rem_intra8x8_pred_mode},
               from_left / from_top={a mode of the neighbouring MACROBLOCK that was the smaller of the two, so set the prediction},
               slice={"I", "P"})
  mb_type_inc  {(kind, ctxIdxInc of the first mb_type bin in an I slice): count}
  t8_inc       (the parent's) now with the intra macroblocks' flags
  i8           also: cbp0={(ctxIdx of the four luma bins, of the chroma bin) of an I8x8 macroblock with coded_block_pattern 0},
               cbp_nb={ctxIdx of a coded_block_pattern bin whose increment read such a macroblock as a neighbour},
               t8_nb={ctxIdxInc of a transform_size_8x8_flag that counted one}, dqp_behind={ctxIdxInc of the mb_qp_delta behind one}
  u8           tests/h264_synth_t8.py tally(), for every picture

An I8x8 macroblock may have coded_block_pattern 0: the flag, the modes, the chroma mode and the pattern's bins, no mb_qp_delta and no
residual; the mb_qp_delta of the macroblock behind it has ctxIdxInc 0 (9.3.3.1.1.5: the previous macroblock in decoding order has
coded_block_pattern 0).  Beside I8x8: I_NxN with the flag 0 (I4x4, every block in DC prediction, which must be the predicted mode), and
P_L0_L0_16x8, P_L0_L0_8x16 and P_8x8 with chosen sub types (one reference, every mvd 0 next to macroblocks whose mvd is 0), with
transform_size_8x8_flag written exactly where 7.3.5 has it.
"""
from h264_synth_cabac import CabacSynth, skip, i16, pcm, p16  # noqa: F401
from h264_synth_t8 import INTER, SUB_PARTS, flag_present, part, tally  # noqa: F401

NEEDS_TOP, NEEDS_LEFT = (0, 3, 7), (1, 8)                       # 8.3.2.2: vertical, diagonal down left, vertical left; horizontal, horizontal up


def i8(modes=(2, 2, 2, 2), cbp_l=15, cbp_c=0, dqp=0, luma8=None, cdc=None, cac=None):
    """I_NxN with transform_size_8x8_flag 1.  modes: Intra8x8PredMode per 8x8 block, of 0, 1, 2, 3, 7, 8 (the modes that read no corner
    sample); luma8: {luma8x8BlkIdx: 64 levels in 8x8 zigzag scan order} - every block of a set cbp_l bit needs a coefficient"""
    return ("i8", dict(modes=tuple(modes), cbp_l=cbp_l, cbp_c=cbp_c, dqp=dqp, luma8=luma8 or {}, cdc=cdc, cac=cac or {}))


def i4(cbp_l=0, cbp_c=0, dqp=0, luma=None, cdc=None, cac=None):
    """I_NxN with transform_size_8x8_flag 0, every block DC.  luma: {luma4x4BlkIdx: 16 levels in scan order}"""
    return ("i4", dict(i4=1, cbp_l=cbp_l, cbp_c=cbp_c, dqp=dqp, luma=luma or {}, cdc=cdc, cac=cac or {}))


MB_TYPE_BINS = {"p16x8": ((14, 0), (15, 1), (17, 1)), "p8x16": ((14, 0), (15, 1), (17, 0)), "p8x8": ((14, 0), (15, 0), (16, 1))}      # Table 9-37, 9.3.3.1.2
SUB_TYPE_BINS = (((21, 1),), ((21, 0), (22, 0)), ((21, 0), (22, 1), (23, 1)), ((21, 0), (22, 1), (23, 0)))      # P_L0_8x8, 8x4, 4x8, 4x4


class CabacSynthI8(CabacSynth):
    def __init__(self, mb_w, mb_h, **kw):
        CabacSynth.__init__(self, mb_w, mb_h, **kw)
        assert self.t8_mode
        self.count.update(i8=dict(avail=set(), first=set(), prev={}, pred=set(), rem=set(), from_left=set(), from_top=set(), slice=set(), cbp0=set(), cbp_nb=set(), t8_nb=set(), dqp_behind=set()), mb_type_inc={})
        self._uncoded_at = None                                   # the address of the last I8x8 macroblock written without a coefficient

    def picture(self, slices, idr=False):
        self.ipm = [None] * self.n                                # per I8x8 macroblock: Intra8x8PredMode of its four blocks
        self.uncoded = set()
        CabacSynth.picture(self, slices, idr)
        tally(self.count, self.mb_w, self.n, [s for s in slices if s.get("pps")], self.pic_init_qp)

    def _slice(self, si, s, idr):
        self._first_mb = s["first_mb"]
        self._uncoded_at = None
        return CabacSynth._slice(self, si, s, idr)

    # ---- mb_type: the parent's, with the I_NxN neighbours' terms ------------------------------------------------------------------
    def _mb_type_intra(self, e, k, is_p, m):
        """m None: I_PCM; "i8": I_NxN; else the I16x16 description"""
        if is_p:
            e.decision(14, 1)
            c0, cac, cc0, cc1, cp0, cp1 = 17, 18, 19, 19, 20, 20
        else:
            inc = sum(1 for N in (self._left(k), self._up(k)) if N is not None and self.info[N]["kind"] not in ("i8", "i4"))
            self._bump(self.count["mb_type_inc"], ("pcm" if m is None else m if m in ("i8", "i4") else "i16", inc))
            c0, cac, cc0, cc1, cp0, cp1 = 3 + inc, 6, 7, 8, 9, 10
        if m in ("i8", "i4"):
            e.decision(c0, 0)
            return
        e.decision(c0, 1)
        if m is None:
            e.terminate(1)
            return
        e.terminate(0)
        e.decision(cac, 1 if m["cbp_l"] else 0)
        e.decision(cc0, 1 if m["cbp_c"] else 0)
        if m["cbp_c"]:
            e.decision(cc1, 1 if m["cbp_c"] == 2 else 0)
        e.decision(cp0, 1); e.decision(cp1, 0)

    def _i16(self, e, k, m, is_p, qp):
        """(the parent sends every macroblock that is neither skipped, I_PCM nor P_L0_16x16 here)"""
        self._k = k
        if "modes" in m:
            return self._i8(e, k, m, is_p, qp)
        if "i4" in m:
            return self._i4(e, k, m, is_p, qp)
        if "subs" in m:
            return self._inter(e, k, m, qp)
        return CabacSynth._i16(self, e, k, m, is_p, qp)

    def _cbf_of(self, k, N, cat, slot, side):
        if N is None and self.info[k]["kind"] in ("i8", "i4"):
            return 1                                             # not available and the current macroblock is intra (9.3.3.1.1.9)
        return CabacSynth._cbf_of(self, k, N, cat, slot, side)

    # ---- 8.3.2.1 ---------------------------------------------------------------------------------------------------------------------
    def _mode_of(self, N, blk):
        """Intra8x8PredMode of block `blk` of the available macroblock N as a neighbour: 2 unless N is I8x8 (no I4x4 is written)"""
        return self.ipm[N][blk] if self.ipm[N] else 2

    def _i8(self, e, k, m, is_p, qp):
        C, I = self.count, self.count["i8"]
        A, B = self._left(k), self._up(k)
        I["avail"].add(("L" if A is not None else "-", "T" if B is not None else "-"))
        I["slice"].add("P" if is_p else "I")
        if k == self._first_mb:
            I["first"].add(k)
        self._mb_type_intra(e, k, is_p, "i8")
        self._t8_flag(e, k, 1)
        modes = []
        for blk, mode in enumerate(m["modes"]):
            bx, by = blk & 1, blk >> 1
            has_left, has_top = bx or A is not None, by or B is not None
            assert mode in (0, 1, 2, 3, 7, 8) and (mode not in NEEDS_TOP or has_top) and (mode not in NEEDS_LEFT or has_left), (k, blk, mode)
            if not (has_left and has_top):
                pred = 2                                         # dcPredModePredictedFlag
            else:
                ma = modes[blk - 1] if bx else self._mode_of(A, blk + 1)
                mb = modes[blk - 2] if by else self._mode_of(B, blk + 2)
                pred = min(ma, mb)
                if not bx and ma < mb:
                    I["from_left"].add(ma)
                if not by and mb < ma:
                    I["from_top"].add(mb)
            self._bump(I["prev"], 1 if mode == pred else 0)
            e.decision(68, 1 if mode == pred else 0)
            if mode == pred:
                I["pred"].add(pred)
            else:
                rem = mode if mode < pred else mode - 1
                I["rem"].add(rem)
                for i in range(3):
                    e.decision(69, rem >> i & 1)
            modes.append(mode)
        self.ipm[k] = modes
        e.decision(64, 0)                                        # intra_chroma_pred_mode 0, as every intra macroblock here has it
        self.info[k] = dict(kind="i8", cbp_l=m["cbp_l"], cbp_c=m["cbp_c"], t8=1, mvd=(0, 0), ref=0)
        self._cbp_cabac(e, k, m)
        if m["cbp_l"] or m["cbp_c"]:
            qp = self._dqp_cabac(e, qp, m["dqp"])
        else:
            self.prev_dqp = 0                                    # no mb_qp_delta: QPY stays QPY,PRED (7.4.5)
            self._qp_seen(qp)
            self.uncoded.add(k)
            self._uncoded_at = k
        levels = []
        for b8 in range(4):
            if m["cbp_l"] >> b8 & 1:
                c64 = m["luma8"].get(b8, [0] * 64)
                self._residual_cabac(e, k, 5, None, c64, 64)
                levels += c64
                for i4 in range(4):
                    self.cbf[k][self._raster(b8 * 4 + i4)] = 1   # inferred for the 4x4 blocks of an 8x8 block (7.4.5.3.3)
        self._chroma_cabac(e, k, m)
        for v in (m["cdc"] or []) if m["cbp_c"] else []:
            levels += v
        for v in m["cac"].values() if m["cbp_c"] == 2 else []:
            levels += v
        self.written[-1][k].update(levels=sorted(v for v in levels if v), modes=tuple(modes))
        return qp

    def _p16(self, e, k, m, num_ref, qp):
        self._k = k
        A, B = self._left(k), self._up(k)
        if m["cbp_l"] and self.t8_mode and any(N in self.uncoded for N in (A, B)):
            self.count["i8"]["t8_nb"].add(sum(1 for N in (A, B) if N is not None and self.info[N]["t8"]))
        return CabacSynth._p16(self, e, k, m, num_ref, qp)

    def _dqp_cabac(self, e, qp, dqp):
        if self._uncoded_at is not None and self._uncoded_at == self._k - 1:
            assert self.prev_dqp == 0
            self.count["i8"]["dqp_behind"].add(0)
        return CabacSynth._dqp_cabac(self, e, qp, dqp)

    def _t8_flag(self, e, k, t8):
        """transform_size_8x8_flag (9.3.3.1.1.10)"""
        A, B = self._left(k), self._up(k)
        inc = sum(1 for N in (A, B) if N is not None and self.info[N]["t8"])
        self._bump(self.count["t8_inc"], inc)
        if any(N in self.uncoded for N in (A, B)):
            self.count["i8"]["t8_nb"].add(inc)
        e.decision(399 + inc, t8)

    def _luma_cabac(self, e, k, m, t8, key8):
        for b8 in range(4):
            if not m["cbp_l"] >> b8 & 1:
                continue
            if t8:
                self._residual_cabac(e, k, 5, None, m[key8].get(b8, [0] * 64), 64)
                for i4 in range(4):
                    self.cbf[k][self._raster(b8 * 4 + i4)] = 1
            else:
                for i4 in range(4):
                    self._residual_cabac(e, k, 2, self._raster(b8 * 4 + i4), m["luma"].get(b8 * 4 + i4, [0] * 16), 16)

    def _i4(self, e, k, m, is_p, qp):
        A, B = self._left(k), self._up(k)
        self._mb_type_intra(e, k, is_p, "i4")
        self._t8_flag(e, k, 0)
        for N, blks in ((A, (1, 3)), (B, (2, 3))):
            assert N is None or all(self._mode_of(N, blk) == 2 for blk in blks), "the predicted mode must be DC"
        for _ in range(16):
            e.decision(68, 1)                                    # prev_intra4x4_pred_mode_flag
        self.ipm[k] = [2] * 4
        e.decision(64, 0)
        self.info[k] = dict(kind="i4", cbp_l=m["cbp_l"], cbp_c=m["cbp_c"], t8=0, mvd=(0, 0), ref=0)
        self._cbp_cabac(e, k, m)
        if m["cbp_l"] or m["cbp_c"]:
            qp = self._dqp_cabac(e, qp, m["dqp"])
        else:
            self.prev_dqp = 0
            self._qp_seen(qp)
        self._luma_cabac(e, k, m, 0, None)
        self._chroma_cabac(e, k, m)
        self.written[-1][k].update(levels=[])
        return qp

    def _inter(self, e, k, m, qp):
        kind = self.written[-1][k]["kind"]
        A, B = self._left(k), self._up(k)
        for c, v in MB_TYPE_BINS[kind]:
            e.decision(c, v)
        if kind == "p8x8":
            for st in m["subs"]:
                for c, v in SUB_TYPE_BINS[st]:
                    e.decision(c, v)
        assert all(N is None or self.info[N]["mvd"] == (0, 0) for N in (A, B)), "mvd 0 is written with ctxIdxInc 0"
        for _ in range(sum(SUB_PARTS[st] for st in m["subs"]) if kind == "p8x8" else 2):
            e.decision(40, 0); e.decision(47, 0)                 # mvd_l0 0, 0
        self.count["num_ref_idx"][1] = max(self.count["num_ref_idx"].get(1, 0), 0)
        t8 = m["t8"]
        assert flag_present(kind, m) or not t8
        self.info[k] = dict(kind=kind, cbp_l=m["cbp_l"], cbp_c=m["cbp_c"], t8=t8, mvd=(0, 0), ref=0)
        self._cbp_cabac(e, k, m)
        if flag_present(kind, m):
            self._t8_flag(e, k, t8)
        if m["cbp_l"] or m["cbp_c"]:
            qp = self._dqp_cabac(e, qp, m["dqp"])
        else:
            self.prev_dqp = 0
            self._qp_seen(qp)
        self._luma_cabac(e, k, m, t8, "luma8")
        self._chroma_cabac(e, k, m)
        self.written[-1][k].update(levels=[])
        return qp

    def _cbp_cabac(self, e, k, m):
        """coded_block_pattern (9.3.2.6, 9.3.3.1.1.4): four luma bins by their own neighbours, then the chroma TU"""
        A, B = self._left(k), self._up(k)
        I = self.count["i8"]
        own, luma_ctx = self.info[k]["kind"] == "i8" and not (m["cbp_l"] or m["cbp_c"]), []
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
            luma_ctx.append(73 + cond[0] + 2 * cond[1])
            if (not b8 & 1 and A in self.uncoded) or (not b8 & 2 and B in self.uncoded):
                I["cbp_nb"].add(73 + cond[0] + 2 * cond[1])

        def chroma(level):
            return [1 if N is not None and (self.info[N]["kind"] == "pcm" or (self.info[N]["kind"] != "skip" and self.info[N]["cbp_c"] >= level)) else 0 for N in (A, B)]
        nz = chroma(1)
        e.decision(77 + nz[0] + 2 * nz[1], 1 if m["cbp_c"] else 0)
        if own:
            I["cbp0"].add((tuple(luma_ctx), 77 + nz[0] + 2 * nz[1]))
        if any(N in self.uncoded for N in (A, B)):
            I["cbp_nb"].add(77 + nz[0] + 2 * nz[1])
        if m["cbp_c"]:
            two = chroma(2)
            e.decision(77 + 4 + two[0] + 2 * two[1], 1 if m["cbp_c"] == 2 else 0)
