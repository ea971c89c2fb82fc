"""tests/h264_synth.py with the 8x8 transform under CAVLC: a High-profile PPS with transform_8x8_mode_flag, and the macroblock
I_NxN with transform_size_8x8_flag = 1 (7.3.5, 7.3.5.1, 7.3.5.3.2) in I and in P slices.  An 8x8 block's 64 coefficients travel as four
interleaved 4x4 blocks of 16 (coefficient 4 * i + j of the 8x8 scan is coefficient i of block j), each with the nC of its place.
Nothing in h264_synth.py changes; what is here is written from the same clauses.

Beside I8x8: I_NxN with the flag 0 (I4x4, every prev_intra4x4_pred_mode_flag 1), and the inter types whose transform_size_8x8_flag is
present or absent by 7.3.5: P_L0_16x16 with the flag, P_L0_L0_16x8, P_L0_L0_8x16 and P_8x8 with chosen sub types (their mvd all 0, one
reference).  The flag is written exactly where the syntax has it: CodedBlockPatternLuma > 0 and no sub-macroblock partition below 8x8.

tally() counts, from what a picture was written of, where a macroblock without any coefficient sits under the 8x8 transform; both
writers (this one and tests/h264_synth_cabac_i8.py) call it for every picture.  Synth.count["u8"]:
  n            I8x8 macroblocks with coded_block_pattern 0 ("i8u" below)
  first        {first_mb of slices that start with one};  avail: {(left, top) availability in its slice}
  beside       {label of a macroblock left of, right of, above or below one, in the picture}: "i8" (coded), "i8u", "i4", "i16", "pcm",
               "p16" (flag absent or 0), "p16t8" (flag 1), "p16x8", "p8x16", "p8x8", "skip"
  pairs        how often two stand side by side in one slice
  last_slice, last_pic   how many end their slice, their picture
  carried      {(the QP carried into one, SliceQPY, pic_init_qp)};  behind: {(label, mb_qp_delta or None) of the macroblock after one}
  deblock      {disable_deblocking_filter_idc of its slice};  slice: {"I", "P"}
  inter        {(kind, cbp_l != 0, cbp_c, sub types or None, the flag as written: None, 0 or 1)} of the inter macroblocks
  between      those of `inter` that stand between two macroblocks of their slice and row whose flag is 1
  i8u_between  {(label left, label right)} of an i8u in a P slice between two inter macroblocks without the flag
  log          per picture, per macroblock: (label, transform_size_8x8_flag, coded_block_pattern or None, QPY behind it)"""
import h264_synth as S
from h264_synth import Bits, TABLES, i16, pcm, skip  # noqa: F401

INTER = ("p16", "p16x8", "p8x16", "p8x8")
SUB_PARTS = (1, 2, 2, 4)                                         # mvd pairs of sub_mb_type P_L0_8x8, 8x4, 4x8, 4x4


def i8(modes=(None, None, None, None), cbp_l=0, cbp_c=0, dqp=0, luma=None, cdc=None, cac=None, chroma_mode=0):
    """I_NxN with the 8x8 transform.  modes: per 8x8 block None (prev_intra8x8_pred_mode_flag = 1: the predicted mode) or
    rem_intra8x8_pred_mode 0..7; luma: {luma8x8BlkIdx: 64 levels in 8x8 scan order} for blocks whose cbp_l bit is set"""
    return ("i8", dict(modes=modes, cbp_l=cbp_l, cbp_c=cbp_c, dqp=dqp, luma=luma or {}, cdc=cdc, cac=cac or {}, chroma_mode=chroma_mode))


def i4(cbp_l=0, cbp_c=0, dqp=0, luma=None, cdc=None, cac=None):
    """I_NxN with transform_size_8x8_flag 0, every block in its predicted mode.  luma: {luma4x4BlkIdx: 16 levels}"""
    return ("i4", dict(cbp_l=cbp_l, cbp_c=cbp_c, dqp=dqp, luma=luma or {}, cdc=cdc, cac=cac or {}))


def p16(t8=0, luma8=None, **kw):
    """the parent's P_L0_16x16 with transform_size_8x8_flag; luma8: {luma8x8BlkIdx: 64 levels in 8x8 scan order}"""
    kind, m = S.p16(**kw)
    m["t8"], m["luma8"] = t8, luma8 or {}
    return kind, m


def part(kind, subs=None, t8=0, cbp_l=0, cbp_c=0, dqp=0, luma=None, luma8=None, cdc=None, cac=None):
    """P_L0_L0_16x8 ("p16x8"), P_L0_L0_8x16 ("p8x16") or P_8x8 ("p8x8", subs: four sub_mb_type 0..3), every mvd 0"""
    assert kind in INTER[1:] and (kind == "p8x8") == (subs is not None)
    return (kind, dict(subs=tuple(subs) if subs else None, t8=t8, cbp_l=cbp_l, cbp_c=cbp_c, dqp=dqp, luma=luma or {}, luma8=luma8 or {}, cdc=cdc, cac=cac or {},
                       mvd=(0, 0), ref=0))


def flag_present(kind, m):
    """7.3.5 under transform_8x8_mode_flag 1, for an inter macroblock: is transform_size_8x8_flag in the stream"""
    return bool(m["cbp_l"]) and not (kind == "p8x8" and any(m["subs"]))


def label(kind, m):
    if kind == "i8":
        return "i8" if m["cbp_l"] or m["cbp_c"] else "i8u"
    if kind == "p16":
        return "p16t8" if m.get("t8") else "p16"
    return kind


def tally(C, mb_w, n, slices, pic_init_qp):
    """see the module's text"""
    U = C.setdefault("u8", dict(n=0, first=set(), avail=set(), beside=set(), pairs=0, last_slice=0, last_pic=0, carried=set(), behind=set(), deblock=set(),
                                slice=set(), inter=set(), between=set(), i8u_between=set(), log=[]))
    lab, t8, sl, before, after, desc = [None] * n, [0] * n, [-1] * n, [None] * n, [None] * n, [None] * n
    ends = set()
    for si, s in enumerate(slices):
        qp, k = s["qp"], s["first_mb"]
        for kind, m in s["mbs"]:
            for _ in range(m if kind == "skip" else 1):
                lab[k], sl[k], before[k], desc[k] = label(kind, m), si, qp, (kind, m)
                if kind == "i8":
                    t8[k] = 1
                elif kind in INTER:
                    t8[k] = m.get("t8", 0)
                coded = kind == "i16" or (kind not in ("skip", "pcm") and (m["cbp_l"] or m["cbp_c"]))
                if coded:
                    qp = (qp + m["dqp"] + 52) % 52
                after[k] = qp
                k += 1
        ends.add(k - 1)
    U["log"].append([None if lab[k] is None else (lab[k], t8[k], desc[k][1]["cbp_l"] | desc[k][1]["cbp_c"] << 4 if lab[k] not in ("skip", "pcm") else None, after[k])
                     for k in range(n)])

    def same(a, b):
        return 0 <= b < n and sl[b] == sl[a] and sl[a] >= 0
    for k in range(n):
        if lab[k] is None:
            continue
        kind, m = desc[k]
        s = slices[sl[k]]
        left = k - 1 if k % mb_w else None
        right = k + 1 if (k + 1) % mb_w else None
        if lab[k] == "i8u":
            U["n"] += 1
            if k == s["first_mb"]:
                U["first"].add(k)
            U["avail"].add(("L" if left is not None and same(k, left) else "-", "T" if k >= mb_w and same(k, k - mb_w) else "-"))
            for q in (left, right, k - mb_w if k >= mb_w else None, k + mb_w if k + mb_w < n else None):
                if q is not None and lab[q] is not None:
                    U["beside"].add(lab[q])
            if left is not None and same(k, left) and lab[left] == "i8u":
                U["pairs"] += 1
            if k in ends:
                U["last_slice"] += 1
                if k == n - 1:
                    U["last_pic"] += 1
            elif same(k, k + 1):
                nk, nm = desc[k + 1]
                coded = nk == "i16" or (nk not in ("skip", "pcm") and (nm["cbp_l"] or nm["cbp_c"]))
                U["behind"].add((lab[k + 1], nm["dqp"] if coded else None))
            U["carried"].add((before[k], s["qp"], pic_init_qp))
            U["deblock"].add(s.get("deblock", (0, 0, 0))[0])
            U["slice"].add(s["type"])
            if s["type"] == "P" and left is not None and right is not None and same(k, left) and same(k, right):
                if all(desc[q][0] in INTER and not flag_present(*desc[q]) for q in (left, right)):
                    U["i8u_between"].add((lab[left], lab[right]))
        if kind in INTER:
            key = (kind, bool(m["cbp_l"]), m["cbp_c"], m.get("subs"), m.get("t8", 0) if flag_present(kind, m) else None)
            U["inter"].add(key)
            if left is not None and right is not None and same(k, left) and same(k, right) and t8[left] and t8[right]:
                U["between"].add(key)


class SynthT8(S.Synth):
    def __init__(self, mb_w, mb_h, **kw):
        kw.setdefault("profile", 100)
        super().__init__(mb_w, mb_h, **kw)

    def _pps(self, pps_id=0, cabac=0, t8=1):
        super()._pps(pps_id, cabac, t8)

    def picture(self, slices, idr=False):
        super().picture(slices, idr)
        tally(self.count, self.mb_w, self.n, slices, self.pic_init_qp)

    def _slice(self, si, s, idr):
        if all(kind in ("skip", "pcm", "i16") or (kind == "p16" and not m.get("t8")) for kind, m in s["mbs"]):
            return super()._slice(si, s, idr)
        C = self.count
        is_p = s["type"] == "P"
        b = Bits()
        num_ref, qp = self._header(b, s, idr)
        k, run = s["first_mb"], 0
        for kind, m in s["mbs"]:
            if kind == "skip":
                assert is_p
                for _ in range(m):
                    self.slice_of[k] = si; k += 1
                run += m
                continue
            if is_p:
                b.ue(run); C["skip_runs"].append(run); run = 0
            self.slice_of[k] = si
            if kind == "pcm":
                b.ue(25 + (5 if is_p else 0))
                C["pcm_phase"].add(len(b) % 8)
                while len(b) % 8:
                    b.u(1, 0)
                for c in m:
                    b.u(8, c)
                self.tc[k] = [16] * 24
            elif kind in INTER:
                assert is_p
                qp = self._inter(b, k, kind, m, num_ref, qp)
            elif kind in ("i8", "i4"):
                b.ue(5 if is_p else 0)                               # mb_type I_NxN
                if kind == "i8":
                    b.u(1, 1)                                        # transform_size_8x8_flag
                    for rem in m["modes"]:
                        if rem is None:
                            b.u(1, 1)
                        else:
                            b.u(1, 0); b.u(3, rem)
                else:
                    b.u(1, 0)
                    b.u(16, 0xffff)                                  # prev_intra4x4_pred_mode_flag of the 16 blocks
                b.ue(m.get("chroma_mode", 0))
                cbp = m["cbp_l"] | (m["cbp_c"] << 4)
                b.ue(TABLES["kCbpIntra"].index(cbp))
                if cbp:
                    qp = self._dqp(b, qp, m["dqp"])
                else:
                    self._qp_seen(qp)
                for b8 in range(4):
                    if m["cbp_l"] >> b8 & 1:
                        self._luma8x8(b, k, b8, m, kind == "i8", "luma")
                self._chroma(b, k, m)
            else:
                assert kind == "i16"
                b.ue(1 + 2 + 4 * m["cbp_c"] + (12 if m["cbp_l"] else 0) + (5 if is_p else 0))
                b.ue(0)
                qp = self._dqp(b, qp, m["dqp"])
                self._residual(b, k, "i16dc", 0, m["dc"], 16)
                if m["cbp_l"]:
                    for blk in range(16):
                        self._residual(b, k, "luma", blk, m["ac"].get(blk, [0] * 15), 15)
                self._chroma(b, k, m)
            k += 1
        if run:
            b.ue(run); C["skip_runs"].append(run)
        self.last_align = b.trailing(s.get("align", 0))
        C["align"].add(self.last_align)
        b.b = b.b[8:]
        self._nal(3, 5 if idr else 1, b)

    def _luma8x8(self, b, k, b8, m, t8, key8):
        """the four 4x4 blocks of 8x8 block b8: interleaved from 64 levels under the 8x8 transform, else their own 16 each"""
        if t8:
            c64 = m[key8].get(b8, [0] * 64)
            assert len(c64) == 64
            for j in range(4):
                self._residual(b, k, "luma", b8 * 4 + j, [c64[4 * i + j] for i in range(16)], 16)
        else:
            for j in range(4):
                self._residual(b, k, "luma", b8 * 4 + j, m["luma"].get(b8 * 4 + j, [0] * 16), 16)

    def _inter(self, b, k, kind, m, num_ref, qp):
        C = self.count
        b.ue(INTER.index(kind))
        if kind == "p8x8":
            for st in m["subs"]:
                b.ue(st)
        assert num_ref == 1 or kind == "p16"
        if num_ref > 1:
            assert 0 <= m["ref"] < num_ref
            if num_ref == 2:
                b.u(1, 1 - m["ref"])
            else:
                b.ue(m["ref"])
        C["num_ref_idx"][num_ref] = max(C["num_ref_idx"].get(num_ref, 0), m["ref"])
        pairs = 1 if kind == "p16" else sum(SUB_PARTS[st] for st in m["subs"]) if kind == "p8x8" else 2
        for _ in range(pairs):
            for v in m["mvd"]:
                b.se(v)
                C["mvd_min"] = min(C["mvd_min"], v); C["mvd_max"] = max(C["mvd_max"], v)
        cbp = m["cbp_l"] | (m["cbp_c"] << 4)
        b.ue(TABLES["kCbpInter"].index(cbp))
        t8 = m.get("t8", 0)
        assert flag_present(kind, m) or not t8
        if flag_present(kind, m):
            b.u(1, t8)                                               # transform_size_8x8_flag
        if cbp:
            qp = self._dqp(b, qp, m["dqp"])
        else:
            self._qp_seen(qp)
        for b8 in range(4):
            if m["cbp_l"] >> b8 & 1:
                self._luma8x8(b, k, b8, m, t8, "luma8")
        self._chroma(b, k, m)
        return qp
