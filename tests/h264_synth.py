"""A small Annex-B CAVLC writer for tests: enough of the H.264 syntax to place any value in the fields whose range edges the corpus
never reaches (mb_skip_run, num_ref_idx_l0_active, level_prefix and levels, mvd, qp and mb_qp_delta, I_PCM at any bit phase).

Written from the syntax of ITU-T H.264 clauses 7.3 and 9.2, not from the product's parser or restorer.  Only the CONTENTS of the VLC
tables (coeff_token, total_zeros, run_before, coded_block_pattern) are read from the product's headers: the corpus pins them.

The subset: SPS (profile 66 or 100, frame macroblocks only, POC type 2), PPS (CAVLC, deblocking control present), I and P slice
headers (first_mb, num_ref_idx_active_override, sliding-window marking, no reordering), macroblocks P_Skip (as runs), P_L0_16x16,
I16x16 with DC prediction, I_PCM; residual_block_cavlc in full.  Pure Python and deterministic.  tests/h264_synth_cabac.py builds
on it: a slice may name another PPS ("pps") and carry cabac_init_idc ("init_idc"); _pps() writes further parameter sets.

The writer counts what it wrote (Synth.count), so that a test can assert that a stream reaches the edge it is named after:
  skip_runs            every mb_skip_run written, in order
  num_ref_idx          {num_ref_idx_l0_active: highest ref_idx written under it}
  prefix               {(level_prefix, suffixLength): count}
  coeff_token          {(nC class 0..4, maxNumCoeff, total_coeff, trailing_ones): count}; class 4 is chroma DC
  total_zeros          {(maxNumCoeff, total_coeff): largest total_zeros written}
  run_before           {(min(zerosLeft, 7), run_before): count}
  level_min/level_max, mvd_min/mvd_max, qp_min/qp_max, dqp_min/dqp_max
  pcm_phase            set of bit positions (mod 8) at which pcm_alignment_zero_bits started
  align                set of (alignment bits behind a slice's stop bit, their value)
  epb                  emulation prevention bytes inserted
"""
import os
import re

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "losslessh264_amd", "csrc", "host")


def _rows(txt, name):
    """the rows {..}, {..} of `name[..][..] = { {row}, {row} };` as lists of integer tuples"""
    body = txt[txt.index(name):]
    body = body[body.index("=") + 1:body.index("};")]
    body = re.sub(r"/\*.*?\*/", "", body)
    rows = []
    for row in re.findall(r"\{\s*((?:\{[^{}]*\}\s*,?\s*)+)\}", body):
        rows.append([tuple(int(x) for x in e.split(",")) for e in re.findall(r"\{([^{}]*)\}", row)])
    return rows


def _load_tables():
    vlc = open(os.path.join(_CSRC, "h264_vlc_tables.h")).read()
    tab = open(os.path.join(_CSRC, "h264_tables.h")).read()
    T = {}
    T["coeff_token"] = [{(e[2], e[3]): (e[0], e[1]) for e in row if e[0]} for row in _rows(vlc, "kCoeffToken[5][62]")]
    T["total_zeros"] = [{e[2]: (e[0], e[1]) for e in row if e[0]} for row in _rows(vlc, "kTotalZeros[16][16]")]
    T["total_zeros_cdc"] = [{e[2]: (e[0], e[1]) for e in row if e[0]} for row in _rows(vlc, "kTotalZerosChromaDc[4][4]")]
    T["run_before"] = [{e[2]: (e[0], e[1]) for e in row if e[0]} for row in _rows(vlc, "kRunBefore[8][15]")]
    for name in ("kCbpIntra", "kCbpInter"):
        m = re.search(name + r"\[48\]\s*=\s*\{([^}]*)\}", tab)
        T[name] = [int(x) for x in m.group(1).split(",")]
    assert [len(t) for t in T["coeff_token"]] == [62, 62, 62, 62, 14] and len(T["total_zeros"]) == 16 and len(T["run_before"]) == 8
    return T


TABLES = _load_tables()


class Bits:
    def __init__(self):
        self.b = []

    def u(self, n, v):
        assert 0 <= v < (1 << n), (n, v)
        for i in range(n - 1, -1, -1):
            self.b.append((v >> i) & 1)

    def ue(self, v):
        assert v >= 0
        n = (v + 1).bit_length()
        self.u(n - 1, 0)
        self.u(n, v + 1)

    def se(self, v):
        self.ue(2 * v - 1 if v > 0 else -2 * v)

    def vlc(self, len_code):
        self.u(len_code[0], len_code[1])

    def __len__(self):
        return len(self.b)

    def trailing(self, align=0):
        """rbsp_trailing_bits; align: what to put where the alignment zero bits belong (a decoder that stops at the picture's last
        macroblock never looks at them) -> (how many alignment bits, their value)"""
        self.b.append(1)
        n = -len(self.b) % 8
        self.u(n, align & ((1 << n) - 1))
        return n, align & ((1 << n) - 1)

    def bytes(self):
        assert len(self.b) % 8 == 0
        out = bytearray()
        for i in range(0, len(self.b), 8):
            v = 0
            for x in self.b[i:i + 8]:
                v = v * 2 + x
            out.append(v)
        return bytes(out)


def escape(rbsp):
    """emulation prevention (7.4.1): 00 00 0x with x <= 3 becomes 00 00 03 0x -> (bytes, how many were inserted)"""
    out, zeros, n = bytearray(), 0, 0
    for c in rbsp:
        if zeros >= 2 and c <= 3:
            out.append(3); zeros = 0; n += 1
        out.append(c)
        zeros = zeros + 1 if c == 0 else 0
    return bytes(out), n


# ---- macroblock descriptions ------------------------------------------------------------------------------------------------------
def skip(n):
    return ("skip", n)


def p16(ref=0, mvd=(0, 0), cbp_l=0, cbp_c=0, dqp=0, luma=None, cdc=None, cac=None):
    """P_L0_16x16.  luma: {luma4x4BlkIdx: 16 levels in scan order} for blocks whose 8x8 has its cbp_l bit; cdc: [4 Cb levels, 4 Cr
    levels]; cac: {(plane, blkIdx): 15 levels}"""
    return ("p16", dict(ref=ref, mvd=mvd, cbp_l=cbp_l, cbp_c=cbp_c, dqp=dqp, luma=luma or {}, cdc=cdc, cac=cac or {}))


def i16(cbp_l=0, cbp_c=0, dqp=0, dc=None, ac=None, cdc=None, cac=None):
    """I16x16, DC prediction for luma and chroma.  dc: 16 levels; ac: {luma4x4BlkIdx: 15 levels} (cbp_l 15 only)"""
    assert cbp_l in (0, 15)
    return ("i16", dict(cbp_l=cbp_l, cbp_c=cbp_c, dqp=dqp, dc=dc or [0] * 16, ac=ac or {}, cdc=cdc, cac=cac or {}))


def pcm(samples):
    assert len(samples) == 384
    return ("pcm", bytes(samples))


class Synth:
    def __init__(self, mb_w, mb_h, profile=66, num_ref_frames=1, pic_init_qp=26, log2_max_frame_num=8):
        self.mb_w, self.mb_h, self.n = mb_w, mb_h, mb_w * mb_h
        self.profile, self.num_ref_frames, self.pic_init_qp, self.l2fn = profile, num_ref_frames, pic_init_qp, log2_max_frame_num
        self.out = bytearray()
        self.frame_num = 0
        self.count = dict(skip_runs=[], num_ref_idx={}, prefix={}, coeff_token={}, total_zeros={}, run_before={}, level_min=0, level_max=0,
                          mvd_min=0, mvd_max=0, qp_min=99, qp_max=-1, dqp_min=0, dqp_max=0, pcm_phase=set(), align=set(), epb=0, pictures=0)
        self._sps()
        self._pps()

    # ---- NAL units ---------------------------------------------------------------------------------------------------------------
    def _nal(self, ref_idc, typ, bits):
        body, n = escape(bits.bytes())
        self.count["epb"] += n
        self.out += b"\x00\x00\x00\x01" + bytes([(ref_idc << 5) | typ]) + body

    def _sps(self):
        b = Bits()
        b.u(8, self.profile); b.u(8, 0); b.u(8, 40)
        b.ue(0)
        if self.profile == 100:
            b.ue(1); b.ue(0); b.ue(0); b.u(1, 0); b.u(1, 0)      # 4:2:0, 8 bits, no bypass, no scaling matrices
        b.ue(self.l2fn - 4)
        b.ue(2)                                                  # pic_order_cnt_type
        b.ue(self.num_ref_frames)
        b.u(1, 0)                                                # gaps_in_frame_num_value_allowed
        b.ue(self.mb_w - 1); b.ue(self.mb_h - 1)
        b.u(1, 1)                                                # frame_mbs_only
        b.u(1, 1)                                                # direct_8x8_inference
        b.u(1, 0); b.u(1, 0)                                     # no cropping, no VUI
        b.trailing()
        self._nal(3, 7, b)

    def _pps(self, pps_id=0, cabac=0, t8=0):
        b = Bits()
        b.ue(pps_id); b.ue(0)
        b.u(1, cabac)                                            # entropy_coding_mode_flag: CAVLC unless a subclass asks
        b.u(1, 0)                                                # bottom_field_pic_order_in_frame_present
        b.ue(0)                                                  # one slice group
        b.ue(0); b.ue(0)                                         # num_ref_idx default 1 / 1
        b.u(1, 0); b.u(2, 0)                                     # no weighted prediction
        b.se(self.pic_init_qp - 26); b.se(0); b.se(0)
        b.u(1, 1)                                                # deblocking_filter_control_present
        b.u(1, 0); b.u(1, 0)                                     # constrained_intra_pred, redundant_pic_cnt_present
        if self.profile == 100:
            b.u(1, t8); b.u(1, 0); b.se(0)                       # transform_8x8_mode, no scaling matrices, second chroma offset
        b.trailing()
        self._nal(3, 8, b)

    # ---- pictures ----------------------------------------------------------------------------------------------------------------
    def picture(self, slices, idr=False):
        """slices: list of dict(first_mb, type 'I' / 'P', qp, mbs=[...], num_ref=None or the overriding num_ref_idx_l0_active,
        deblock=(disable_idc, alpha_div2, beta_div2), align=the bits behind the slice's stop bit (a slice that ends its picture only))"""
        if idr:
            self.frame_num = 0
        self.tc = [[0] * 24 for _ in range(self.n)]              # total_coeff of the 16 luma (raster), 4 Cb, 4 Cr blocks
        self.slice_of = [-1] * self.n
        for si, s in enumerate(slices):
            self._slice(si, s, idr)
        self.frame_num = (self.frame_num + 1) % (1 << self.l2fn)
        self.count["pictures"] += 1

    def _header(self, b, s, idr):
        """slice_header (7.3.3) up to and including the deblocking fields -> (num_ref_idx_l0_active, SliceQPY)"""
        is_p = s["type"] == "P"
        b.u(8, 0)                                                # the NAL header's place, so that bit phases are those of the NAL unit
        b.ue(s["first_mb"]); b.ue(5 if is_p else 7); b.ue(s.get("pps", 0))
        b.u(self.l2fn, self.frame_num)
        if idr:
            b.ue(0)
        num_ref = 1
        if is_p:
            if s.get("num_ref") is not None:
                num_ref = s["num_ref"]
                b.u(1, 1); b.ue(num_ref - 1)
            else:
                b.u(1, 0)
            b.u(1, 0)                                            # no reordering
        if idr:
            b.u(1, 0); b.u(1, 0)
        else:
            b.u(1, 0)                                            # sliding window
        if is_p and s.get("init_idc") is not None:
            b.ue(s["init_idc"])                                  # cabac_init_idc (slices of a CABAC PPS only)
        qp = s["qp"]
        b.se(qp - self.pic_init_qp)
        dis, al, be = s.get("deblock", (0, 0, 0))
        b.ue(dis)
        if dis != 1:
            b.se(al); b.se(be)
        return num_ref, qp

    def _slice(self, si, s, idr):
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
                self.tc[k] = [16] * 24                           # (no mb_qp_delta: QPY,PRED of the next macroblock stays, 7.4.5)
            elif kind == "p16":
                assert is_p
                b.ue(0)
                if num_ref > 1:
                    assert 0 <= m["ref"] < num_ref
                    if num_ref == 2:
                        b.u(1, 1 - m["ref"])
                    else:
                        b.ue(m["ref"])
                C["num_ref_idx"][num_ref] = max(C["num_ref_idx"].get(num_ref, 0), m["ref"])
                for v in m["mvd"]:
                    b.se(v)
                    C["mvd_min"] = min(C["mvd_min"], v); C["mvd_max"] = max(C["mvd_max"], v)
                cbp = m["cbp_l"] | (m["cbp_c"] << 4)
                b.ue(TABLES["kCbpInter"].index(cbp))
                if cbp:
                    qp = self._dqp(b, qp, m["dqp"])
                else:
                    self._qp_seen(qp)
                for i8 in range(4):
                    for i4 in range(4):
                        blk = i8 * 4 + i4
                        if m["cbp_l"] >> i8 & 1:
                            self._residual(b, k, "luma", blk, m["luma"].get(blk, [0] * 16), 16)
                self._chroma(b, k, m)
            else:
                b.ue(1 + 2 + 4 * m["cbp_c"] + (12 if m["cbp_l"] else 0) + (5 if is_p else 0))
                b.ue(0)                                          # intra_chroma_pred_mode DC
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

    def _qp_seen(self, qp):
        C = self.count
        C["qp_min"] = min(C["qp_min"], qp); C["qp_max"] = max(C["qp_max"], qp)

    def _dqp(self, b, qp, dqp):
        C = self.count
        assert -26 <= dqp <= 25
        b.se(dqp)
        C["dqp_min"] = min(C["dqp_min"], dqp); C["dqp_max"] = max(C["dqp_max"], dqp)
        qp = (qp + dqp + 52) % 52
        self._qp_seen(qp)
        return qp

    def _chroma(self, b, k, m):
        if m["cbp_c"]:
            for pl in range(2):
                self._residual(b, k, "cdc", pl, (m["cdc"] or [[0] * 4] * 2)[pl], 4)
        if m["cbp_c"] == 2:
            for pl in range(2):
                for blk in range(4):
                    self._residual(b, k, "cac", (pl, blk), m["cac"].get((pl, blk), [0] * 15), 15)

    # ---- residual_block_cavlc (7.3.5.3.2, 9.2) ----------------------------------------------------------------------------------
    def _nc(self, k, slot_base, bx, by, w):
        """nC of the block at (bx, by) of a w x w grid whose totals live at self.tc[mb][slot_base + by * w + bx] (9.2.1)"""
        def total(mb, x, y):
            return self.tc[mb][slot_base + y * w + x]
        na = nb = None
        if bx > 0:
            na = total(k, bx - 1, by)
        elif k % self.mb_w > 0 and self.slice_of[k - 1] == self.slice_of[k]:
            na = total(k - 1, w - 1, by)
        if by > 0:
            nb = total(k, bx, by - 1)
        elif k >= self.mb_w and self.slice_of[k - self.mb_w] == self.slice_of[k]:
            nb = total(k - self.mb_w, bx, w - 1)
        if na is not None and nb is not None:
            return (na + nb + 1) >> 1
        return na if na is not None else (nb if nb is not None else 0)

    def _residual(self, b, k, kind, blk, coef, maxn):
        C = self.count
        assert len(coef) == maxn
        if kind == "cdc":
            cls = 4
        else:
            if kind == "cac":
                pl, i = blk
                nc = self._nc(k, 16 + 4 * pl, i & 1, i >> 1, 2)
            else:
                bx = (blk & 1) + 2 * (blk >> 2 & 1); by = (blk >> 1 & 1) + 2 * (blk >> 3)
                nc = self._nc(k, 0, bx, by, 4)
            cls = 0 if nc < 2 else 1 if nc < 4 else 2 if nc < 8 else 3
        pos = [i for i, v in enumerate(coef) if v]
        total = len(pos)
        levels = [coef[i] for i in reversed(pos)]                # highest frequency first
        t1 = 0
        while t1 < min(3, total) and abs(levels[t1]) == 1:
            t1 += 1
        if kind == "cac":
            self.tc[k][16 + 4 * blk[0] + blk[1]] = total
        elif kind == "luma":
            self.tc[k][((blk >> 1 & 1) + 2 * (blk >> 3)) * 4 + (blk & 1) + 2 * (blk >> 2 & 1)] = total
        b.vlc(TABLES["coeff_token"][cls][(total, t1)])
        key = (cls, maxn, total, t1)
        C["coeff_token"][key] = C["coeff_token"].get(key, 0) + 1
        if total == 0:
            return
        for v in levels[:t1]:
            b.u(1, 1 if v < 0 else 0)
        sl = 1 if total > 10 and t1 < 3 else 0
        for i, v in enumerate(levels[t1:]):
            C["level_min"] = min(C["level_min"], v); C["level_max"] = max(C["level_max"], v)
            code = 2 * v - 2 if v > 0 else -2 * v - 1
            if i == 0 and t1 < 3:
                code -= 2
            self._level(b, code, sl)
            if sl == 0:
                sl = 1
            if abs(v) > (3 << (sl - 1)) and sl < 6:
                sl += 1
        if total < maxn:
            tz = pos[-1] + 1 - total
            b.vlc((TABLES["total_zeros_cdc"] if kind == "cdc" else TABLES["total_zeros"])[total][tz])
            C["total_zeros"][(maxn, total)] = max(C["total_zeros"].get((maxn, total), 0), tz)
            left = tz
            for j in range(total - 1, 0, -1):
                if left <= 0:
                    break
                r = pos[j] - pos[j - 1] - 1
                b.vlc(TABLES["run_before"][min(left, 7)][r])
                key = (min(left, 7), r)
                C["run_before"][key] = C["run_before"].get(key, 0) + 1
                left -= r

    def _level(self, b, code, sl):
        """level_prefix / level_suffix for levelCode at suffixLength sl (9.2.2.1, read backwards)"""
        C = self.count
        if sl == 0 and code < 14:
            prefix, nsuf, suf = code, 0, 0
        elif sl == 0 and code < 30:
            prefix, nsuf, suf = 14, 4, code - 14
        elif sl > 0 and code < (15 << sl):
            prefix, nsuf, suf = code >> sl, sl, code & ((1 << sl) - 1)
        else:
            rest = code - (15 << sl) - (15 if sl == 0 else 0)
            prefix = 15
            while rest - ((1 << (prefix - 3)) - 4096) >= (1 << (prefix - 3)):
                prefix += 1
            nsuf, suf = prefix - 3, rest - ((1 << (prefix - 3)) - 4096)
            assert prefix == 15 or self.profile == 100, "level_prefix above 15 needs a High profile"
        b.u(prefix, 0); b.u(1, 1)
        if nsuf:
            b.u(nsuf, suf)
        C["prefix"][(prefix, sl)] = C["prefix"].get((prefix, sl), 0) + 1

    def bytes(self):
        return bytes(self.out)
