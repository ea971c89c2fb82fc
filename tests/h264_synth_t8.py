"""tests/h264_synth.py with the 8x8 transform under CAVLC: a High-profile PPS with transform_8x8_mode_flag, and the macroblock
I_NxN with transform_size_8x8_flag = 1 (7.3.5, 7.3.5.1, 7.3.5.3.2) in I slices.  An 8x8 block's 64 coefficients travel as four
interleaved 4x4 blocks of 16 (coefficient 4 * i + j of the 8x8 scan is coefficient i of block j), each with the nC of its place.
Nothing in h264_synth.py changes; what is here is written from the same clauses."""
import h264_synth as S
from h264_synth import Bits, TABLES, i16  # noqa: F401


def i8(modes=(None, None, None, None), cbp_l=0, cbp_c=0, dqp=0, luma=None, cdc=None, cac=None, chroma_mode=0):
    """I_NxN with the 8x8 transform.  modes: per 8x8 block None (prev_intra8x8_pred_mode_flag = 1: the predicted mode) or
    rem_intra8x8_pred_mode 0..7; luma: {luma8x8BlkIdx: 64 levels in 8x8 scan order} for blocks whose cbp_l bit is set"""
    return ("i8", dict(modes=modes, cbp_l=cbp_l, cbp_c=cbp_c, dqp=dqp, luma=luma or {}, cdc=cdc, cac=cac or {}, chroma_mode=chroma_mode))


class SynthT8(S.Synth):
    def __init__(self, mb_w, mb_h, **kw):
        kw.setdefault("profile", 100)
        super().__init__(mb_w, mb_h, **kw)

    def _pps(self, pps_id=0, cabac=0, t8=1):
        super()._pps(pps_id, cabac, t8)

    def _slice(self, si, s, idr):
        if not any(kind == "i8" for kind, _ in s["mbs"]):
            return super()._slice(si, s, idr)
        assert s["type"] == "I"
        b = Bits()
        _, qp = self._header(b, s, idr)
        k = s["first_mb"]
        for kind, m in s["mbs"]:
            self.slice_of[k] = si
            if kind == "i8":
                b.ue(0)                                              # mb_type I_NxN
                b.u(1, 1)                                            # transform_size_8x8_flag
                for rem in m["modes"]:
                    if rem is None:
                        b.u(1, 1)
                    else:
                        b.u(1, 0); b.u(3, rem)
                b.ue(m["chroma_mode"])
                cbp = m["cbp_l"] | (m["cbp_c"] << 4)
                b.ue(TABLES["kCbpIntra"].index(cbp))
                if cbp:
                    qp = self._dqp(b, qp, m["dqp"])
                else:
                    self._qp_seen(qp)
                for b8 in range(4):
                    if m["cbp_l"] >> b8 & 1:
                        c64 = m["luma"].get(b8, [0] * 64)
                        assert len(c64) == 64
                        for j in range(4):
                            self._residual(b, k, "luma", b8 * 4 + j, [c64[4 * i + j] for i in range(16)], 16)
                self._chroma(b, k, m)
            else:
                assert kind == "i16"
                b.ue(1 + 2 + 4 * m["cbp_c"] + (12 if m["cbp_l"] else 0))
                b.ue(0)
                qp = self._dqp(b, qp, m["dqp"])
                self._residual(b, k, "i16dc", 0, m["dc"], 16)
                if m["cbp_l"]:
                    for blk in range(16):
                        self._residual(b, k, "luma", blk, m["ac"].get(blk, [0] * 15), 15)
                self._chroma(b, k, m)
            k += 1
        self.last_align = b.trailing(s.get("align", 0))
        self.count["align"].add(self.last_align)
        b.b = b.b[8:]
        self._nal(3, 5 if idr else 1, b)
