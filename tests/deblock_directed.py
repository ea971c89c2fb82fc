"""Directed inputs of the reconstruct kernel's in-loop filter (no GPU here): pictures whose samples, strengths and QPs are set so that
single lines sit on, and one short of, every threshold of filter_edge / deblock_phase (csrc/lh264_kernels.hip), on every entry of the
alpha / beta / tc0 tables under each of the three QP lookups (inner edge, left and top macroblock edge), on the reference's stale
tc0 of Cb's inner horizontal edge, on the scalar short cuts of deblock_phase and on lines that read what an earlier filter wrote.

Exact control of the samples a filter sees:
  bS 3, 4  IPCM macroblocks (their reconstruction is the given samples, their QP the record's); bS 4 on the edge between an inter
           macroblock without inner edges and an IPCM one, so that nothing touched the line before
  bS 1     P macroblocks with zero vectors over an unfiltered IPCM reference whose reference INDICES differ (both name one picture)
  bS 2     a lone DC coefficient of 16: a nonzero count whose residual is (32 + 16) >> 6 = 0
  bS 1 on edges 1 and 3: vectors 4 quarter samples apart along the edge, over content that does not change in that direction
A *cell* is a condition on one line of the oracle's trace (oracle_lib.recon_frame_traced), which sees the samples as they are when
the edge is filtered.  cells() evaluates them; tests/test_deblock_directed.py demands every one, tests/test_deblock_directed_gpu.py
runs the pictures through the kernel."""
import numpy as np

import oracle_lib as O
import recon_directed as D
from synth import IPCM, SKIP

# H.264 Tables 8-16 (alpha', beta') and 8-17 (tC0 for bS 1, 2, 3), by indexA / indexB
ALPHA = np.array([0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144,
                             162, 182, 203, 226, 255, 255])
BETA = np.array([0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17,
                            18, 18])
TC0 = np.array([[0, 0, 0]] * 17 + [[0, 0, 1]] * 4 + [[0, 1, 1]] * 2 + [[1, 1, 1]] * 4 + [[1, 1, 2]] * 4 + [[1, 2, 3]] * 2 +
               [[2, 2, 3], [2, 2, 4], [2, 3, 4], [2, 3, 4], [3, 3, 5], [3, 4, 6], [3, 4, 6], [4, 5, 7], [4, 5, 8], [4, 6, 9], [5, 7, 10], [6, 8, 11],
                [6, 8, 13], [7, 10, 14], [8, 11, 16], [9, 12, 18], [10, 13, 20], [11, 15, 23], [13, 17, 25]])
assert len(ALPHA) == len(BETA) == len(TC0) == 52
IDX = range(16, 52)            # the indices with a nonzero alpha / beta


def tab(i):
    return np.clip(i, 0, 51)


def tc_of(idx, bs, luma):
    """the tc the reference passes for a line: tc0 (luma), tc0 + 1 (chroma); 0 for bS 4, -1 for bS 0"""
    idx, bs = np.asarray(idx), np.asarray(bs)
    t = TC0[tab(idx), np.clip(bs - 1, 0, 2)] + np.where(luma, 0, 1)
    return np.where(bs == 0, -1, np.where(bs == 4, 0, t))


# ---- the filter, restated in numpy ----------------------------------------------------------------------------------------------------
def model(before, bs, alpha, beta, tc, luma):
    """the four edge filters on lines p3 p2 p1 p0 q0 q1 q2 q3 (one per row of `before`) -> dict: `out` and every decision on the way"""
    b = np.asarray(before).astype(np.int64)
    bs, alpha, beta, tc, luma = (np.asarray(a) for a in (bs, alpha, beta, tc, luma))
    p3, p2, p1, p0, q0, q1, q2, q3 = (b[:, i] for i in range(8))
    d = np.abs(p0 - q0)
    on = (bs > 0) & (d < alpha) & (np.abs(p1 - p0) < beta) & (np.abs(q1 - q0) < beta)
    ap, aq = luma & (np.abs(p2 - p0) < beta), luma & (np.abs(q2 - q0) < beta)
    tc0 = np.maximum(np.where(luma, tc, tc - 1), 0)
    t = np.where(luma, tc0 + ap + aq, tc0 + 1)
    raw = (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3
    dl = np.clip(raw, -t, t)
    avg = (p0 + q0 + 1) >> 1
    cp, cq = (p2 + avg - 2 * p1) >> 1, (q2 + avg - 2 * q1) >> 1
    out = b.copy()
    lt = on & (bs < 4)
    out[:, 3] = np.where(lt, np.clip(p0 + dl, 0, 255), p0)
    out[:, 4] = np.where(lt, np.clip(q0 - dl, 0, 255), q0)
    out[:, 2] = np.where(lt & ap, p1 + np.clip(cp, -tc0, tc0), p1)
    out[:, 5] = np.where(lt & aq, q1 + np.clip(cq, -tc0, tc0), q1)
    s4 = on & (bs == 4)
    small = luma & (d < (alpha >> 2) + 2)
    sp, sq = small & ap, small & aq
    out[:, 3] = np.where(s4, np.where(sp, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, (2 * p1 + p0 + q1 + 2) >> 2), out[:, 3])
    out[:, 4] = np.where(s4, np.where(sq, (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3, (2 * q1 + q0 + p1 + 2) >> 2), out[:, 4])
    out[:, 2] = np.where(s4 & sp, (p2 + p1 + p0 + q0 + 2) >> 2, out[:, 2])
    out[:, 5] = np.where(s4 & sq, (p0 + q0 + q1 + q2 + 2) >> 2, out[:, 5])
    out[:, 1] = np.where(s4 & sp, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, p2)
    out[:, 6] = np.where(s4 & sq, (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3, q2)
    return dict(out=out, on=on, lt=lt, s4=s4, ap=ap, aq=aq, tc0=tc0, t=t, raw=raw, dl=dl, cp=cp, cq=cq, small=small, sp=sp, sq=sq, d=d,
                dp1=p1 - p0, dq1=q1 - q0, dp2=p2 - p0, dq2=q2 - q0, dq=q0 - p0, p=b)


def model_of(r):
    return model(r["before"], r["bs"], r["alpha"], r["beta"], r["tc"], r["plane"] == 0)


def edge_class(r):
    """0 inner edge, 1 left macroblock edge, 2 top macroblock edge: the three lookups of deblock_phase"""
    return np.where(r["edge"] > 0, 0, np.where(r["dir"] == 0, 1, 2))


CLS = ("inner", "left", "top")


# ---- cells on single lines: families A-E ----------------------------------------------------------------------------------------------
def max_raw(alpha, beta):
    """the largest |(4 (q0 - p0) + (p1 - q1) + 4) >> 3| of a line that passes the three gates: q0 - p0 = alpha - 1, p1 - p0 = beta - 1,
    q0 - q1 = beta - 1, so p1 - q1 = 2 (beta - 1) - (alpha - 1)"""
    return (3 * (alpha - 1) + 2 * (beta - 1) + 4) >> 3


MAX_SPREAD = 24              # indexB - indexA = beta_offset - alpha_c0_offset, both -12..12


def tc_pin_spread(idx, bs, luma):
    """indexB - indexA (0 or MAX_SPREAD) under which a line filtered at indexA = idx can have an unclipped |delta| >= t + 1, the
    smallest t being tc0 (luma: ap and aq off), tc0 + 1 (chroma); None if not even the largest beta the offsets allow gives one"""
    for spread in (0, MAX_SPREAD):
        if max_raw(int(ALPHA[idx]), int(BETA[min(idx + spread, 51)])) >= int(TC0[idx][bs - 1]) + (1 if luma else 2):
            return spread
    return None


def tc_pin_reachable(idx, bs, luma):
    return tc_pin_spread(idx, bs, luma) is not None


def line_cell_names():
    """every cell of families A-E that is a condition on one line -> (names, {name: reason} of those no line can reach)"""
    names, unreach = [], {}
    for pl in "YC":
        for bs in (1, 2, 3, 4):
            for gate in ("pq", "p1", "q1"):
                for kind in ("pass", "fail"):
                    for sg in "+-":
                        names.append("A/%s/bs%d/%s/%s/%s" % (pl, bs, gate, kind, sg))
    names += ["A/alpha0_beta+", "A/alpha+_beta0"]
    names += ["B/%s/%s/%s" % (g, k, s) for g in ("p2", "q2") for k in ("pass", "fail") for s in "+-"]
    names += ["B/pair/ap%daq%d" % (a, b) for a in (0, 1) for b in (0, 1)]
    names += ["B/delta/" + k for k in ("inside", "eq+", "eq-", "beyond+", "beyond-")]
    names += ["B/%s/%s" % (s, k) for s in ("p1corr", "q1corr") for k in ("inside", "clip+", "clip-")]
    names += ["B/tc0_0/ap_only", "B/tc0_0/aq_only"]
    names += ["B/clip_u8/" + k for k in ("p0>255", "q0<0", "p0<0", "q0>255")]
    names += ["C/small/pass", "C/small/fail"] + ["C/pair/sp%dsq%d" % (a, b) for a in (0, 1) for b in (0, 1)]
    names += ["C/ap_not_small", "C/aq_not_small", "C/p3_weight", "C/q3_weight"]
    names += ["D/lt4/%s/%s" % (z, k) for z in ("tc0_0", "tc0_pos") for k in ("inside", "eq+", "eq-", "beyond+", "beyond-")]
    names += ["D/eq4", "D/p1_stays/lt4", "D/q1_stays/lt4", "D/p1_stays/eq4", "D/q1_stays/eq4"]
    for c in CLS:
        for i in IDX:
            names += ["E/%s/A%d/%s" % (c, i, k) for k in ("pass", "fail")] + ["E/%s/B%d/%s" % (c, i, k) for k in ("pass", "fail")]
            for pl in "YC":
                for bs in (1, 2, 3):
                    n = "E/%s/tc/%s/A%d/bs%d" % (c, pl, i, bs)
                    names.append(n)
                    if bs == 3 and c != "inner":
                        unreach[n] = "bS 3 arises on inner edges of intra macroblocks only: their macroblock edges carry bS 4 (deblock_mb)"
                    elif not tc_pin_reachable(i, bs, pl == "Y"):
                        bmax = int(BETA[min(i + MAX_SPREAD, 51)])
                        unreach[n] = ("no filtered line has |delta| > t here: alpha %d and the largest beta the offsets allow, %d, bound it by %d, "
                                      "t is at least %d" % (ALPHA[i], bmax, max_raw(int(ALPHA[i]), bmax), TC0[i][bs - 1] + (0 if pl == "Y" else 1)))
    names += ["E/clamp/A<0", "E/clamp/A>51", "E/clamp/B<0", "E/clamp/B>51"]
    return names, unreach


def line_cells(r):
    """records -> {cell: mask over the records} for the cells of line_cell_names (E/clamp and the untraced cases are in cells())"""
    m = model_of(r)
    luma = r["plane"] == 0
    al, be, bs = r["alpha"].astype(int), r["beta"].astype(int), r["bs"]
    d, dp1, dq1, dp2, dq2, dq = m["d"], m["dp1"], m["dq1"], m["dp2"], m["dq2"], m["dq"]
    g_pq, g_p1, g_q1 = d < al, np.abs(dp1) < be, np.abs(dq1) < be
    live = (bs > 0) & (al > 0) & (be > 0)
    out = {}
    for pl, sel in (("Y", luma), ("C", ~luma)):
        for b in (1, 2, 3, 4):
            s = sel & live & (bs == b)
            for gate, val, thr, others in (("pq", dq, al, g_p1 & g_q1), ("p1", dp1, be, g_pq & g_q1), ("q1", dq1, be, g_pq & g_p1)):
                for kind, off in (("pass", 1), ("fail", 0)):
                    for sg, sv in (("+", 1), ("-", -1)):
                        out["A/%s/bs%d/%s/%s/%s" % (pl, b, gate, kind, sg)] = s & others & (val == sv * (thr - off))
    out["A/alpha0_beta+"] = (bs > 0) & (al == 0) & (be > 0)
    out["A/alpha+_beta0"] = (bs > 0) & (al > 0) & (be == 0)
    lt, s4, t, tc0, raw = m["lt"], m["s4"], m["t"], m["tc0"], m["raw"]
    yl = luma & lt
    for g, val in (("p2", dp2), ("q2", dq2)):
        for kind, off in (("pass", 1), ("fail", 0)):
            for sg, sv in (("+", 1), ("-", -1)):
                out["B/%s/%s/%s" % (g, kind, sg)] = yl & (val == sv * (be - off)) & (be > 1)
    for a in (0, 1):
        for b in (0, 1):
            out["B/pair/ap%daq%d" % (a, b)] = yl & (m["ap"] == a) & (m["aq"] == b)
            out["C/pair/sp%dsq%d" % (a, b)] = luma & s4 & m["small"] & (m["ap"] == a) & (m["aq"] == b)

    def delta_cells(prefix, sel):
        out[prefix + "inside"] = sel & (np.abs(raw) < t) & (raw != 0)
        out[prefix + "eq+"], out[prefix + "eq-"] = sel & (raw == t) & (t > 0), sel & (raw == -t) & (t > 0)
        out[prefix + "beyond+"], out[prefix + "beyond-"] = sel & (raw > t), sel & (raw < -t)
    delta_cells("B/delta/", yl)
    for s, c, a in (("p1corr", m["cp"], m["ap"]), ("q1corr", m["cq"], m["aq"])):
        out["B/%s/inside" % s] = yl & a & (np.abs(c) <= tc0) & (c != 0)
        out["B/%s/clip+" % s], out["B/%s/clip-" % s] = yl & a & (c > tc0), yl & a & (c < -tc0)
    out["B/tc0_0/ap_only"] = yl & (tc0 == 0) & m["ap"] & ~m["aq"] & (raw != 0) & (m["cp"] != 0)
    out["B/tc0_0/aq_only"] = yl & (tc0 == 0) & m["aq"] & ~m["ap"] & (raw != 0) & (m["cq"] != 0)
    p0, q0 = m["p"][:, 3], m["p"][:, 4]
    out["B/clip_u8/p0>255"], out["B/clip_u8/p0<0"] = yl & (p0 + m["dl"] > 255), yl & (p0 + m["dl"] < 0)
    out["B/clip_u8/q0<0"], out["B/clip_u8/q0>255"] = yl & (q0 - m["dl"] < 0), yl & (q0 - m["dl"] > 255)
    y4 = luma & s4
    out["C/small/pass"] = y4 & (al % 4 != 0) & (d == (al >> 2) + 1)
    out["C/small/fail"] = y4 & (al % 4 != 0) & (d == (al >> 2) + 2)
    out["C/ap_not_small"], out["C/aq_not_small"] = y4 & m["ap"] & ~m["small"], y4 & m["aq"] & ~m["small"]
    p = m["p"]
    out["C/p3_weight"] = y4 & m["sp"] & (((p[:, 0] + 3 * p[:, 1] + p[:, 2] + p[:, 3] + p[:, 4] + 4) >> 3) != m["out"][:, 1])
    out["C/q3_weight"] = y4 & m["sq"] & (((p[:, 7] + 3 * p[:, 6] + p[:, 5] + p[:, 4] + p[:, 3] + 4) >> 3) != m["out"][:, 6])
    cl = ~luma & lt
    delta_cells("D/lt4/tc0_0/", cl & (tc0 == 0))
    delta_cells("D/lt4/tc0_pos/", cl & (tc0 > 0))
    out["D/eq4"] = ~luma & s4 & (m["out"][:, 3] != p0)
    # what the luma filter would do to p1 / q1 of the same samples under the same alpha, beta and tc0
    ml = model(r["before"], bs, al, be, tc0, np.ones(len(r), bool))
    for s, i in (("p1", 2), ("q1", 5)):
        out["D/%s_stays/lt4" % s] = cl & (ml["out"][:, i] != p[:, i])
        out["D/%s_stays/eq4" % s] = ~luma & s4 & (ml["out"][:, i] != p[:, i])
    cls = edge_class(r)
    on = m["on"]
    open_b = g_p1 & g_q1
    pin = on & (bs < 4) & (np.abs(raw) >= t + 1)
    ia, ib, it = tab(r["idx_a"].astype(int)), tab(r["idx_b"].astype(int)), tab(r["idx_tc"].astype(int))
    for ci, c in enumerate(CLS):
        sc = (cls == ci) & live
        for i in IDX:
            sa = sc & luma & (ia == i)
            out["E/%s/A%d/pass" % (c, i)], out["E/%s/A%d/fail" % (c, i)] = sa & open_b & (d == al - 1), sa & open_b & (d == al)
            sb = sc & luma & (ib == i) & g_pq
            dmax = np.maximum(np.abs(dp1), np.abs(dq1))
            out["E/%s/B%d/pass" % (c, i)], out["E/%s/B%d/fail" % (c, i)] = sb & (dmax == be - 1), sb & (dmax == be)
            for pl, sel in (("Y", luma), ("C", ~luma)):
                for b in (1, 2, 3):
                    out["E/%s/tc/%s/A%d/bs%d" % (c, pl, i, b)] = sc & sel & pin & (it == i) & (bs == b)
    out["E/clamp/A<0"], out["E/clamp/A>51"] = r["idx_a"] < 0, r["idx_a"] > 51
    out["E/clamp/B<0"], out["E/clamp/B>51"] = r["idx_b"] < 0, r["idx_b"] > 51
    return out


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def zorder(bx, by):
    return (bx & 1) | (by & 1) << 1 | (bx >> 1) << 2 | (by >> 1) << 3


class Scene:
    """a P picture of zero vectors over an unfiltered IPCM picture that holds the wanted samples: what the P picture's filter sees is
    what was put into Y, U, V.  kind per macroblock: F one partition (ref r), V left / right halves (r, 1 - r), H upper / lower halves,
    Q quadrants (r, 1-r, 1-r, r), X sixteen 4x4 partitions with the vectors of .mv, S skipped, I IPCM."""

    def __init__(self, name, mb_w, mb_h, kind="F", qp=30, ao=0, bo=0, idc=0, n_slices=1, base=128):
        n = mb_w * mb_h
        self.name, self.mb_w, self.mb_h, self.n_slices = name, mb_w, mb_h, n_slices
        self.Y = np.full((16 * mb_h, 16 * mb_w), base, np.uint8)
        self.U = np.full((8 * mb_h, 8 * mb_w), base, np.uint8)
        self.V = np.full((8 * mb_h, 8 * mb_w), base, np.uint8)
        self.kind, self.ref = [kind] * n, np.zeros(n, int)
        self.qp_y, self.qp_c = np.full(n, qp), np.full((n, 2), qp)
        self.mv = np.zeros((n, 16, 2), np.int16)
        self.t8 = np.zeros(n, bool)
        self.nz = []                                     # (macroblock, bx, by): a DC coefficient of 16 in that 4x4 block
        self.slice_par = [dict(ao=ao, bo=bo, idc=idc) for _ in range(n_slices)]
        self.first_mb = None                             # explicit slice starts (default: even runs)

    def k(self, x, y):
        return y * self.mb_w + x

    def plane(self, p):
        return (self.Y, self.U, self.V)[p]

    def put(self, p, x, y, dir_, edge, i, line):
        """line p3..q3 across edge `edge` (luma numbering 0..3; chroma: 0, 2) of macroblock (x, y), on its row (dir 0) / column i"""
        bsz, e = (8, edge // 2 * 4) if p else (16, 4 * edge)
        a = self.plane(p)
        if dir_ == 0:
            a[bsz * y + i, bsz * x + e - 4:bsz * x + e + 4] = line
        else:
            a[bsz * y + e - 4:bsz * y + e + 4, bsz * x + i] = line

    def frames(self):
        ref = D.pcm_picture(self.mb_w, self.mb_h, self.Y, self.U, self.V, fid=0)
        f = D.new_frame(1, self.mb_w, self.mb_h, [0], n_slices=self.n_slices)
        n = self.mb_w * self.mb_h
        if self.first_mb is not None:
            b = list(self.first_mb) + [n]
            for s in range(self.n_slices):
                f.slices[s]["first_mb"], f.slices[s]["n_mbs"] = b[s], b[s + 1] - b[s]
                f.mbs["slice_id"][b[s]:b[s + 1]] = s
        for s, par in enumerate(self.slice_par):
            sl = f.slices[s]
            sl["alpha_c0_offset"], sl["beta_offset"], sl["deblock_idc"] = par["ao"], par["bo"], par["idc"]
            sl["n_refs"] = 2
            sl["ref_slot"][:2] = 0                       # both indices name the one reference picture
        pcm = ref.coeffs
        for k in range(n):
            m, kind, r = f.mbs[k], self.kind[k], int(self.ref[k])
            if kind == "I":
                m["mb_type"], m["flags"], m["nzc"], m["chroma_mode"] = IPCM, 2, 16, 6
                f.coeffs[k] = pcm[k]
            elif kind == "S":
                D.set_inter(m, "16x16", [(0, 0)], ref=0)
                m["mb_type"] = SKIP
            elif kind == "X":
                D.set_inter(m, "8x8" if self.t8[k] else "4x4", [(0, 0)] * 16, ref=r)
                m["mv"] = self.mv[k]
            else:
                shape = {"F": "16x16", "V": "8x16", "H": "16x8", "Q": "8x8"}[kind]
                D.set_inter(m, shape, [tuple(self.mv[k][0])] * len(D.SHAPES[shape][2]))
                m["ref_idx"] = {"F": (r, r, r, r), "V": (r, 1 - r, r, 1 - r), "H": (r, r, 1 - r, 1 - r), "Q": (r, 1 - r, 1 - r, r)}[kind]
            m["qp_y"], m["qp_c"] = self.qp_y[k], self.qp_c[k]
            if self.t8[k]:
                m["flags"] = int(m["flags"]) | 1
        for (k, bx, by) in self.nz:
            assert self.kind[k] not in "IS"
            m = f.mbs[k]
            zb = zorder(bx, by)
            f.coeffs[k][(zb >> 2) * 64 if self.t8[k] else zb * 16] = 16
            m["cbp"] = int(m["cbp"]) | 1 << (zb >> 2)
        for k in sorted(set(k for k, _, _ in self.nz)):
            D.set_nzc(f.mbs[k], f.coeffs[k])
        return [ref, f]


def fit(d0, ep1=0, eq1=0, ep2=None, eq2=None, ep3=0, eq3=0, anchor=128):
    """a line from differences: q0 = p0 + d0, p1 = p0 + ep1, p2 = p0 + ep2 (default p1), p3 = p2 + ep3, q1 = q0 + eq1, ...; p0 as near
    to `anchor` as 0..255 allows.  None if no p0 fits."""
    ep2 = ep1 if ep2 is None else ep2
    eq2 = eq1 if eq2 is None else eq2
    rel = np.array([ep2 + ep3, ep2, ep1, 0, d0, d0 + eq1, d0 + eq2, d0 + eq2 + eq3])
    lo, hi = -rel.min(), 255 - rel.max()
    if lo > hi:
        return None
    return (rel + min(max(anchor - d0 // 2, lo), hi)).astype(np.uint8)


def mirror(line):
    return line[::-1].copy()


def battery(alpha, beta, tc0, bs, luma):
    """the lines of families A-D for one set of parameters: each gate at its threshold and one short, both signs; (ap, aq) pairs; the
    delta at, inside and beyond its clip; the p1 / q1 corrections; the strong filter's choices"""
    assert alpha > 0 and beta > 1
    L = []
    mid = min(alpha - 1, 5)
    for sg in (1, -1):
        L += [fit(sg * (alpha - 1)), fit(sg * alpha)]
        for e in (beta - 1, beta):
            L += [fit(mid, ep1=sg * e), fit(mid, eq1=sg * e), fit(-mid, ep1=sg * e), fit(-mid, eq1=sg * e)]
            L += [fit(mid, ep2=sg * e), fit(mid, eq2=sg * e)]
    far = beta + 1
    for a in (0, far):
        for b in (0, far):
            L += [fit(mid, ep2=a, eq2=-b), fit(min(alpha - 1, 20), ep2=a, eq2=-b)]
    if bs < 4:
        # the delta (3 d0 + 4) >> 3 of a line with p1 = p0, q1 = q0 against every t this line can have
        for t in sorted(set([tc0 + (2 if luma else 1), tc0 + (0 if luma else 1)])):
            for sg in (1, -1):
                want = {sg * t: None, sg * (t + 2): None, sg * max(t - 1, 1): None}
                for d0 in range(1, alpha):
                    raw = (3 * sg * d0 + 4) >> 3
                    if raw in want and want[raw] is None:
                        want[raw] = fit(sg * d0) if t == tc0 + (2 if luma else 1) else fit(sg * d0, ep2=far, eq2=-far)
                L += [w for w in want.values() if w is not None]
        for sg in (1, -1):                                # corrections of p1 (and, mirrored, q1): inside, clipped
            L += [fit(sg * 2, ep2=sg * 2), fit(sg * min(alpha - 1, 20), ep2=sg * (beta - 1)), fit(sg * min(alpha - 1, 20), ep2=sg * (beta - 1), eq2=-sg * far)]
        L += [fit(min(alpha - 1, 4), ep2=0, eq2=far), fit(min(alpha - 1, 4), ep2=far, eq2=0)]
        if beta > 4:                                      # clip_u8 at both ends, on both sides
            L += [np.array([255, 255, 255, 255, 255, 251, 251, 251], np.uint8), np.array([0, 0, 0, 0, 0, 5, 5, 5], np.uint8),
                  np.array([4, 4, 4, 0, 0, 0, 0, 0], np.uint8), np.array([250, 250, 250, 255, 255, 255, 255, 255], np.uint8)]
    else:
        s = (alpha >> 2) + 2
        for sg in (1, -1):
            for d0 in (s - 1, s):
                for a in (0, far):
                    for b in (0, far):
                        L += [fit(sg * d0, ep2=sg * a, eq2=-sg * b, ep3=-9, eq3=9)]
        L += [fit(8, ep2=beta - 1), fit(-8, eq2=beta - 1)]
    L = [l for l in L if l is not None]
    L += [mirror(l) for l in L]
    seen, outl = set(), []
    for l in L:
        if l.tobytes() not in seen:
            seen.add(l.tobytes())
            outl.append(l)
    return outl


def _rows(lines, per):
    return [lines[i:i + per] for i in range(0, len(lines), per)]


def inner_scene(name, groups, bs, luma, qps, ao=0, bo=0):
    """1 x N: macroblock j carries groups[j] (<= 16 luma / 8 + 8 chroma lines) on its first inner vertical edge, rows exact: bS 1 by
    reference indices (V) on edge 2, bS 2 by a coefficient in every block right of edge 2, bS 3 IPCM on edge 1 (no left neighbour)"""
    s = Scene(name, 1, len(groups), kind="I" if bs == 3 else "V" if bs == 1 else "F", ao=ao, bo=bo)
    for j, g in enumerate(groups):
        s.qp_y[j], s.qp_c[j] = qps[j], qps[j]
        if bs == 2:
            s.nz += [(j, 2, by) for by in range(4)]
        for i, l in enumerate(g):
            if luma:
                s.put(0, 0, j, 0, 1 if bs == 3 else 2, i, l)
            else:
                s.put(1 + i // 8, 0, j, 0, 2, i % 8, l)
    return s


def left_scene(name, groups, bs, luma, qps, ao=0, bo=0):
    """2 x N: the left edge of macroblock (1, j): bS 4 IPCM beside an inter macroblock without inner edges, bS 1 by the reference index,
    bS 2 by a coefficient in every block right of the edge.  qps[j] = (left, current)"""
    s = Scene(name, 2, len(groups), kind="F", ao=ao, bo=bo)
    for j, g in enumerate(groups):
        k = s.k(1, j)
        s.qp_y[k - 1], s.qp_c[k - 1], s.qp_y[k], s.qp_c[k] = qps[j][0], qps[j][0], qps[j][1], qps[j][1]
        if bs == 4:
            s.kind[k] = "I"
        elif bs == 1:
            s.ref[k] = 1
        else:
            s.nz += [(k, 0, by) for by in range(4)]
        for i, l in enumerate(g):
            if luma:
                s.put(0, 1, j, 0, 0, i, l)
            else:
                s.put(1 + i // 8, 1, j, 0, 0, i % 8, l)
    return s


def top_scene(name, groups, bs, luma, qps, ao=0, bo=0):
    """N x 2: the top edge of macroblock (j, 1).  bS 1: by the reference index, no vertical edge is live, 16 (8 + 8) columns each their
    own line.  bS 2 (a coefficient in blocks (1, 0) and (2, 0)) and bS 4 (IPCM) have live vertical edges around the line: one line a
    macroblock, the same in every column, so that those edges change nothing.  qps[j] = (top, current)"""
    s = Scene(name, len(groups), 2, kind="F", ao=ao, bo=bo)
    for j, g in enumerate(groups):
        k = s.k(j, 1)
        s.qp_y[j], s.qp_c[j], s.qp_y[k], s.qp_c[k] = qps[j][0], qps[j][0], qps[j][1], qps[j][1]
        if bs == 4:
            s.kind[k] = "I"
        elif bs == 1:
            s.ref[k] = 1
        else:
            s.nz += [(k, 1, 0), (k, 2, 0)]
        if bs == 1:
            for i, l in enumerate(g):
                if luma:
                    s.put(0, j, 1, 1, 0, i, l)
                else:
                    s.put(1 + i // 8, j, 1, 1, 0, i % 8, l)
        else:
            assert len(g) == 1
            for i in range(16 if luma else 8):
                for p in ((0,) if luma else (1, 2)):
                    s.put(p, j, 1, 1, 0, i, g[0])
    return s


# ---- families A-D: the battery at a middle QP and at one where tc0 is 0 ----------------------------------------------------------------
def family_abcd():
    scenes = []
    for idx in (35, 22):              # alpha 45 (no multiple of 4), beta 10, tc0 2 3 4 | alpha 9, beta 3, tc0 0 1 1
        for bs in (1, 2, 3, 4):
            if idx == 22 and bs > 1:
                continue
            tc0 = 0 if bs == 4 else int(TC0[idx][bs - 1])
            for luma in (True, False):
                groups = _rows(battery(int(ALPHA[idx]), int(BETA[idx]), tc0, bs, luma), 16)
                name = "abcd idx%d bs%d %s" % (idx, bs, "Y" if luma else "C")
                for gi, gg in enumerate(_rows(groups, 4)):
                    if bs == 4:
                        scenes.append(left_scene("%s #%d" % (name, gi), gg, 4, luma, [(idx - 2, idx + 2)] * len(gg)))
                    else:
                        scenes.append(inner_scene("%s #%d" % (name, gi), gg, bs, luma, [idx] * len(gg)))
    # alpha | beta == 0 and the two mixed cases: IPCM columns whose offsets push one index below 16
    for name, ao, bo in (("zero_ab", -12, -12), ("alpha0", -12, 12), ("beta0", 12, -12)):
        g = [[fit(3), fit(-3), fit(1, ep1=1), fit(0)]] * 3
        scenes.append(inner_scene("abcd " + name, g, 3, True, [20, 14, 26], ao=ao, bo=bo))
        scenes.append(inner_scene("abcd %s C" % name, g, 3, False, [20, 14, 26], ao=ao, bo=bo))
    return scenes


# ---- family E: every table entry under each of the three lookups ----------------------------------------------------------------------
def table_lines(idx, bs, luma, spread=0):
    """alpha and beta at and one short of the threshold, and a line whose delta is clipped by more than 1 (None where no line is),
    for indexA = idx and indexB = idx + spread"""
    a, b, tc0 = int(ALPHA[idx]), int(BETA[min(idx + spread, 51)]), int(TC0[idx][bs - 1])
    sg = 1 if idx & 1 else -1
    mid = min(a - 1, 6)
    L = [fit(sg * (a - 1)), fit(sg * a), fit(sg * mid, ep1=sg * (b - 1)), fit(sg * mid, ep1=sg * b), fit(-sg * mid, eq1=sg * (b - 1)), fit(-sg * mid, eq1=sg * b)]
    pin = None
    if max_raw(a, b) >= tc0 + (1 if luma else 2):
        t = tc0 + (0 if luma else 1)
        for d0 in range(1, a):                      # the smallest step that does it, the gates as open as they go
            l = fit(sg * d0, ep1=sg * (b - 1), eq1=-sg * (b - 1), ep2=sg * (b + 1), eq2=-sg * (b + 1))
            if l is not None and abs((4 * sg * d0 + 2 * sg * (b - 1) - sg * d0 + 4) >> 3) >= t + 1:
                pin = l
                break
    return L, pin


def _avg_pair(idx, odd):
    """(neighbour, current) QPs whose rounded average is idx and which both differ from it"""
    cur = min(51, idx + 3)
    return (2 * idx - cur - (1 if odd else 0), cur)


def family_e():
    scenes = []
    for bs in (1, 2, 3):
        for luma in (True, False):
            jobs = []
            for idx in IDX:
                L, pin = table_lines(idx, bs, luma)
                jobs.append((idx, (L if luma else []) + ([pin] if pin is not None else [])))
            jobs = [j for j in jobs if j[1]]
            tag = "bs%d %s" % (bs, "Y" if luma else "C")
            for gi, gg in enumerate(_rows(jobs, 6)):
                scenes.append(inner_scene("E inner %s #%d" % (tag, gi), [g for _, g in gg], bs, luma, [i for i, _ in gg]))
                if bs < 3:
                    scenes.append(left_scene("E left %s #%d" % (tag, gi), [g for _, g in gg], bs, luma, [_avg_pair(i, i & 1) for i, _ in gg]))
                if bs == 1:
                    scenes.append(top_scene("E top %s #%d" % (tag, gi), [g for _, g in gg], bs, luma, [_avg_pair(i, not i & 1) for i, _ in gg]))
            if bs == 2:                                    # the top edge under bS 2: one line a macroblock
                pins = [(i, g[-1]) for i, g in jobs if tc_pin_spread(i, bs, luma) == 0]
                for gi, gg in enumerate(_rows(pins, 9)):
                    scenes.append(top_scene("E top %s #%d" % (tag, gi), [[g] for _, g in gg], bs, luma, [_avg_pair(i, not i & 1) for i, _ in gg]))
    # the tc0 entries of the lowest indices, where only a beta from further up the table lets |delta| exceed t: alpha_c0_offset -12,
    # beta_offset +12, QP = index + 12
    for bs in (1, 2, 3):
        for luma in (True, False):
            pins = [(i, table_lines(i, bs, luma, MAX_SPREAD)[1]) for i in IDX if tc_pin_spread(i, bs, luma) == MAX_SPREAD]
            if not pins:
                continue
            tag = "bs%d %s wide beta" % (bs, "Y" if luma else "C")
            kw = dict(ao=-12, bo=12)
            scenes.append(inner_scene("E inner " + tag, [[g] for _, g in pins], bs, luma, [i + 12 for i, _ in pins], **kw))
            if bs < 3:
                scenes.append(left_scene("E left " + tag, [[g] for _, g in pins], bs, luma, [_avg_pair(i + 12, i & 1) for i, _ in pins], **kw))
                scenes.append(top_scene("E top " + tag, [[g] for _, g in pins], bs, luma, [_avg_pair(i + 12, not i & 1) for i, _ in pins], **kw))
    # qp + offset beyond both ends of the tables
    for name, qp, ao, bo in (("A<0", 5, -12, 12), ("A>51", 45, 12, 0), ("B<0", 5, 12, -12), ("B>51", 45, 0, 12)):
        scenes.append(inner_scene("E clamp " + name, [[fit(3), fit(-2, ep1=1)]], 3, True, [qp], ao=ao, bo=bo))
    return scenes


# ---- family F: which QP goes with which edge -------------------------------------------------------------------------------------------
F_OFFSET = 12                                # index = QP + 12: the triples below reach 51, 46 and 40, whose tc0 lie 3 and more apart
F_CONFIGS = {"inner max, top min": (39, 29, 17), "left max, inner min": (28, 50, 40), "top max, inner min": (28, 40, 50), "left min": (39, 17, 29)}


def family_f():
    """2 x 2, the subject at (1, 1): QPs (own, left, top) whose own, left-averaged and top-averaged indices are 51 / 46 / 40 in four
    orders, Cb one and Cr two below.  Lines on a left, a top and an inner edge that sit between the class's own alpha (beta) and the
    others', and clipped lines that show the class's tc0."""
    scenes = []
    for cname, (qo, ql, qt) in F_CONFIGS.items():
        for variant in ("edges", "inner"):
            s = Scene("F %s, %s" % (cname, variant), 2, 2, kind="F" if variant == "edges" else "V", ao=F_OFFSET, bo=F_OFFSET)
            k = 3
            for kk, q in ((0, 30), (1, qt), (2, ql), (3, qo)):
                s.qp_y[kk], s.qp_c[kk] = q, (q - 1, q - 2)
            if variant == "edges":
                s.ref[k] = 1
            for p in range(3):
                own = s.qp_y[k] - p
                avg = {0: own, 1: (own + ql - p + 1) >> 1, 2: (own + qt - p + 1) >> 1}
                al = {c: int(ALPHA[tab(avg[c] + F_OFFSET)]) for c in avg}
                be = {c: int(BETA[tab(avg[c] + F_OFFSET)]) for c in avg}
                for c in ((1, 2) if variant == "edges" else (0,)):
                    amin, bmin = min(al.values()), min(be.values())
                    L = [fit(al[c] - 1), fit(-al[c]), fit(4, ep1=be[c] - 1), fit(-4, eq1=be[c]),
                         fit(amin - 1, ep2=bmin - 1 if p == 0 else None), fit(-(amin - 1))]
                    for i, l in enumerate(L):
                        if c == 0:
                            s.put(p, 1, 1, 0, 2, i if p == 0 else i % 8, l)
                        elif c == 1:
                            s.put(p, 1, 1, 0, 0, i if p == 0 else 2 + i, l)
                        else:                                # (where the two sets of lines cross they share only q2, q3)
                            s.put(p, 1, 1, 1, 0, (3 + i) if p == 0 else 2 + i, l)
            scenes.append(s)
    return scenes


# ---- family G: the reference's stale tc0 ------------------------------------------------------------------------------------------------
def family_g():
    scenes = []

    def chroma_steps(s, dir_):
        for p in (1, 2):
            for y in range(s.mb_h):
                for i in range(8):
                    s.put(p, 0, y, dir_, 2, i, fit(24 if (i + p) & 1 else -24))
    for name, kind, qc in (("intra", "I", (30, 40)), ("intra, Cr off", "I", (30, 10)), ("inter", "Q", (35, 45))):
        for dir_ in (1, 0):
            s = Scene("G %s dir%d" % (name, dir_), 1, 2, kind=kind, qp=34)
            s.qp_c[:] = qc
            chroma_steps(s, dir_)
            for p in (1, 2):                        # every other edge sees samples that do not change along its line
                a = s.plane(p)
                a[:] = a[:, :1] if dir_ == 1 else a[:1, :]
            scenes.append(s)
    return scenes


# ---- family H: the scalar short cuts of deblock_phase ----------------------------------------------------------------------------------
H_PATTERNS = {False: [(0, (2,)), (0, ()), (0, (1,)), (1, ()), (0, (3,)), (1, (1,)), (1, (2,)), (1, (3,))], True: [(0, (2,)), (0, ()), (1, ()), (1, (2,))]}


def _stepped(n, seed):
    """n samples, a step of 3..6 at every fourth, small ripples between: every gate of a QP near 40 is open across every edge"""
    rng = np.random.default_rng(seed)
    v = 90 + np.cumsum(np.where(np.arange(n) % 4 == 0, rng.integers(3, 7, n) * rng.choice([-1, 1], n), 0)) + rng.integers(-1, 2, n)
    return np.clip(v, 0, 255).astype(np.uint8)


def _oriented(s, dir_, seed):
    """content that does not change along the edges of direction dir_ (so a vector of one sample along them predicts the same), stepped
    across them"""
    for p in range(3):
        a = s.plane(p)
        v = _stepped(a.shape[1 - dir_] if dir_ == 0 else a.shape[0], seed + p)
        a[:] = v[None, :] if dir_ == 0 else v[:, None]


def h_pattern_scene(dir_, t8):
    """one row (dir 0) / column (dir 1) of macroblocks, each with exactly the edges of H_PATTERNS live: sixteen 4x4 partitions (four
    8x8 under the 8x8 transform) whose vectors differ by 4 quarter samples ALONG the edge between the block columns (rows) the edge
    separates, nowhere else"""
    pats = H_PATTERNS[t8]
    n = len(pats)
    s = Scene("H dir%d %s live edges" % (dir_, "8x8" if t8 else "4x4"), n if dir_ == 0 else 1, 1 if dir_ == 0 else n, kind="X", qp=40)
    _oriented(s, dir_, 100 + dir_)
    prev = 0
    for k, (e0, inner) in enumerate(pats):
        lev = prev ^ (4 if (e0 and k) else 0)
        levels = []
        for e in range(4):
            if e in inner:
                lev ^= 4
            levels.append(lev)
        prev = lev
        s.t8[k] = t8
        for b in range(16):
            bx, by = b & 3, b >> 2
            s.mv[k][b][1 - dir_] = levels[bx if dir_ == 0 else by]
    return s


def h_mixed_scene(dir_):
    """inner edge 2 with the strengths 0 1 2 0 over its four segments, and the three rotations: 1 by a vector along the edge in the
    two blocks behind it, 2 by a coefficient in the block behind it"""
    s = Scene("H dir%d mixed strengths" % dir_, 4 if dir_ == 0 else 1, 1 if dir_ == 0 else 4, kind="X", qp=40)
    _oriented(s, dir_, 200 + dir_)
    for k in range(4):
        for seg in range(4):
            want = [0, 1, 2, 0][(seg + k) % 4]
            for c in (2, 3):
                b = (seg * 4 + c) if dir_ == 0 else (c * 4 + seg)
                s.mv[k][b][1 - dir_] = 4 if want == 1 else 0
            if want == 2:
                s.nz.append((k, 2, seg) if dir_ == 0 else (k, seg, 2))
    return s


def family_h():
    scenes = [h_pattern_scene(d, t8) for d in (0, 1) for t8 in (False, True)] + [h_mixed_scene(d) for d in (0, 1)]
    rng = np.random.default_rng(300)
    for name, kinds in (("inter beside intra", "IVIH"), ("IPCM beside SKIP", "SISI")):
        s = Scene("H " + name, 2, 2, qp=38)
        s.kind = list(kinds)
        s.Y[:], s.U[:], s.V[:] = (D.content_smooth_steps(rng, *s.plane(p).shape) for p in range(3))
        scenes.append(s)
    return scenes


# ---- family I: order - lines that read what an earlier filter wrote -------------------------------------------------------------------
I_SIZES = ((1, 4), (2, 3), (3, 4), (3, 3))


def family_i():
    """all-IPCM pictures (bS 4 on every macroblock edge, 3 inside) of smooth stepped content at QPs where most gates are open: every
    filter's input has been written by another.  Which line depends on which earlier filter is measured from the trace (order_cells)."""
    scenes = []
    for (w, h) in I_SIZES:
        for seed in range(3):
            rng = np.random.default_rng(400 + 10 * w + h + 100 * seed)
            s = Scene("I %dx%d #%d" % (w, h, seed), w, h, kind="I")
            s.qp_y[:] = rng.integers(30, 46, w * h)
            s.qp_c[:] = rng.integers(30, 46, (w * h, 2))
            for p in range(3):
                a = s.plane(p)
                y, x = np.mgrid[0:a.shape[0], 0:a.shape[1]]
                a[:] = np.clip(int(rng.integers(70, 170)) + rng.integers(-2, 3, a.shape) + rng.integers(2, 7) * ((x // 4) % 3) + rng.integers(2, 7) * ((y // 4) % 3), 0, 255)
            scenes.append(s)
    return scenes


# ---- family J: slices -------------------------------------------------------------------------------------------------------------------
def family_j():
    scenes = []
    rng = np.random.default_rng(500)
    for where, first in (("row", 6), ("mid", 7)):
        for name, par in (("idc1 above idc0", [dict(ao=0, bo=0, idc=1), dict(ao=0, bo=0, idc=0)]),
                          ("idc0 above idc1", [dict(ao=0, bo=0, idc=0), dict(ao=0, bo=0, idc=1)]),
                          ("offsets", [dict(ao=12, bo=-12, idc=0), dict(ao=-12, bo=12, idc=0)]),
                          ("idc2", [dict(ao=0, bo=0, idc=2), dict(ao=0, bo=0, idc=2)])):
            s = Scene("J %s, %s" % (name, where), 3, 4, kind="I", qp=30 if name == "offsets" else 38, n_slices=2)
            s.first_mb, s.slice_par = [0, first], par
            s.Y[:], s.U[:], s.V[:] = (D.content_smooth_steps(rng, *s.plane(p).shape) for p in range(3))
            if name == "offsets":            # across the border: open under the lower slice's (alpha 5, beta 14), shut under the upper's (101, 2)
                for x in range(3):
                    for i in range(16):
                        s.put(0, x, 2, 1, 0, i, fit(3 if i & 1 else -3, ep1=5, eq1=-4))
                for i in range(16):
                    s.put(0, 1, 2, 0, 0, i, fit(3 if i & 1 else -3, ep1=5, eq1=-4))
            scenes.append(s)
    return scenes


def families():
    """family -> [Scene]"""
    return {"ABCD": family_abcd(), "E": family_e(), "F": family_f(), "G": family_g(), "H": family_h(), "I": family_i(), "J": family_j()}


# ---- cells that need the picture around the line: families F-J (and the untraced cases of A, E) -----------------------------------------
def context_cell_names():
    names, unreach = ["A/zero_ab", "E/avg_odd/left", "E/avg_odd/top"], {}
    names += ["F/%s/%s/%s" % (pl, par, c) for pl in ("Y", "Cb", "Cr") for par in ("alpha/on", "alpha/off", "beta/on", "beta/off", "tc") for c in CLS]
    names += ["G/stale", "G/own_when_cr_off", "G/no/cb_vert_inner", "G/no/cb_left", "G/no/cb_top", "G/no/cr", "G/no/inter"]
    for n in ("G/no/cb_left", "G/no/cb_top"):
        unreach[n] = "the rule needs an intra macroblock, whose own macroblock edges carry bS 4: no tc0 is used there"
    for d in "vh":
        names += ["H/%s/4x4/%s" % (d, p) for p in ("none", "e0", "e1", "e2", "e3", "e0+e1", "e0+e2", "e0+e3")]
        names += ["H/%s/8x8/%s" % (d, p) for p in ("none", "e0", "e2", "e0+e2")]
        names += ["H/%s/e1_not_e2" % d, "H/%s/e2_not_e1" % d] + ["H/%s/mixed/rot%d" % (d, r) for r in range(4)]
    names += ["H/inter_beside_intra", "H/ipcm_beside_skip"]
    for c in ORDER_CELLS:
        names.append("I/" + c)
        for pos, ok in (("firstcol", c not in ("left_e3_for_e0",)), ("lastcol", c not in ("right_e0_for_top_below", "corner3")),
                        ("lastrow", c != "corner3"), ("w1", c not in ("left_e3_for_e0", "right_e0_for_top_below", "corner3")), ("w2", True), ("w3", True)):
            n = "I/%s/%s" % (c, pos)
            names.append(n)
            if not ok:
                unreach[n] = "needs a macroblock to the left (right, below) that this position does not have"
    names += ["J/%s/%s" % (c, w) for c in ("idc1_above_idc0", "idc0_above_idc1", "offsets", "idc2") for w in ("row", "mid")]
    return names, unreach


ORDER_CELLS = ("prev_edge_row", "prev_edge_col", "vert_for_horiz", "left_e3_for_e0", "top_e3_for_top", "strong_p2q2", "right_e0_for_top_below", "corner3")


def _positions(r, j):
    """plane coordinates (x, y) of sample j (0..7 = p3..q3) of record r"""
    o = j - 4
    return (int(r["x"]) + o, int(r["y"])) if r["dir"] == 0 else (int(r["x"]), int(r["y"]) + o)


def order_cells(f, rec, pre):
    """-> {cell: count}.  Walks the trace keeping, per sample, who wrote it last; a line counts for a cell when an input it reads was
    written by that earlier filter AND, with that one sample put back to its pre-deblock value, the line's decisions or the changes
    it makes come out different."""
    w, h = f.mb_w, f.mb_h
    out = {}
    writer = [dict() for _ in range(3)]          # (x, y) -> (mb, dir, edge, j, bs)
    history = [dict() for _ in range(3)]         # luma (x, y) -> [(mb, value)]
    prel = np.stack([[pre.plane(int(r["plane"]))[_positions(r, j)[::-1]] for j in range(8)] for r in rec]) if len(rec) else np.zeros((0, 8))
    ma = model_of(rec)
    sens = []                                    # [j]: does the line decide or change otherwise with sample j alone at its pre-deblock value?
    for j in range(8):
        alt = rec["before"].astype(np.int64)
        alt[:, j] = prel[:, j] if len(rec) else 0
        mp = model(alt, rec["bs"], rec["alpha"], rec["beta"], rec["tc"], rec["plane"] == 0)
        sens.append((ma["on"] != mp["on"]) | (ma["on"] & ((ma["ap"] != mp["ap"]) | (ma["aq"] != mp["aq"]))) | ((ma["out"] - ma["p"]) != (mp["out"] - mp["p"])).any(1))

    def hit(c, k):
        x, y = k % w, k // w
        for n in [c] + [c + "/" + pos for pos, ok in (("firstcol", x == 0), ("lastcol", x == w - 1), ("lastrow", y == h - 1), ("w%d" % w, w <= 3)) if ok]:
            out[n] = out.get(n, 0) + 1
    for i, r in enumerate(rec):
        p, k = int(r["plane"]), int(r["mb"])
        for j in range(8):
            pos = _positions(r, j)
            wr = writer[p].get(pos)
            if wr is None or r["before"][j] == prel[i][j] or not sens[j][i]:
                continue
            wk, wd, we, wj, wb = wr
            if wk == k and wd == r["dir"] and we == r["edge"] - 1:
                hit("prev_edge_row" if wd == 0 else "prev_edge_col", k)
            if r["dir"] == 1 and wd == 0:
                hit("vert_for_horiz", k)
            if r["dir"] == 0 and r["edge"] == 0 and wk == k - 1 and wd == 0 and we == 3:
                hit("left_e3_for_e0", k)
            if r["dir"] == 1 and r["edge"] == 0 and wk == k - w and wd == 1 and we == 3:
                hit("top_e3_for_top", k)
            if wb == 4 and wj in (1, 6):
                hit("strong_p2q2", k)
            if r["dir"] == 1 and r["edge"] == 0 and wk == k - w + 1 and wd == 0 and we == 0 and (k % w) < w - 1:
                hit("right_e0_for_top_below", k)
        for j in range(8):
            if r["after"][j] != r["before"][j]:
                pos = _positions(r, j)
                writer[p][pos] = (k, int(r["dir"]), int(r["edge"]), j, int(r["bs"]))
                if p == 0:
                    history[0].setdefault(pos, []).append((k, int(r["after"][j])))
    for (x, y), hs in history[0].items():
        k = (y // 16) * w + x // 16
        if x % 16 >= 13 and y % 16 >= 13 and x // 16 < w - 1 and y // 16 < h - 1:
            val = {}
            for wk, v in hs:
                val[wk] = v
            if all(q in val for q in (k, k + 1, k + w)) and len({val[k], val[k + 1], val[k + w]}) == 3:
                hit("corner3", k)
    return out


def context_cells(scene, f, rec, pre):
    """-> {cell: count} for the cells of context_cell_names"""
    out = {}

    def add(n, c):
        c = int(c)
        if c:
            out[n] = out.get(n, 0) + c
    w = f.mb_w
    mbs, sl = f.mbs, f.slices
    intra = mbs["mb_type"] == IPCM
    sid = mbs["slice_id"].astype(int)
    ao, bo, idc = sl["alpha_c0_offset"][sid].astype(int), sl["beta_offset"][sid].astype(int), sl["deblock_idc"][sid]
    fam = scene.name.split()[0]
    k = rec["mb"].astype(int)
    luma, cls, pl = rec["plane"] == 0, edge_class(rec), rec["plane"].astype(int)
    nb = np.where(cls == 1, k - 1, np.where(cls == 2, k - w, k))
    m = model_of(rec)
    changed = (m["out"] != m["p"]).any(1)
    # A: an intra macroblock whose inner alpha and beta are both 0 hands nothing to the filters
    for kk in range(len(mbs)):
        if intra[kk] and idc[kk] != 1 and mbs["qp_y"][kk] + ao[kk] < 16 and mbs["qp_y"][kk] + bo[kk] < 16:
            add("A/zero_ab", not ((k == kk) & (rec["edge"] > 0) & luma).any())
    odd = ((mbs["qp_y"][k].astype(int) + mbs["qp_y"][nb]) & 1) == 1
    add("E/avg_odd/left", (luma & (cls == 1) & odd & changed).sum())
    add("E/avg_odd/top", (luma & (cls == 2) & odd & changed).sum())
    qpl = np.where(pl == 0, mbs["qp_y"][k], mbs["qp_c"][k, np.maximum(pl - 1, 0)]).astype(int)

    def q_of(kk, p):
        return np.where(p == 0, mbs["qp_y"][kk], mbs["qp_c"][kk, np.maximum(p - 1, 0)]).astype(int)
    if fam == "F" and len(rec):
        has = (k % w > 0) & (k >= w)
        kl, kt = np.maximum(k - 1, 0), np.maximum(k - w, 0)
        qs = [qpl, (qpl + q_of(kl, pl) + 1) >> 1, (qpl + q_of(kt, pl) + 1) >> 1]
        distinct = has & (qs[0] != qs[1]) & (qs[0] != qs[2]) & (qs[1] != qs[2])
        al = [ALPHA[tab(q + ao[k])] for q in qs]
        be = [BETA[tab(q + bo[k])] for q in qs]
        tc = [tc_of(q + ao[k], rec["bs"], luma) for q in qs]
        for ci, c in enumerate(CLS):
            o1, o2 = [o for o in range(3) if o != ci]
            sel = distinct & (cls == ci)
            for par, arrs in (("alpha", al), ("beta", be), ("tc", tc)):
                alts = []
                for o in (o1, o2):
                    a_, b_, t_ = (arrs[o] if par == "alpha" else rec["alpha"]), (arrs[o] if par == "beta" else rec["beta"]), (arrs[o] if par == "tc" else rec["tc"])
                    alts.append(model(rec["before"], rec["bs"], a_, b_, t_, luma))
                d1, d2 = ((a_["out"] != m["out"]).any(1) for a_ in alts)
                for p, pn in enumerate(("Y", "Cb", "Cr")):
                    s2 = sel & (pl == p) & d1 & d2
                    if par == "tc":
                        add("F/%s/tc/%s" % (pn, c), (s2 & (rec["bs"] < 4) & (np.abs(tc[o1] - rec["tc"]) >= 2) & (np.abs(tc[o2] - rec["tc"]) >= 2)).sum())
                    else:
                        add("F/%s/%s/on/%s" % (pn, par, c), (s2 & m["on"] & ~alts[0]["on"] & ~alts[1]["on"]).sum())
                        add("F/%s/%s/off/%s" % (pn, par, c), (s2 & ~m["on"] & alts[0]["on"] & alts[1]["on"]).sum())
    if fam == "G" and len(rec):
        qc = mbs["qp_c"][k].astype(int)
        differ = qc[:, 0] != qc[:, 1]
        other = np.where(pl == 1, qc[:, 1], qc[:, 0]) + ao[k]           # the other chroma plane's indexA (inner edges)
        tc_other = tc_of(other, rec["bs"], False)
        cr_on = (ALPHA[tab(qc[:, 1] + ao[k])] | BETA[tab(qc[:, 1] + bo[k])]) != 0
        clipped = m["lt"] & (np.abs(m["raw"]) > np.maximum(rec["tc"], tc_other))
        tc_own = tc_of(rec["idx_a"].astype(int), rec["bs"], False)
        inner_h, inner_v = (rec["dir"] == 1) & (rec["edge"] == 2), (rec["dir"] == 0) & (rec["edge"] == 2)
        base = differ & clipped
        add("G/stale", (base & intra[k] & (pl == 1) & inner_h & (rec["idx_tc"] != rec["idx_a"]) & (tc_own != rec["tc"])).sum())
        add("G/own_when_cr_off", (differ & m["lt"] & (np.abs(m["raw"]) > rec["tc"]) & intra[k] & (pl == 1) & inner_h & ~cr_on & (rec["idx_tc"] == rec["idx_a"]) & (rec["tc"] > 1)).sum())
        same = (rec["idx_tc"] == rec["idx_a"]) & (tc_other != rec["tc"]) & cr_on
        add("G/no/cb_vert_inner", (base & intra[k] & (pl == 1) & inner_v & same).sum())
        add("G/no/cr", (base & intra[k] & (pl == 2) & inner_h & same).sum())
        add("G/no/inter", (base & ~intra[k] & (pl == 1) & inner_h & same).sum())
    if fam == "H":
        t8 = (mbs["flags"] & 1) != 0
        for d, dn in ((0, "v"), (1, "h")):
            live = np.zeros((len(mbs), 4), bool)
            for e in range(4):
                s_ = luma & (rec["dir"] == d) & (rec["edge"] == e) & (rec["bs"] > 0)
                live[np.unique(k[s_]), e] = True
            step = 1 if d == 0 else w
            for kk in range(len(mbs)):
                if scene.kind[kk] != "X":
                    continue
                name = "+".join("e%d" % e for e in range(4) if live[kk, e]) or "none"
                if name == "none":
                    x, y = kk % w, kk // w
                    ok = (0 < x < w - 1) if d == 0 else (0 < y < f.mb_h - 1)
                    if not (ok and live[kk - step].any() and live[kk + step].any()):
                        continue
                if "mixed" not in scene.name:
                    add("H/%s/%s/%s" % (dn, "8x8" if t8[kk] else "4x4", name), 1)
                # the chroma edge at sample 4 lies on luma edge 2: with luma edge 1 live and edge 2 dead it must stay as it is
                cp = pre.plane(1)
                x0, y0 = 8 * (kk % w), 8 * (kk // w)
                stepc = (cp[y0:y0 + 8, x0 + 3] != cp[y0:y0 + 8, x0 + 4]).any() if d == 0 else (cp[y0 + 3, x0:x0 + 8] != cp[y0 + 4, x0:x0 + 8]).any()
                if stepc and live[kk, 1] and not live[kk, 2]:
                    add("H/%s/e1_not_e2" % dn, 1)
                if stepc and live[kk, 2] and not live[kk, 1] and ((k == kk) & (pl > 0) & (rec["dir"] == d) & (rec["edge"] == 2) & changed).any():
                    add("H/%s/e2_not_e1" % dn, 1)
                for e in (1, 2, 3):
                    s_ = np.nonzero(luma & (rec["dir"] == d) & (rec["edge"] == e) & (k == kk))[0]
                    if len(s_) == 16:
                        segs = [int(rec["bs"][s_[4 * g]]) for g in range(4)]
                        for r_ in range(4):
                            if segs == [[0, 1, 2, 0][(g + r_) % 4] for g in range(4)]:
                                add("H/%s/mixed/rot%d" % (dn, r_), 1)
        inter = ~intra
        e0_4 = set(np.unique(k[(rec["edge"] == 0) & (rec["bs"] == 4) & inter[k] & changed]))
        in_le2 = set(np.unique(k[(rec["edge"] > 0) & (rec["bs"] > 0) & (rec["bs"] <= 2) & inter[k] & changed]))
        add("H/inter_beside_intra", len(e0_4 & in_le2))
        add("H/ipcm_beside_skip", ((rec["edge"] == 0) & intra[k] & (mbs["mb_type"][nb] == SKIP) & changed).sum())
    if fam == "I":
        for n, c in order_cells(f, rec, pre).items():
            add("I/" + n, c)
    if fam == "J":
        where = "mid" if scene.name.endswith("mid") else "row"
        cross = (sid[k] != sid[nb]) & (rec["edge"] == 0)
        border = [kk for kk in range(len(mbs)) if sid[kk] == 1 and ((kk >= w and sid[kk - w] == 0) or (kk % w and sid[kk - 1] == 0))]
        if "idc1 above idc0" in scene.name:
            add("J/idc1_above_idc0/" + where, (cross & (m["out"][:, :4] != m["p"][:, :4]).any(1) & (idc[nb] == 1)).sum())
        if "idc0 above idc1" in scene.name:
            add("J/idc0_above_idc1/" + where, len(border) if not (sid[k] == 1).any() and (sid[k] == 0).any() else 0)
        if "idc2" in scene.name:
            add("J/idc2/" + where, len(border) if not cross.any() and (sid[k] == 1).any() else 0)
        if "offsets" in scene.name:
            qa = (q_of(k, pl) + q_of(nb, pl) + 1) >> 1
            alt = model(rec["before"], rec["bs"], ALPHA[tab(qa + ao[nb])], BETA[tab(qa + bo[nb])], tc_of(qa + ao[nb], rec["bs"], luma), luma)
            add("J/offsets/" + where, (cross & (rec["idx_a"] == qa + ao[k]) & m["on"] & changed & (alt["out"] != m["out"]).any(1)).sum())
    return out


def cells(scene, f, rec, pre):
    """every cell of A-J this picture's trace reaches -> {name: count}"""
    out = {n: int(v.sum()) for n, v in line_cells(rec).items() if v.any()}
    for n, c in context_cells(scene, f, rec, pre).items():
        out[n] = out.get(n, 0) + c
    return out


def all_cell_names():
    a, ua = line_cell_names()
    b, ub = context_cell_names()
    ua = dict(ua)
    ua["D/lt4/tc0_0/inside"] = "with tc0 = 0 a chroma line's t is 1: no nonzero delta is smaller"
    ua.update(ub)
    return a + b, ua


# ---- running a scene through the oracle -----------------------------------------------------------------------------------------------
def run_oracle(frames, trace=True):
    """-> (pictures, pre-deblock pictures, trace records of the last picture)"""
    pics, pre, rec = {}, [], None
    for f in frames:
        refs = [pics[r] for r in f.ref_ids]
        a = O.HostPic(f.mb_w, f.mb_h)
        O.recon_frame(f.mbs, f.coeffs, f.slices, a, refs, O.NO_DEBLOCK | O.NO_EXPAND)
        pre.append(a)
        dst = O.HostPic(f.mb_w, f.mb_h)
        if trace:
            rec = O.recon_frame_traced(f.mbs, f.coeffs, f.slices, dst, refs, 0)
        else:
            O.recon_frame(f.mbs, f.coeffs, f.slices, dst, refs, 0)
        pics[f.id] = dst
    return [pics[f.id] for f in frames], pre, rec
