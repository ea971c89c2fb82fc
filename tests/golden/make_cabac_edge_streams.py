#!/usr/bin/env python3
"""The CABAC syntax-edge streams of tests/golden/cabac_edge/ and the reference's verdict on them, tests/golden/cabac_edge_ref.json.

build() writes every stream with tests/h264_synth_cabac.py (pure Python, deterministic) and returns {name: (bytes, counters)}; the
counters carry under "written" what the writer put into every macroblock of a CABAC slice, per picture, for the tests that compare it
with what the front end reads back.  main() is make_edge_streams.main() over these streams: the unmodified reference
(oracle/_ref/h264dec), once per stream on the CPU, compress and decode, then restore.  Only streams and records are committed.
"""
import copy
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import h264_synth_cabac as K  # noqa: E402
import make_edge_streams as M  # noqa: E402

EDGE_DIR = os.path.join(HERE, "cabac_edge")
MAXN = {0: 16, 1: 15, 2: 16, 3: 4, 4: 15, 5: 64}
CARRY_SEED = 49                                                  # set by the search of carry_search(), see cabac_carry()


class Joined:
    """streams behind each other (each with its own parameter sets and IDR picture) as one; the counters merged"""

    def __init__(self, parts):
        self.parts = parts
        self.n = parts[0].n
        self.count = copy.deepcopy(parts[0].count)
        self.written = list(parts[0].written)
        for p in parts[1:]:
            self.written += p.written
            for k, v in p.count.items():
                c = self.count
                if isinstance(v, set):
                    c[k] |= v
                elif k in ("pictures", "epb", "epb_arith"):
                    c[k] += v
                elif k.endswith("_min"):
                    c[k] = min(c[k], v)
                elif k.endswith("_max"):
                    c[k] = max(c[k], v)
                elif k in ("skip_inc", "cbf_inc", "abs_level", "t8_inc"):
                    for a, b in v.items():
                        c[k][a] = c[k].get(a, 0) + b

    def bytes(self):
        return b"".join(p.bytes() for p in self.parts)


def _blank_idr(S, qp=26):
    S.picture([dict(first_mb=0, type="I", qp=qp, pps=1, mbs=[K.i16()] * S.n)], idr=True)


def _one(v, n=16, at=0):
    return [0] * at + [v] + [0] * (n - at - 1)


# ---- levels ------------------------------------------------------------------------------------------------------------------------
def level_values():
    """coeff_abs_level_minus1: around the TU prefix's cMax 14 (the UEG0 joint) and around every power of two of the Exp-Golomb suffix,
    up to what int16 levels (those of levels_ext) hold: 32766 for +-32767, 32767 for -32768 alone"""
    v = {0, 1, 12, 13, 14, 15, 16}
    for k in range(15):
        v |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    return sorted(v | {32766, 32767})


def level_blocks(cat):
    """blocks of ctxBlockCat `cat`: every value with both signs, then a full block of ones, then a full block of levels above 1"""
    n = MAXN[cat]
    seq = []
    for v in level_values():
        seq += [v + 1, -(v + 1)] if v < 32767 else [-(v + 1)]
    blocks = [seq[i:i + n] + [0] * (n - len(seq[i:i + n])) for i in range(0, len(seq), n)]
    blocks.append([(1, -1)[i % 2] for i in range(n)])
    blocks.append([(2, -3, 5)[i % 3] for i in range(n)])
    return blocks


def cabac_levels():
    """8x2, one slice a picture: an I picture of I16x16 macroblocks (ctxBlockCat 0, 1, 3, 4) and a P picture (2, 5, 3, 4)"""
    S = K.CabacSynth(8, 2)
    b = {c: level_blocks(c) for c in range(6)}
    imbs, pmbs = [], []
    for j in range(S.n):
        dc = b[0][j] if j < len(b[0]) else _one(j - 7)
        ac = {i: b[1][16 * j + i] for i in range(16) if 16 * j + i < len(b[1])}
        cdc = [b[3][2 * j + i] if 2 * j + i < len(b[3]) else [0] * 4 for i in range(2)]
        cac = {(i >> 2, i & 3): b[4][8 * j + i] for i in range(8) if 8 * j + i < len(b[4])}
        imbs.append(K.i16(cbp_l=15 if ac else 0, cbp_c=2 if cac else 1, dc=dc, ac=ac, cdc=cdc, cac=cac))
        rev = len(b[3]) - 1 - 2 * j                              # the P picture takes the chroma blocks from the other end
        pc = dict(cbp_c=2 if cac else 1, cdc=[b[3][rev - i] if rev - i >= 0 else [0] * 4 for i in range(2)], cac=cac)
        if j == 0:
            pmbs.append(K.p16(mvd=(1, -1), cbp_l=15, luma={i: b[2][i] for i in range(min(16, len(b[2])))}, **pc))
        elif j == 1:
            assert len(b[5]) <= 4 and len(b[2]) <= 16
            pmbs.append(K.p16(t8=1, cbp_l=(1 << len(b[5])) - 1, luma8=dict(enumerate(b[5])), **pc))
        else:
            pmbs.append(K.p16(mvd=(j % 3, 0), cbp_l=1, luma={0: _one(j)}, **pc))
    S.picture([dict(first_mb=0, type="I", qp=4, pps=1, mbs=imbs)], idr=True)
    S.picture([dict(first_mb=0, type="P", qp=2, pps=1, init_idc=1, mbs=pmbs)])
    return S


# ---- significance maps -------------------------------------------------------------------------------------------------------------
def sig_blocks(cat):
    """one block per position with that single coefficient, a full block, an all-zero block (ctxBlockCat 5 has none: no flag)"""
    n = MAXN[cat]
    out = [_one((2, -1, 1, -3)[i % 4], n, i) for i in range(n)] + [[(1, -2)[i % 2] for i in range(n)]]
    return out + ([[0] * n] if cat != 5 else [])


def cabac_sigmap():
    """5x4: an I picture (ctxBlockCat 0, 1, 3, 4) and a P picture (2, 5, 3, 4), one slice each"""
    S = K.CabacSynth(5, 4)
    b = {c: sig_blocks(c) for c in range(6)}
    imbs, pmbs = [], []
    for j in range(S.n):
        ac = {i: b[1][16 * j + i] for i in range(16) if 16 * j + i < len(b[1])}
        cdc = [b[3][2 * j + i] if 2 * j + i < len(b[3]) else [0] * 4 for i in range(2)]
        cac = {(i >> 2, i & 3): b[4][8 * j + i] for i in range(8) if 8 * j + i < len(b[4])}
        imbs.append(K.i16(cbp_l=15 if ac else 0, cbp_c=2 if cac else 1, dc=b[0][j] if j < len(b[0]) else [0] * 16, ac=ac, cdc=cdc, cac=cac))
        pc = dict(cbp_c=2 if cac else 1, cdc=cdc[::-1], cac=cac)
        if j < 2:
            pmbs.append(K.p16(mvd=(0, 1), cbp_l=15, luma={i: b[2][16 * j + i] for i in range(16) if 16 * j + i < len(b[2])}, **pc))
        elif 4 * (j - 2) < len(b[5]):
            blocks = b[5][4 * (j - 2):4 * (j - 2) + 4]
            pmbs.append(K.p16(t8=1, cbp_l=(1 << len(blocks)) - 1, luma8=dict(enumerate(blocks)), **pc))
        else:
            pmbs.append(K.skip(1))
    S.picture([dict(first_mb=0, type="I", qp=30, pps=1, mbs=imbs)], idr=True)
    S.picture([dict(first_mb=0, type="P", qp=28, pps=1, init_idc=2, mbs=pmbs)])
    return S


# ---- mvd ---------------------------------------------------------------------------------------------------------------------------
def cabac_mvd():
    """two rows.  Picture 1: the row of mvd_edges (+v then -v, both components; the prefix's cMax 9 between 8 and 9) over a skipped row.
    Picture 2: the lower row's macroblocks have |mvd| 1 and see above them 1, 2, 31, 32: neighbour sums 2, 3, 32, 33"""
    vals = M.mvd_values()
    S = K.CabacSynth(2 * len(vals), 2)
    w = S.mb_w
    S.picture([dict(first_mb=0, type="I", qp=26, pps=1, mbs=[K.i16(dc=[(7 * k) % 41 - 20, (3 * k) % 7 - 3] + [0] * 14) for k in range(S.n)])], idr=True)
    mbs = []
    for v in vals:
        mbs += [K.p16(mvd=(v, v)), K.p16(mvd=(-v, -v))]
    S.picture([dict(first_mb=0, type="P", qp=26, pps=1, init_idc=0, mbs=mbs + [K.skip(w)])])
    up = [5, 1, 2, 31, 32]
    top = [K.p16(mvd=(u, -u)) for u in up] + [K.p16(mvd=(-u, u)) for u in up[::-1]] + [K.skip(w - 10)]
    low = [K.p16(mvd=(-1, 1), cbp_l=1, luma={0: _one(1 + x)}) for x in range(5)] + [K.skip(w - 5)]
    S.picture([dict(first_mb=0, type="P", qp=26, pps=1, init_idc=1, mbs=top + low)])
    return S


# ---- qp ----------------------------------------------------------------------------------------------------------------------------
def cabac_qp():
    """4x4: the jumps of qp_edges in an I and a P picture; in the P picture a delta behind a skipped macroblock, an I_PCM and a P
    macroblock without residual; then SliceQPY 0 and 51 in I slices and in P slices of every cabac_init_idc"""
    S = K.CabacSynth(4, 4)
    dq = [0] + [1] * 10 + [1, -26, 25, 25, -26]
    S.picture([dict(first_mb=0, type="I", qp=41, pps=1,
                    mbs=[K.i16(cbp_l=15, cbp_c=1, dqp=d, dc=[3 * (k % 5) - 6, 1] + [0] * 14, ac={5: [1] + [0] * 14}, cdc=[[k % 3 - 1, 0, 0, 0], [1, 0, 0, 0]])
                         for k, d in enumerate(dq)])], idr=True)

    def coded(k, d):
        return K.p16(mvd=(k, -k), cbp_l=1, dqp=d, luma={0: _one(k - 4 or 1)})
    mbs = [coded(0, 6), coded(1, 1), K.skip(1), coded(2, -26), coded(3, 25), K.pcm([128] * 384), coded(4, 25), K.p16(mvd=(1, 1)), coded(5, -26),
           coded(6, 1), coded(7, 0), coded(8, 2), K.i16(dqp=-3, dc=_one(2)), K.i16(dqp=0), coded(9, 1), K.skip(1)]
    S.picture([dict(first_mb=0, type="P", qp=45, pps=1, init_idc=0, mbs=mbs)])
    S.picture([dict(first_mb=8 * i, type="I", qp=q, pps=1, mbs=[K.i16(cbp_c=1, dc=_one(3 + k), cdc=[[1, 0, 0, 0], [0, -1, 0, 0]]) for k in range(8)])
               for i, q in enumerate((0, 51))])
    sl = []
    for i, (idc, q) in enumerate((i, q) for i in range(3) for q in (0, 51)):
        n = 2 if i < 5 else 6
        sl.append(dict(first_mb=2 * i, type="P", qp=q, pps=1, init_idc=idc,
                       mbs=[K.p16(mvd=(i, k), cbp_l=2, cbp_c=1, luma={4: _one(-2 - k)}, cdc=[[0, 2, 0, 0], [1, 0, 0, 0]]) for k in range(n)]))
    S.picture(sl)
    return S


# ---- ref_idx -----------------------------------------------------------------------------------------------------------------------
def cabac_refidx(pictures):
    """nref() of make_edge_streams with CABAC slices: picture i (2..16) has i active references and uses the highest ref_idx; the
    pattern alternates so that the fourth macroblock sees no, one and two neighbours with ref_idx above 0"""
    S = K.CabacSynth(2, 2, num_ref_frames=16)
    S.picture([dict(first_mb=0, type="I", qp=26, pps=1, mbs=[K.i16(dc=_one(10 * k - 15)) for k in range(4)])], idr=True)
    for i in range(1, pictures):
        nr = None if i == 1 else min(i, 16)
        top = (nr or 1) - 1
        refs = [top, 0, top, top // 2] if i % 2 else [top, top, top, 0]
        S.picture([dict(first_mb=0, type="P", qp=26, pps=1, init_idc=i % 3, num_ref=nr,
                        mbs=[K.p16(ref=r, mvd=(k - 1, 1 - k), cbp_l=1, luma={0: _one(3 + (i + k) % 5)}) for k, r in enumerate(refs)])])
    return S


# ---- skip --------------------------------------------------------------------------------------------------------------------------
def cabac_skip():
    """40x30: a P picture of 1200 skip flags; a P picture in three slices whose flags see no, skipped and coded neighbours.  Behind it a
    1x1 stream whose P slice is one skip flag and the end of the slice: the shortest slice data there is"""
    S = K.CabacSynth(40, 30)
    _blank_idr(S)
    S.picture([dict(first_mb=0, type="P", qp=26, pps=1, init_idc=0, mbs=[K.skip(1200)])])

    def c(k):
        return K.p16(mvd=(k % 3 - 1, 0))
    a = [c(0), c(1), K.skip(38)] + [c(2), K.skip(1), c(3), K.skip(37)] + [K.skip(320)]
    S.picture([dict(first_mb=0, type="P", qp=26, pps=1, init_idc=1, mbs=a),
               dict(first_mb=400, type="P", qp=26, pps=1, init_idc=2, mbs=[K.skip(399), c(4)]),
               dict(first_mb=800, type="P", qp=26, pps=1, init_idc=0, mbs=[c(k) for k in range(80)] + [K.skip(320)])])
    T = K.CabacSynth(1, 1)
    _blank_idr(T)
    T.picture([dict(first_mb=0, type="P", qp=26, pps=1, init_idc=0, mbs=[K.skip(1)])])
    return Joined([S, T])


# ---- I_PCM -------------------------------------------------------------------------------------------------------------------------
def cabac_pcm():
    """4x2: I_PCM as first, last and consecutive macroblocks of an I and a P slice and behind a skip, samples all 0 and all 255; a coded
    macroblock to the right of and below an I_PCM"""
    S = K.CabacSynth(4, 2)
    z, f = K.pcm([0] * 384), K.pcm([255] * 384)

    def ci(k):
        return K.i16(cbp_l=15, cbp_c=2, dc=_one(k + 1), ac={0: _one(1, 15), 5: _one(-1, 15, 3)}, cdc=[[1, 0, 0, 0], [0, 0, 0, 2]], cac={(0, 0): _one(1, 15), (1, 2): _one(1, 15)})

    def cp(k):
        return K.p16(mvd=(k, 1), cbp_l=15, cbp_c=2, luma={0: _one(2), 10: _one(-1)}, cdc=[[1, 0, 0, 0], [0, 0, 0, 2]], cac={(0, 0): _one(1, 15), (1, 2): _one(1, 15)})
    S.picture([dict(first_mb=0, type="I", qp=26, pps=1, mbs=[z, f, ci(0), ci(1), ci(2), ci(3), ci(4), f])], idr=True)
    S.picture([dict(first_mb=0, type="P", qp=26, pps=1, init_idc=0, mbs=[f, cp(0), K.skip(1), z, cp(1), K.skip(1), f, f])])
    S.picture([dict(first_mb=0, type="P", qp=30, pps=1, init_idc=2, mbs=[K.skip(1), z, cp(2), cp(3)]),
               dict(first_mb=4, type="I", qp=22, pps=1, mbs=[ci(5), f, ci(6), ci(7)])])
    return S


# ---- header and stop bit phases ----------------------------------------------------------------------------------------------------
def _phases(l2fn):
    S = K.CabacSynth(4, 2, log2_max_frame_num=l2fn)
    _blank_idr(S)
    for nr in (None, 1, 2):
        for qp in (26, 27, 29, 33, 10):
            for deb in ((0, 0, 0), (1, 0, 0), (2, 1, 0), (0, 2, -3)):
                for lv in range(1, 4):
                    if len(S.count["hdr_phase"]) == 8 and len(S.count["stop_phase"]) == 8:
                        return S
                    T = copy.deepcopy(S)
                    T.picture([dict(first_mb=a, type="P", qp=qp, pps=1, init_idc=(a + lv) % 3, num_ref=nr, deblock=deb,
                                    mbs=[K.p16(mvd=(a, lv), cbp_l=1, luma={0: _one(lv * (a + 1))})] * n) for a, n in ((0, 1), (1, 2), (3, 4), (7, 1))])
                    if len(T.count["hdr_phase"]) + len(T.count["stop_phase"]) > len(S.count["hdr_phase"]) + len(S.count["stop_phase"]):
                        S = T
    return S


def cabac_phase():
    """4x2, four slices a picture (first_mb 0, 1, 3, 7: ue(v) of 1, 3, 5 and 7 bits), with slice_qp_delta, the deblocking fields and
    num_ref_idx_active_override varied until the headers have ended at all eight bit phases and the stop bits too; once with a
    frame_num of 4 bits and once, behind it, with one of 9 bits"""
    return Joined([_phases(4), _phases(9)])


# ---- outstanding bits --------------------------------------------------------------------------------------------------------------
def _lcg(seed):
    x = (seed * 2654435761 + 12345) & 0xffffffff
    while True:
        x = (x * 1664525 + 1013904223) & 0xffffffff
        yield x >> 8


def cabac_carry(seed=None):
    """5x4 P picture.  First sixteen macroblocks of nothing but most probable bins, which leave the low end of the interval at rest:
    zero bytes, and an emulation prevention byte inside the arithmetic-coded data.  Then four bypass-heavy macroblocks, levels and mvd
    whose Exp-Golomb suffixes are a few thousand bypass bins, drawn from a generator whose seed a search on the CPU picked
    (carry_search) for the longest chain of outstanding bits: 9 of them span a whole output byte"""
    r = _lcg(CARRY_SEED if seed is None else seed)
    S = K.CabacSynth(5, 4)
    _blank_idr(S)

    def lv():
        v = next(r) % 16000 + 40
        return -v if next(r) & 1 else v
    mbs = [K.p16(mvd=(lv() // 4, lv() // 4), cbp_l=15, cbp_c=1, luma={i: [lv() if j < 6 else 0 for j in range(16)] for i in range(16)},
                 cdc=[[lv(), lv(), 0, 0], [0, lv(), 0, 0]]) for _ in range(4)]
    S.picture([dict(first_mb=0, type="P", qp=26, pps=1, init_idc=0, mbs=[K.p16()] * 16 + mbs)])
    return S


def carry_search(limit=400):
    best = None
    for seed in range(limit):
        c = cabac_carry(seed).count
        key = (min(c["outstanding_max"], 9) + 9 * min(c["epb_arith"], 1), c["outstanding_max"])
        if best is None or key > best[0]:
            best = (key, seed)
            print("seed", seed, "outstanding_max", c["outstanding_max"], "epb_arith", c["epb_arith"], flush=True)
    return best


# ---- both entropy coders in one stream ---------------------------------------------------------------------------------------------
def cabac_mixed():
    """4x4: PPS 0 (CAVLC) and PPS 1 (CABAC) alternate between pictures, each picture in two or three slices (a change of
    pic_parameter_set_id between two slices begins a new picture, 7.4.1.2.4: one picture cannot hold both); cabac_init_idc differs
    between the slices of one picture; transform_size_8x8_flag on and off beside each other under all three of its increments"""
    S = K.CabacSynth(4, 4)

    def ci(k):
        return K.i16(cbp_c=1, dc=_one(2 * k - 7), cdc=[[k % 3, 0, 0, 0], [0, 1, 0, 0]])

    def cp(k, t8=0):
        if t8:
            return K.p16(t8=1, mvd=(k % 4 - 2, 1), cbp_l=5, luma8={0: _one(2, 64, k), 2: _one(-1, 64, 63 - k)})
        return K.p16(mvd=(k % 4 - 2, 1), cbp_l=5, luma={0: _one(2), 9: _one(-1, 16, k % 16)})
    S.picture([dict(first_mb=0, type="I", qp=28, pps=1, mbs=[ci(k) for k in range(8)]),
               dict(first_mb=8, type="I", qp=24, pps=1, mbs=[ci(k) for k in range(8, 16)])], idr=True)
    t8 = [1, 1, 1, 0, 1, 1, 0, 1]
    S.picture([dict(first_mb=0, type="P", qp=26, pps=0, mbs=[cp(k) for k in range(6)] + [K.skip(2)]),
               dict(first_mb=8, type="P", qp=27, pps=0, mbs=[cp(k) for k in range(8)])])
    S.picture([dict(first_mb=0, type="P", qp=25, pps=1, init_idc=2, mbs=[cp(k, t) for k, t in enumerate(t8)]),
               dict(first_mb=8, type="P", qp=26, pps=1, init_idc=0, mbs=[cp(1), K.skip(1), cp(2, 1), cp(3, 1)]),
               dict(first_mb=12, type="P", qp=26, pps=1, init_idc=1, mbs=[K.skip(1), cp(3), cp(4, 1), K.skip(1)])])
    S.picture([dict(first_mb=0, type="I", qp=26, pps=0, mbs=[ci(k) for k in range(12)]),
               dict(first_mb=12, type="P", qp=26, pps=0, mbs=[cp(k) for k in range(4)])])
    S.picture([dict(first_mb=0, type="P", qp=26, pps=1, init_idc=1, mbs=[cp(k, t) for k, t in enumerate(t8[::-1])]),
               dict(first_mb=8, type="I", qp=30, pps=1, mbs=[ci(k) for k in range(8)])])
    S.picture([dict(first_mb=0, type="P", qp=26, pps=0, mbs=[cp(k) for k in range(16)])])
    return S


BUILDERS = {
    "cabac_levels": cabac_levels,
    "cabac_sigmap": cabac_sigmap,
    "cabac_mvd": cabac_mvd,
    "cabac_qp": cabac_qp,
    "cabac_refidx": lambda: cabac_refidx(16),
    "cabac_refidx16": lambda: cabac_refidx(18),
    "cabac_skip": cabac_skip,
    "cabac_pcm": cabac_pcm,
    "cabac_phase": cabac_phase,
    "cabac_carry": cabac_carry,
    "cabac_mixed": cabac_mixed,
}


def build():
    out = {}
    for name, fn in BUILDERS.items():
        S = fn()
        S.count["mbs"] = S.n
        S.count["written"] = S.written
        out[name] = (S.bytes(), S.count)
    return out


def main(only):
    """only: the streams to write and take the verdict on again (none named: all)"""
    os.makedirs(EDGE_DIR, exist_ok=True)
    streams = build()
    tmp = tempfile.mkdtemp(prefix="lh264_cabac_edge_")
    path = os.path.join(HERE, "cabac_edge_ref.json")
    out = json.load(open(path)) if only and os.path.exists(path) else {}
    for name, (data, count) in streams.items():
        if only and name not in only:
            continue
        open(os.path.join(EDGE_DIR, name + ".264"), "wb").write(data)
        out[name] = M.reference_verdict(name, data, tmp, count["pictures"], count["mbs"], messages=True)
        out[name]["reference_decodes"] = bool(out[name]["compress_rc"] == 0 and out[name]["yuv_bytes"] == sum(len(p) for p in count["written"]) * 384)
        print(name, len(data), "bytes; reference: rc", out[name]["compress_rc"], "decodes", out[name]["reference_decodes"],
              "roundtrip" if out[name]["reference_roundtrip"] else "NO roundtrip", flush=True)
    json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    shutil.rmtree(tmp)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--carry-search"]:
        print(carry_search(int(sys.argv[2]) if len(sys.argv) > 2 else 400))
    else:
        main(sys.argv[1:])
