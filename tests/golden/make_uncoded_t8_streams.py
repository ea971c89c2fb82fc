"""Writes tests/golden/uncoded_t8/: macroblocks that code nothing under the 8x8 transform, on every path (tests/test_uncoded_t8.py,
tests/test_uncoded_t8_gpu.py).  Pictures of 4 x 3 macroblocks; flat neighbours at different levels (I16x16 with a DC coefficient, I_PCM)
and carried QPs of 36..45 (and 0 and 51), so that the in-loop filter moves samples around the macroblocks under test and a wrong QP, a
wrong boundary strength or a skipped edge changes bytes.

  i8_cbp0_cavlc_p       CAVLC, P slices: I_NxN with transform_size_8x8_flag 1 and coded_block_pattern 0 ("i8u") as the first macroblock
                        of a slice, with a left-only and a top-only neighbour, beside I8x8 coded, I4x4, I16x16, I_PCM, P_L0_16x16 with
                        and without the flag and P_Skip, two in a row, as the last macroblock of a slice and of the picture, behind a
                        macroblock whose mb_qp_delta moved the QP away from SliceQPY, in front of one with a non-zero mb_qp_delta, at
                        carried QP 0 and 51, under disable_deblocking_filter_idc 0, 1 and 2
  i8_cbp0_cabac         the same places in CABAC I and P slices
  i8_cbp0_cavlc_i_same  a CAVLC I picture with i8u macroblocks behind an I picture that has, at each of their places, a coded
                        macroblock at exactly the QP carried into the later one
  i8_cbp0_cavlc_i_stale the same two pictures, the earlier one's QP at those places 12 away from the carried one; in front of them a
                        first picture that holds one i8u.  THE ONE STREAM THE REFERENCE DECODES OTHERWISE: its CAVLC reader of I slices
                        (decode_slice.cpp:3328) refreshes a macroblock's entries of pLumaQp / pChromaQp for coded_block_pattern 0 only
                        under IS_INTRA4x4, which an I8x8 macroblock is not, so its filter reads what the picture before left there
  inter_t8_absent_cavlc, inter_t8_absent_cabac
                        under transform_8x8_mode_flag 1: P_L0_16x16, P_L0_L0_16x8 and P_L0_L0_8x16 with cbp_l 0 and cbp_c 0, 1, 2 (no
                        flag); P_8x8 with four sub types 8x8 and cbp_l non-zero (the flag present, 0 and 1); P_8x8 with a smaller sub
                        type and cbp_l 15 (no flag) - each between two macroblocks whose flag is 1; an i8u between such macroblocks

build() -> {name: (bytes, the writer's counters)}.  main() writes the files and runs the unmodified reference (oracle/_ref/h264dec and
oracle/_ref/ref_dump, built by oracle/Makefile) on each of them, once, on the CPU.  tests/golden/uncoded_t8_ref.json keeps its verdict:
exit status, SHA-1 and size of the YUV, SHA-1 per picture, the size and SHA-1 of every file it wrote in compress mode, whether its own
restore returned the input - and, from the dump, the luma QP the reference held for every macroblock when it reconstructed the picture.
The reference's pictures of the one stream it decodes otherwise are kept as they are (uncoded_t8_stale_ref.yuv, 4608 bytes a picture)."""
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import h264_synth_cabac_i8 as K8  # noqa: E402
import h264_synth_t8 as T  # noqa: E402

OUT = os.path.join(HERE, "uncoded_t8")
STALE = "i8_cbp0_cavlc_i_stale"
MB_W, MB_H, N = 4, 3, 12
PIC_BYTES = N * 384
CDC = [[3, 0, -1, 0], [0, 2, 0, 0]]


def _c64(seed):
    c = [0] * 64
    c[0] = 4 + seed; c[1] = -2; c[2] = 1; c[3] = -1; c[6] = 2 - seed; c[9] = 1; c[21] = -1; c[40 + seed] = 1
    return c


FULL = {k: _c64(k) for k in range(4)}
L16 = {0: [2, -1] + [0] * 14, 5: [1] + [0] * 15, 10: [-1, 1] + [0] * 14, 15: [1] + [0] * 15}


class Cavlc:
    """the descriptions of tests/h264_synth_t8.py"""
    cabac = False
    pcm, skip, i4, part = staticmethod(T.pcm), staticmethod(T.skip), staticmethod(T.i4), staticmethod(T.part)

    @staticmethod
    def new():
        return T.SynthT8(MB_W, MB_H, pic_init_qp=28)

    @staticmethod
    def sl(first_mb, typ, qp, mbs, deblock=(0, 0, 0)):
        return dict(first_mb=first_mb, type=typ, qp=qp, mbs=mbs, deblock=deblock)

    @staticmethod
    def i8u():
        return T.i8()

    @staticmethod
    def i8c(cbp_l=5, cbp_c=0, dqp=0):
        return T.i8(cbp_l=cbp_l, cbp_c=cbp_c, dqp=dqp, luma=FULL, cdc=CDC)

    @staticmethod
    def i16(v, dqp=0, c=0):
        """flat: a luma DC level and, with c, chroma DC levels c (Cb) and -c (Cr)"""
        return T.i16(dc=[v] + [0] * 15, dqp=dqp, cbp_c=1 if c else 0, cdc=[[c, 0, 0, 0], [-c, 0, 0, 0]] if c else None)

    @staticmethod
    def p16(**kw):
        return T.p16(**kw)


class Cabac(Cavlc):
    """the descriptions of tests/h264_synth_cabac_i8.py: every slice under the CABAC PPS"""
    cabac = True
    i4, part = staticmethod(K8.i4), staticmethod(K8.part)

    @staticmethod
    def new():
        return K8.CabacSynthI8(MB_W, MB_H, pic_init_qp=28)

    @staticmethod
    def sl(first_mb, typ, qp, mbs, deblock=(0, 0, 0)):
        return dict(first_mb=first_mb, type=typ, qp=qp, mbs=mbs, deblock=deblock, pps=1, init_idc=first_mb % 3)

    @staticmethod
    def i8u():
        return K8.i8(cbp_l=0, cbp_c=0)

    @staticmethod
    def i8c(cbp_l=5, cbp_c=0, dqp=0):
        return K8.i8(cbp_l=cbp_l, cbp_c=cbp_c, dqp=dqp, luma8=FULL, cdc=CDC)

    @staticmethod
    def p16(**kw):
        return K8.p16(**kw)


def _flat_idr(W, s, qp=40):
    """an IDR picture of I16x16 macroblocks at levels that differ from neighbour to neighbour"""
    s.picture([W.sl(0, "I", qp, [W.i16(v) for v in (-9, 6, -4, 8, 7, -8, 9, -5, -6, 5, -7, 4)])], idr=True)


def _end(W, s):
    s.picture([W.sl(0, "P", 28, [W.skip(N)])])                   # (the reference's console application writes a picture when the next one arrives)


def i8_cbp0(W):
    """W: Cavlc (P slices behind a flat IDR picture) or Cabac (the first picture is the IDR picture itself, in I slices)"""
    s = W.new()
    u, c = W.i8u, W.i8c
    if not W.cabac:
        _flat_idr(W, s)
    first = "I" if W.cabac else "P"
    # picture 1: SliceQPY 40 and 38, filter on.  macroblock 0 starts its slice; 1 stands beside it; 2 moves the QP to 43, which 3 and 4
    # carry (4 has the upper neighbour only); 5 is coded with a non-zero mb_qp_delta behind them; 7 beside I4x4, 9 beside I_PCM, 11 ends
    # its slice and the picture
    s.picture([W.sl(0, first, 40, [u(), u(), W.i16(-8, dqp=3), u(), u(), c(cbp_l=9, cbp_c=1, dqp=-2)]),
               W.sl(6, first, 38, [W.i4(cbp_l=3, luma=L16), u(), W.pcm([70] * 256 + [120] * 128), u(), W.i16(9, dqp=4), u()])], idr=W.cabac)
    # picture 2, P slices: beside P_L0_16x16 with the flag 1, without the flag, and P_Skip; idc 2 (no filtering across the slice's
    # edge) and idc 1 (none at all)
    s.picture([W.sl(0, "P", 45, [W.p16(cbp_l=3, t8=1, luma8=FULL), u(), W.p16(), W.skip(2), u(), W.p16(cbp_l=4, cbp_c=1, luma=L16, cdc=CDC, dqp=-5), u()], deblock=(2, 0, 0)),
               W.sl(8, "P", 36, [u(), W.skip(1), u(), W.p16(cbp_c=2, cdc=CDC, cac={(0, 1): [1] + [0] * 14}, dqp=2)], deblock=(1, 0, 0))])
    # picture 3: the carried QP 51, and 0 behind a macroblock whose mb_qp_delta goes round the end
    s.picture([W.sl(0, first if W.cabac else "P", 51, [u(), W.i16(-3, dqp=1), u(), W.i16(2, dqp=-1), u(), c(dqp=-11), u(), W.i16(-6), W.i16(7, dqp=2), u(), u(), c(cbp_l=0, cbp_c=2)])])
    _end(W, s)
    return s.bytes(), s.count


# where the I picture under test has its i8u macroblocks, and the QP carried into each
I_UNDER_TEST = {1: 42, 2: 42, 5: 38, 7: 43, 10: 36, 11: 36}


def i8_cbp0_cavlc_i(shift):
    """shift 0: i8_cbp0_cavlc_i_same; 12: ..._stale (with the first picture)"""
    W = Cavlc
    s = W.new()
    u = W.i8u
    if shift:
        s.picture([W.sl(0, "I", 44, [W.i16(-6), W.i16(7, c=4), W.i16(-5), W.i16(6), W.i16(8, c=-4), u(), W.i16(-7, c=3), W.i16(5), W.i16(-4), W.i16(6, c=-5), W.i16(-8), W.i16(3)])], idr=True)
    # the earlier picture: an I16x16 macroblock everywhere, its QP at the places under test the carried one less `shift`
    qp, mbs = 40, []
    for k in range(N):
        want = I_UNDER_TEST.get(k, 40) - (shift if k in I_UNDER_TEST else 0)
        mbs.append(W.i16((-7, 6, -5, 8)[k % 4] * (1 if k < 8 else -1), dqp=want - qp))
        qp = want
    s.picture([W.sl(0, "I", 40, mbs)], idr=not shift)
    s.picture([W.sl(0, "I", 40, [W.i16(-8, dqp=2, c=4), u(), u(), W.i16(7, dqp=-4, c=-4), W.i8c(cbp_l=6, cbp_c=1), u(), W.i16(-6, dqp=5, c=5), u(),
                                 W.i4(cbp_l=8, luma=L16, dqp=-7), W.i16(6, c=-5), u(), u()])])
    _end(W, s)
    carried = {k: v for k, v in I_UNDER_TEST.items()}
    assert s.count["u8"]["n"] == len(carried) + (1 if shift else 0)
    return s.bytes(), s.count


def inter_t8_absent(W):
    s = W.new()
    _flat_idr(W, s)
    u, part = W.i8u, W.part
    t8 = lambda dqp=0: W.p16(cbp_l=15, t8=1, luma8=FULL, dqp=dqp)      # noqa: E731  (a macroblock whose flag is 1)
    cac = {(1, 2): [1, -1] + [0] * 13}
    under_test = [W.p16(), W.p16(cbp_c=1, cdc=CDC, dqp=-1), W.p16(cbp_c=2, cdc=CDC, cac=cac),
                  part("p16x8"), part("p16x8", cbp_c=1, cdc=CDC, dqp=2), part("p16x8", cbp_c=2, cdc=CDC, cac=cac),
                  part("p8x16"), part("p8x16", cbp_c=1, cdc=CDC), part("p8x16", cbp_c=2, cdc=CDC, cac=cac, dqp=1),
                  part("p8x8", subs=(0, 0, 0, 0), cbp_l=6, t8=0, luma=L16), part("p8x8", subs=(0, 0, 0, 0), cbp_l=9, t8=1, luma8=FULL, dqp=-3),
                  part("p8x8", subs=(0, 1, 0, 0), cbp_l=15, luma=L16)]
    last = [W.skip(1), W.p16(cbp_l=2, luma=L16), part("p8x8", subs=(3, 2, 1, 0), cbp_l=15, cbp_c=1, luma=L16, cdc=CDC), W.i16(5),
            part("p8x8", subs=(0, 0, 0, 0), cbp_l=15, t8=1, luma8=FULL), W.skip(1)]
    # rows of: flag 1, the macroblock under test, flag 1, one more
    for p in range(4):
        mbs = []
        for r in range(3):
            mbs += [t8(), under_test[3 * p + r], t8((-2, 0, 1)[r]), last[(3 * p + r) % len(last)]]
        s.picture([W.sl(0, "P", (38, 41, 44, 37)[p], mbs, deblock=(0, p - 1, 1 - p))])
    # an I8x8 macroblock without coefficients between inter macroblocks without the flag, in two slices
    s.picture([W.sl(0, "P", 43, [part("p16x8"), u(), part("p8x16", cbp_c=1, cdc=CDC, dqp=3), t8(), W.p16(), u()]),
               W.sl(6, "P", 39, [part("p8x8", subs=(0, 0, 0, 2), cbp_l=15, luma=L16), t8(), part("p8x8", subs=(1, 1, 1, 1)), u(), W.p16(cbp_c=1, cdc=CDC), t8()])])
    _end(W, s)
    return s.bytes(), s.count


def build():
    """-> {name: (bytes, the writer's counters)}"""
    return {"i8_cbp0_cavlc_p": i8_cbp0(Cavlc), "i8_cbp0_cabac": i8_cbp0(Cabac), "i8_cbp0_cavlc_i_same": i8_cbp0_cavlc_i(0), STALE: i8_cbp0_cavlc_i(12),
            "inter_t8_absent_cavlc": inter_t8_absent(Cavlc), "inter_t8_absent_cabac": inter_t8_absent(Cabac)}


def sha1(b):
    return hashlib.sha1(b).hexdigest()


def reference_verdict(name, data, tmp):
    from refdump import read_dump
    wd = os.path.join(tmp, name)
    os.makedirs(wd)
    src, pip, yuv, back = (os.path.join(wd, f) for f in (name + ".264", "out.pip", "out.yuv", "back.264"))
    open(src, "wb").write(data)

    def run(binary, *args):
        return subprocess.call([os.path.join(ROOT, "oracle", "_ref", binary)] + list(args), cwd=wd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    rec = dict(bytes=len(data), sha1=sha1(data), decode_rc=run("h264dec", src, pip, yuv))
    pictures = open(yuv, "rb").read() if os.path.exists(yuv) else b""
    rec.update(yuv_bytes=len(pictures), yuv_sha1=sha1(pictures), picture_sha1=[sha1(pictures[i:i + PIC_BYTES]) for i in range(0, len(pictures), PIC_BYTES)])
    files = {}
    if os.path.exists(pip):
        b = open(pip, "rb").read(); files["main"] = [len(b), sha1(b)]
    for q in glob.glob(pip + ".*"):
        b = open(q, "rb").read(); files[q.rsplit(".", 1)[1]] = [len(b), sha1(b)]
    rec["files"] = files
    rec["restore_rc"] = run("h264dec", pip, back)
    rec["reference_roundtrip"] = bool(os.path.exists(back) and open(back, "rb").read() == data)
    # the dump: what the reference handed to its reconstruction, taken when it reconstructs each slice
    rec["dump_rc"] = run("ref_dump", wd, src)
    dmp = os.path.join(wd, name + ".264.dmp")
    if rec["dump_rc"] == 0 and os.path.exists(dmp):
        frames = read_dump(dmp)
        rec["dump_qp_y"] = [[int(v) for v in f.mbs["qp_y"]] for f in frames]
        rec["dump_qp_c"] = [[int(v) for v in f.mbs["qp_c"][:, 0]] for f in frames]
        rec["dump_picture_sha1"] = [sha1(b"".join(np_bytes(p) for p in f.fin)) if f.has_final else None for f in frames]
    return rec, pictures


def np_bytes(a):
    import numpy as np
    return np.ascontiguousarray(a).tobytes()


def main():
    os.makedirs(OUT, exist_ok=True)
    ref = {}
    with tempfile.TemporaryDirectory(prefix="lh264_uncoded_t8_") as tmp:
        for name, (data, _) in sorted(build().items()):
            open(os.path.join(OUT, name + ".264"), "wb").write(data)
            ref[name], pictures = reference_verdict(name, data, tmp)
            assert ref[name]["decode_rc"] == 0, (name, "the reference refused the stream")
            if name == STALE:
                open(os.path.join(HERE, "uncoded_t8_stale_ref.yuv"), "wb").write(pictures)
            print(name, len(data), "bytes; reference: decodes, %d pictures," % len(ref[name]["picture_sha1"]), "roundtrip" if ref[name]["reference_roundtrip"] else "NO roundtrip", flush=True)
    json.dump(ref, open(os.path.join(HERE, "uncoded_t8_ref.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
