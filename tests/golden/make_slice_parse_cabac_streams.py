"""Writes tests/golden/slice_parse_cabac/: streams for paths of the CABAC macroblock layer (csrc/lh264_slice_cabac.h) that no other
committed CABAC stream reaches (tests/test_slice_parse_cabac.py counts what the set reaches).

  cabac_wide.264   257 x 2 macroblocks - wider than the 256 columns whose line of neighbour state the kernel keeps in LDS.  An IDR
                   picture and a P picture of two CABAC slices each, the second starting mid-row at macroblock 100, so that in the
                   second row columns 100..256 have both neighbours in their slice, columns 255 / 256 among them, and columns 0..99
                   the left one only.  I16x16 with and without coefficients, one I_PCM, P_L0_16x16 with mvd and residual, skips.

  cabac_i8.264     4 x 3 macroblocks, written by tests/h264_synth_cabac_i8.py.  An IDR picture of two slices, the second starting
                   mid-row at macroblock 6, and a P picture.  I8x8 macroblocks with neither, the left, the upper and both neighbours in
                   their slice; two that are a slice's first macroblock; the transform_size_8x8_flag increments 0, 1 and 2 (in the P
                   picture also from P_L0_16x16 macroblocks with the 8x8 transform); mb_type increments 0, 1 and 2 on I8x8 and on
                   I16x16 macroblocks (an I_NxN neighbour adds nothing); prev_intra8x8_pred_mode_flag both ways, with the predicted
                   mode coming from the left macroblock's right column and from the upper macroblock's bottom row.  Every I8x8
                   macroblock carries a coefficient (those without: tests/golden/uncoded_t8/).

main() writes the files and runs the unmodified reference (oracle/_ref/h264dec, built by oracle/Makefile) on each of them, once, on the
CPU: `h264dec in.264 out.pip out.yuv`.  tests/golden/slice_parse_cabac_ref.json keeps its verdict: the exit status and the SHA-1 of
the pictures it wrote."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import h264_synth_cabac as K  # noqa: E402
import h264_synth_cabac_i8 as K8  # noqa: E402

OUT = os.path.join(HERE, "slice_parse_cabac")
W, SPLIT = 257, 100


def _i(k):
    """an I16x16 macroblock whose content depends on its address: every third one has AC and chroma coefficients"""
    dc = [(7 * k) % 23 - 11, (3 * k) % 5 - 2] + [0] * 14
    if k % 3:
        return K.i16(dc=dc)
    return K.i16(cbp_l=15, cbp_c=2, dc=dc, ac={k % 16: [1 + k % 3, 0, -1] + [0] * 12}, cdc=[[2, 0, -1, 0], [0, 1, 0, 0]], cac={(k % 2, k % 4): [1] + [0] * 14})


def _p(k):
    """P_L0_16x16 with a vector difference that changes the mvd context increment from column to column; every fourth carries a residual"""
    mvd = ((k * 5) % 13 - 6, (k * 3) % 9 - 4)
    if k % 4 == 1:
        return K.p16(mvd=mvd, cbp_l=1, cbp_c=1, luma={0: [2, -1] + [0] * 14}, cdc=[[1, 0, 0, 0], [0, 0, -1, 0]], dqp=(k % 3) - 1)
    return K.p16(mvd=mvd)


def _c64(seed):
    """64 levels in scan order: a DC, a few low frequencies, a level above the prefix of coeff_abs_level_minus1 and one far coefficient"""
    c = [0] * 64
    c[0] = 6 + seed; c[1] = -2; c[2] = 1; c[5] = -1 - seed % 2; c[9] = 1; c[20 + seed] = -1; c[41 + 5 * seed] = 1
    if seed == 3:
        c[63] = -1; c[3] = 17
    return c


def build_i8():
    s = K8.CabacSynthI8(4, 3, pic_init_qp=28)
    i8, i16 = K8.i8, K.i16
    full = {k: _c64(k) for k in range(4)}
    cdc = [[3, 0, -1, 0], [0, 2, 0, 0]]
    dc = [5, -1] + [0] * 14
    first = [i8(modes=(2, 1, 0, 0), cbp_l=15, cbp_c=1, luma8=full, cdc=cdc),                     # 0: first of the slice, no neighbour
             i8(modes=(1, 2, 1, 3), cbp_l=5, luma8=full, dqp=2),                                  # 1: left
             i16(dc=dc),                                                                          # 2
             i8(modes=(1, 2, 1, 8), cbp_l=8, cbp_c=2, luma8=full, cdc=cdc, cac={(0, 1): [1, -1] + [0] * 13, (1, 2): [2] + [0] * 14}),   # 3: left, an I16x16
             i8(modes=(2, 7, 2, 8), cbp_l=2, luma8=full, dqp=-3),                                 # 4: top
             i8(modes=(0, 3, 0, 1), cbp_l=0, cbp_c=1, cdc=cdc)]                                   # 5: both, both I8x8; chroma coefficients only
    second = [i8(modes=(2, 1, 0, 0), cbp_l=9, luma8=full),                                        # 6: first of a slice that starts mid-row
              i16(cbp_l=15, dc=dc, ac={3: [1] + [0] * 14}),                                       # 7
              i16(dc=dc), i16(dc=dc, cbp_c=1, cdc=cdc),                                           # 8, 9
              i16(dc=dc, cbp_c=2, cdc=cdc, cac={(1, 3): [1] + [0] * 14}),                         # 10: an I8x8 macroblock above
              i8(modes=(0, 3, 1, 7), cbp_l=6, luma8=full, dqp=1)]                                 # 11: both, and both I16x16: mb_type increment 2
    s.picture([dict(first_mb=0, type="I", qp=28, pps=1, mbs=first), dict(first_mb=6, type="I", qp=33, pps=1, mbs=second)], idr=True)
    p8 = {k: _c64(k) for k in range(4)}
    pmbs = [K.p16(mvd=(2, -1), cbp_l=3, t8=1, luma8=p8),                                          # 0
            i8(modes=(1, 2, 1, 8), cbp_l=1, luma8=full),                                          # 1: the flag's increment from an inter macroblock
            K.skip(1),                                                                            # 2
            K.p16(mvd=(-3, 0)),                                                                   # 3
            i8(modes=(0, 0, 2, 1), cbp_l=12, cbp_c=1, luma8=full, cdc=cdc, dqp=-1),               # 4: top only
            i8(modes=(2, 0, 1, 2), cbp_l=15, luma8=full),                                         # 5: increment 2
            K.p16(mvd=(0, 4), cbp_l=8, t8=1, luma8=p8, cbp_c=1, cdc=cdc),                         # 6: ... and on an inter macroblock beside an I8x8
            K.skip(1),                                                                            # 7
            i16(dc=dc),                                                                           # 8
            i8(modes=(1, 0, 8, 2), cbp_l=4, luma8=full),                                          # 9: left I16x16, top I8x8, in a P slice
            K.skip(2)]
    s.picture([dict(first_mb=0, type="P", qp=30, pps=1, init_idc=1, mbs=pmbs)])
    s.picture([dict(first_mb=0, type="P", qp=28, pps=1, mbs=[K.skip(12)])])
    return s.bytes(), s.count


def build():
    """-> {name: (bytes, the writer's counters)}"""
    s = K.CabacSynth(W, 2, pic_init_qp=28)
    n = 2 * W
    pcm_at = W + 255                                             # second row, column 255: its right neighbour reads the I_PCM terms
    first = [_i(k) for k in range(SPLIT)]
    second = [K.pcm([(k * 7 + j) % 256 for j in range(384)]) if k == pcm_at else _i(k) for k in range(SPLIT, n)]
    s.picture([dict(first_mb=0, type="I", qp=28, pps=1, mbs=first), dict(first_mb=SPLIT, type="I", qp=30, pps=1, mbs=second)], idr=True)
    pa, pb = [], []
    for k in range(n):
        dst = pa if k < SPLIT else pb
        if k in (W + 254, W + 256):
            dst.append(_i(k))                                    # intra macroblocks in a P slice beside column 255
        elif k % 7 in (2, 3) and k not in (W + 255,):
            dst.append(K.skip(1))
        else:
            dst.append(_p(k))
    s.picture([dict(first_mb=0, type="P", qp=28, pps=1, init_idc=1, mbs=pa), dict(first_mb=SPLIT, type="P", qp=27, pps=1, init_idc=2, mbs=pb)])
    s.picture([dict(first_mb=0, type="P", qp=28, pps=1, mbs=[K.skip(n)])])      # (the reference's console application writes a picture when the next one arrives)
    return {"cabac_wide": (s.bytes(), s.count), "cabac_i8": build_i8()}


def main():
    os.makedirs(OUT, exist_ok=True)
    cli = os.path.join(ROOT, "oracle", "_ref", "h264dec")
    ref = {}
    for name, (data, _) in sorted(build().items()):
        open(os.path.join(OUT, name + ".264"), "wb").write(data)
        ref[name] = dict(bytes=len(data), sha1=hashlib.sha1(data).hexdigest())
        if os.path.exists(cli):
            with tempfile.TemporaryDirectory() as d:
                r = subprocess.run([cli, os.path.join(OUT, name + ".264"), os.path.join(d, "o.pip"), os.path.join(d, "o.yuv")], capture_output=True)
                yuv = open(os.path.join(d, "o.yuv"), "rb").read() if os.path.exists(os.path.join(d, "o.yuv")) else b""
            ref[name].update(decode_rc=r.returncode, yuv_bytes=len(yuv), yuv_sha1=hashlib.sha1(yuv).hexdigest())
    json.dump(ref, open(os.path.join(HERE, "slice_parse_cabac_ref.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(ref, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
