"""Writes tests/golden/slice_parse/: streams for branches of the CAVLC macroblock layer that no other committed CAVLC stream reaches
(tests/test_slice_parse.py counts what the set reaches).

  i8_first.264   I_NxN with the 8x8 transform as the first macroblock of a slice - neither the left nor the upper neighbour is
                 available - beside I8x8 macroblocks that have the left or the upper neighbour.  Every I8x8 macroblock carries at
                 least one coefficient: for one with coded_block_pattern 0 in a CAVLC I slice the reference's filter reads the QP that the
                 picture before left at its address (its decode_slice.cpp:3328 refreshes the entry under IS_INTRA4x4 only; DESIGN.md
                 section 6), which is the subject of tests/golden/uncoded_t8/ (make_uncoded_t8_streams.py), not of this stream

main() writes the files and runs the unmodified reference (oracle/_ref/h264dec, built by oracle/Makefile) on each of them, once, on the
CPU: `h264dec in.264 out.pip out.yuv`.  tests/golden/slice_parse_ref.json keeps its verdict: the exit status and the SHA-1 of the
pictures it wrote."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import h264_synth_t8 as T  # noqa: E402

OUT = os.path.join(HERE, "slice_parse")


def _c64(seed):
    """64 levels in scan order: a DC, a few low frequencies and one far coefficient, so that every one of the four interleaved blocks
    carries something and the zero runs differ"""
    c = [0] * 64
    c[0] = 5 + seed; c[1] = -2; c[2] = 1; c[3] = -1; c[6] = 2 - seed; c[9] = 1; c[21] = -1; c[40 + seed] = 1
    return c


def build():
    """-> {name: (bytes, the writer's counters)}"""
    s = T.SynthT8(3, 3, pic_init_qp=28)
    full = {k: _c64(k) for k in range(4)}
    s.picture([
        dict(first_mb=0, type="I", qp=28, mbs=[T.i8(cbp_l=15, cbp_c=1, luma=full, cdc=[[3, 0, -1, 0], [0, 2, 0, 0]]), T.i8(modes=(1, None, 7, None), cbp_l=5, luma=full, dqp=3),
                                               T.i8(cbp_l=4, luma=full), T.i8(cbp_l=2, luma=full, dqp=-40 + 26)]),
        dict(first_mb=4, type="I", qp=40, mbs=[T.i8(modes=(None, 1, None, 7), cbp_l=8, luma=full), T.i16(dc=[4] + [0] * 15)]),
        dict(first_mb=6, type="I", qp=51, mbs=[T.i8(cbp_l=1, luma={0: _c64(0)}, dqp=1), T.i8(cbp_l=8, luma=full), T.i8(cbp_l=15, luma=full, dqp=-1)]),   # QP 51 + 1 goes round to 0, and back
    ], idr=True)
    s.picture([dict(first_mb=0, type="P", qp=28, mbs=[T.S.skip(9)])])          # (the reference's console application writes a picture when the next one arrives)
    return {"i8_first": (s.bytes(), s.count)}


def main():
    os.makedirs(OUT, exist_ok=True)
    cli = os.path.join(ROOT, "oracle", "_ref", "h264dec")
    ref = {}
    for name, (data, _) in sorted(build().items()):
        open(os.path.join(OUT, name + ".264"), "wb").write(data)
        with tempfile.TemporaryDirectory() as d:
            r = subprocess.run([cli, os.path.join(OUT, name + ".264"), os.path.join(d, "o.pip"), os.path.join(d, "o.yuv")], capture_output=True)
            yuv = open(os.path.join(d, "o.yuv"), "rb").read() if os.path.exists(os.path.join(d, "o.yuv")) else b""
        ref[name] = dict(bytes=len(data), sha1=hashlib.sha1(data).hexdigest(), decode_rc=r.returncode, yuv_bytes=len(yuv), yuv_sha1=hashlib.sha1(yuv).hexdigest())
    json.dump(ref, open(os.path.join(HERE, "slice_parse_ref.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(ref, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
