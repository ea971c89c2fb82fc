#!/usr/bin/env python3
"""The streams of tests/golden/escape/ and the reference's verdict on them, tests/golden/escape_ref.json: CAVLC streams with skip runs
above 511 and with 16 active references, the two values the container's prior tables code modulo their tree and the escape stream
(tag 71, include/lh264.h LH264_TAG_ESC) carries.

build() writes every stream with tests/h264_synth.py (pure Python, deterministic) and returns {name: (bytes, counters)}; the tests call
it to check that the committed files regenerate byte for byte.

main() writes the files and then runs the unmodified reference (oracle/_ref/h264dec, built by oracle/Makefile) on each of them, once, on
the CPU, exactly as tests/golden/make_edge_streams.py does (its reference_verdict): the JSON keeps per stream the SHA-1 and size,
whether the reference decodes it and the SHA-1 of the YUV, the size and SHA-1 of every file written in compress mode, and whether its
own restore returned the input.  Only these records are committed.
"""
import importlib.util
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import h264_synth as H  # noqa: E402

ESCAPE_DIR = os.path.join(HERE, "escape")


def _edge():
    spec = importlib.util.spec_from_file_location("make_edge_streams", os.path.join(HERE, "make_edge_streams.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _one(v):
    return [v] + [0] * 15


def _blank_idr(S):
    S.picture([dict(first_mb=0, type="I", qp=26, mbs=[H.i16()] * S.n)], idr=True)


def _coded(k=0, ref=0):
    return H.p16(ref=ref, mvd=(1 + k % 3, -(k % 2)), cbp_l=1, luma={0: _one(2 + k % 4)})


def runs_hi():
    """52x32 = 1664 macroblocks, a blank IDR picture, then P pictures of one slice:
      1  runs of 512 (low part 0) and 1023, a coded macroblock behind each, a closing run of 127
      2  1024, a coded macroblock, an in-range run of 511, a coded macroblock, 127
      3  1636 (1536 + 100), a coded macroblock, 27
      4  one run of 1664 that ends the slice
      5  two slices of 832: the first one run of 832, the second a run of 600, a coded macroblock, 231
    high parts 1, 2 and 3; gaps above 0; a run that ends its slice and runs followed by a macroblock"""
    S = H.Synth(52, 32)
    _blank_idr(S)
    S.picture([dict(first_mb=0, type="P", qp=26, mbs=[H.skip(512), _coded(0), H.skip(1023), _coded(1), H.skip(127)])])
    S.picture([dict(first_mb=0, type="P", qp=26, mbs=[H.skip(1024), _coded(2), H.skip(511), _coded(3), H.skip(127)])])
    S.picture([dict(first_mb=0, type="P", qp=26, mbs=[H.skip(1636), _coded(4), H.skip(27)])])
    S.picture([dict(first_mb=0, type="P", qp=26, mbs=[H.skip(1664)])])
    S.picture([dict(first_mb=0, type="P", qp=26, mbs=[H.skip(832)]),
               dict(first_mb=832, type="P", qp=26, mbs=[H.skip(600), _coded(5), H.skip(231)])])
    assert S.count["skip_runs"] == [512, 1023, 127, 1024, 511, 127, 1636, 27, 1664, 832, 600, 231]
    return S


def _fill_refs(S, mbs_of, blank=False):
    """an IDR picture and 15 P pictures with 1..15 active references: 16 reference pictures are held from here on"""
    S.picture([dict(first_mb=0, type="I", qp=26, mbs=[H.i16(dc=None if blank else _one(10 * (k % 4) - 15)) for k in range(S.n)])], idr=True)
    for i in range(1, 16):
        S.picture([dict(first_mb=0, type="P", qp=26, num_ref=None if i == 1 else i, mbs=mbs_of(i))])


def nref16_mixed():
    """2x2, num_ref_frames 16: after the 16 pictures that fill the reference list, pictures with 16, 16, 15, 16 active references, then
    one picture of two slices with 16 and 3: the NUMREF entries repeat, close and reopen"""
    S = H.Synth(2, 2, num_ref_frames=16)
    _fill_refs(S, lambda i: [_coded(i + k, ref=(i - 1) if k == 0 else 0) for k in range(4)])
    for j, nr in enumerate((16, 16, 15, 16)):
        S.picture([dict(first_mb=0, type="P", qp=26, num_ref=nr, mbs=[_coded(j + k, ref=(nr - 1, 0, nr // 2, 1)[k]) for k in range(4)])])
    S.picture([dict(first_mb=0, type="P", qp=26, num_ref=16, mbs=[_coded(7, ref=15), _coded(8, ref=3)]),
               dict(first_mb=2, type="P", qp=26, num_ref=3, mbs=[_coded(9, ref=2), _coded(10)])])
    assert S.count["num_ref_idx"][16] == 15
    return S


def both():
    """40x30, num_ref_frames 16: 15 P pictures that are one run of 1200 fill the reference list; then runs above 511 and 16 active
    references in the same pictures, so that the entries of the two tables interleave"""
    S = H.Synth(40, 30, num_ref_frames=16)
    _fill_refs(S, lambda i: [H.skip(1200)], blank=True)
    S.picture([dict(first_mb=0, type="P", qp=26, num_ref=16, mbs=[H.skip(600), _coded(0, ref=15), H.skip(599)])])
    S.picture([dict(first_mb=0, type="P", qp=26, num_ref=16, mbs=[_coded(1, ref=7), H.skip(1100), _coded(2, ref=15), H.skip(98)])])
    S.picture([dict(first_mb=0, type="P", qp=26, num_ref=15, mbs=[H.skip(100), _coded(3, ref=14), H.skip(1099)])])
    S.picture([dict(first_mb=0, type="P", qp=26, num_ref=16, mbs=[H.skip(1199), _coded(4, ref=15)])])
    return S


BUILDERS = {"runs_hi": runs_hi, "nref16_mixed": nref16_mixed, "both": both}


def build():
    out = {}
    for name, fn in BUILDERS.items():
        S = fn()
        S.count["mbs"] = S.n
        out[name] = (S.bytes(), S.count)
    return out


def main(only):
    """only: the streams to write and take the verdict on again (none named: all)"""
    os.makedirs(ESCAPE_DIR, exist_ok=True)
    verdict = _edge().reference_verdict
    streams = build()
    tmp = tempfile.mkdtemp(prefix="lh264_escape_")
    path = os.path.join(HERE, "escape_ref.json")
    out = json.load(open(path)) if only and os.path.exists(path) else {}
    for name, (data, count) in streams.items():
        if only and name not in only:
            continue
        open(os.path.join(ESCAPE_DIR, name + ".264"), "wb").write(data)
        out[name] = verdict(name, data, tmp, count["pictures"], count["mbs"])
        print(name, len(data), "bytes; reference: rc", out[name]["compress_rc"], "decodes", out[name]["reference_decodes"],
              "roundtrip" if out[name]["reference_roundtrip"] else "NO roundtrip", flush=True)
    json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main(sys.argv[1:])
