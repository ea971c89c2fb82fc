#!/usr/bin/env python3
"""The range-edge streams of tests/golden/edge/ and the reference's verdict on them, tests/golden/edge_ref.json.

build() writes every stream with tests/h264_synth.py (pure Python, deterministic) and returns {name: (bytes, counters)}; the tests
call it to check that the committed files regenerate byte for byte and to read the writer's counters.

main() writes the files and then runs the unmodified reference (oracle/_ref/h264dec, built by oracle/Makefile) on each of them, once,
on the CPU: compress and decode (`h264dec in.264 out.pip out.yuv`), restore (`h264dec out.pip back.264`).  The JSON
keeps per stream the SHA-1 and size, whether the reference decodes it and the SHA-1 of the cropped YUV, the size and SHA-1 of every
file written in compress mode, and whether its own restore returned the input.  Only these records are committed.
"""
import copy
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import h264_synth as H  # noqa: E402

EDGE_DIR = os.path.join(HERE, "edge")


def _blank_idr(S, qp=26, slice_mbs=None):
    n = S.n
    per = slice_mbs or n
    S.picture([dict(first_mb=a, type="I", qp=qp, mbs=[H.i16()] * min(per, n - a)) for a in range(0, n, per)], idr=True)


def _one(v):
    return [v] + [0] * 15


def skip_stream(longest):
    """40x30, one slice a picture: a blank IDR picture, then a P picture whose longest mb_skip_run is `longest`, followed by a coded
    macroblock; the rest of the picture in runs of at most 300"""
    S = H.Synth(40, 30)
    _blank_idr(S)
    mbs = [H.skip(longest), H.p16(mvd=(1, 0), cbp_l=1, luma={0: _one(2)})]
    rest = S.n - longest - 1
    while rest > 0:
        r = min(rest, 300)
        mbs.append(H.skip(r)); rest -= r
        if rest > 0:
            mbs.append(H.p16(mvd=(0, 1))); rest -= 1
    S.picture([dict(first_mb=0, type="P", qp=26, mbs=mbs)])
    return S


def skip_all():
    """a P picture that is one run of 1200 ending the slice"""
    S = H.Synth(40, 30)
    _blank_idr(S)
    S.picture([dict(first_mb=0, type="P", qp=26, mbs=[H.skip(1200)])])
    return S


def zero_run_4160():
    """80x52 in 10 slices of 416: pictures 2 and 3 are skipped but for one level in the last macroblock of picture 2, so that picture 3
    reads a zero run of 4159 from the model's history (a SKIPRUN prior index of 520 * 16 + 11)"""
    S = H.Synth(80, 52)
    _blank_idr(S, slice_mbs=416)
    sl = [dict(first_mb=a, type="P", qp=26, mbs=[H.skip(416)]) for a in range(0, 4160, 416)]
    sl2 = copy.deepcopy(sl)
    sl2[-1]["mbs"] = [H.skip(415), H.p16(cbp_l=1, luma={0: _one(1)})]
    S.picture(sl2)
    S.picture(sl)
    return S


def nref(pictures):
    """2x2: picture i (2..16) has i active references and uses the highest ref_idx; picture 17 has 16 again.  18 pictures:
    nref_2_3_15_16, refused for its last two; its first 16 pictures alone, at most 15 references: nref_2_3_15, which round-trips"""
    S = H.Synth(2, 2, num_ref_frames=16)
    S.picture([dict(first_mb=0, type="I", qp=26, mbs=[H.i16(dc=_one(10 * k - 15)) for k in range(4)])], idr=True)
    for i in range(1, pictures):
        nr = None if i == 1 else min(i, 16)
        top = (nr or 1) - 1
        refs = [top, 0, top, top // 2]
        S.picture([dict(first_mb=0, type="P", qp=26, num_ref=nr,
                        mbs=[H.p16(ref=r, mvd=(k - 1, 1 - k), cbp_l=1, luma={0: _one(3 + (i + k) % 5)}) for k, r in enumerate(refs)])])
    return S


def mvd_values():
    v = set()
    for k in range(14):
        v |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    return sorted((v | {10, 11}) - {0})                     # 9 | 10 is the unary / exp-Golomb joint of the coder's UEG binarisation


def mvd_edges():
    """one row of macroblocks, so that a motion vector is predicted from the left neighbour alone: mvd +v then -v takes the vector to
    (v, v) and back to 0, for v = 2^k - 1, 2^k, 2^k + 1, k <= 13, and 10, 11"""
    vals = mvd_values()
    S = H.Synth(2 * len(vals), 1)
    S.picture([dict(first_mb=0, type="I", qp=26, mbs=[H.i16(dc=[(7 * k) % 41 - 20, (3 * k) % 7 - 3] + [0] * 14) for k in range(S.n)])], idr=True)
    mbs = []
    for v in vals:
        mbs += [H.p16(mvd=(v, v)), H.p16(mvd=(-v, -v))]
    S.picture([dict(first_mb=0, type="P", qp=26, mbs=mbs)])
    return S


def qp_edges():
    """4x4, deblocking on: an I picture that starts at qp 41, climbs to 51, wraps to 0 with +1, then -26 (26), +25 (51), +25 (24),
    -26 (50); a P picture with the same jumps in P_L0_16x16 macroblocks"""
    S = H.Synth(4, 4)
    dq = [0] + [1] * 10 + [1, -26, 25, 25, -26]
    S.picture([dict(first_mb=0, type="I", qp=41,
                    mbs=[H.i16(cbp_l=15, cbp_c=1, dqp=d, dc=[3 * (k % 5) - 6, 1] + [0] * 14, ac={5: [1] + [0] * 14}, cdc=[[k % 3 - 1, 0, 0, 0], [1, 0, 0, 0]])
                         for k, d in enumerate(dq)])], idr=True)
    pq = [6, 1, -26, 25, 25, -26, 1]
    S.picture([dict(first_mb=0, type="P", qp=45,
                    mbs=[H.p16(mvd=(k, -k), cbp_l=1, dqp=d, luma={0: _one(k - 4 or 1)}) for k, d in enumerate(pq)] + [H.skip(16 - len(pq))])])
    return S


def pcm_edges(sample):
    """4x1: P pictures with a skip run, an I_PCM macroblock of 384 equal samples and a closing skip run; the slice header and the run are
    varied until pcm_alignment_zero_bits has started at each of the 8 bit phases"""
    S = H.Synth(4, 1)
    _blank_idr(S)
    for nr in (None, 1):
        for qp in range(20, 34):
            for r in (1, 2, 3):
                if len(S.count["pcm_phase"]) == 8:
                    return S
                T = copy.deepcopy(S)
                T.picture([dict(first_mb=0, type="P", qp=qp, num_ref=nr, mbs=[H.skip(r), H.pcm([sample] * 384)] + ([H.skip(3 - r)] if r < 3 else []))])
                if len(T.count["pcm_phase"]) > len(S.count["pcm_phase"]):
                    S = T
    return S


def _level_of(code):
    """the level whose levelCode is `code` (9.2.2.1: even codes are positive)"""
    return (code + 2) // 2 if code % 2 == 0 else -((code + 1) // 2)


def _ramp_then(sl, code):
    """levels in coding order (highest frequency first), none of them a trailing one: a ramp that takes suffixLength to `sl`, then the
    level whose levelCode at that suffixLength is `code`.  The first coded level carries the -2 of trailing_ones < 3"""
    ramp = [] if sl == 0 else [2] if sl == 1 else [4, 7, 13, 25, 49][:sl - 1]
    return ramp + [_level_of(code + (2 if not ramp else 0))]


def _escape_base(sl, prefix):
    """the smallest levelCode that level_prefix `prefix` >= 15 codes at suffixLength sl"""
    return (15 << sl) + (15 if sl == 0 else 0) + ((1 << (prefix - 3)) - 4096 if prefix > 15 else 0)


def _packed(coded, maxn, top=False):
    """levels in coding order -> the block in scan order, packed at the low end (total_zeros 0) or at the high end"""
    lo = list(reversed(coded))
    return [0] * (maxn - len(lo)) + lo if top else lo + [0] * (maxn - len(lo))


def level_cases(ext):
    """[(label, levels in coding order)]: every suffixLength 0..6 with each level_prefix of the range, and the range's largest levels"""
    cases = []
    for sl in range(7):
        for prefix in ((16, 17, 18, 19) if ext else (13, 14, 15)):
            code = _escape_base(sl, prefix) if prefix >= 15 else (prefix << sl) + (1 if prefix == 14 and sl == 0 else 0)
            cases.append(("sl%d_p%d" % (sl, prefix), _ramp_then(sl, code)))
    for sl in (0, 6):
        if ext:
            for v in (32767, -32767, -32768):
                cases.append(("sl%d_%d" % (sl, v), _ramp_then(sl, 0)[:-1] + [v]))
        else:
            top = _escape_base(sl, 15) + 4095               # the last code of the 12-bit suffix
            cases.append(("sl%d_top" % sl, _ramp_then(sl, top)))
            cases.append(("sl%d_top-1" % sl, _ramp_then(sl, top - 1)))
    return cases


def levels_stream(ext):
    """one slice a macroblock (no neighbour is available: nC comes from the macroblock's own blocks), qp 0..5; an I picture of I16x16
    and a P picture of P_L0_16x16 macroblocks, see level_cases and the comments below"""
    cases = level_cases(ext)
    imbs, pmbs = [], []
    for i, (label, coded) in enumerate(cases):               # each case in an Intra16x16 DC block and in a P luma block
        imbs.append(H.i16(dc=_packed(coded, 16)))
        pmbs.append(H.p16(cbp_l=1, luma={0: _packed(coded, 16, top=i % 2 == 1)}))
    if not ext:
        full16, full15 = [2, -3] * 8, [-2, 3] * 7 + [2]
        for first in (16, 2, 5):                             # block 1 sees nC = block 0's total: classes 8 and up, 2-3, 4-7; block 0 sees 0
            b0 = full16 if first == 16 else [3] * first + [0] * (16 - first)
            pmbs.append(H.p16(cbp_l=1, cbp_c=2, luma={0: b0, 1: full16}, cdc=[[2, -2, 3, 1], [1, 1, 1, 2]],
                              cac={(0, 0): b0[:15], (0, 1): full15, (1, 0): b0[:15], (1, 1): full15}))
            imbs.append(H.i16(cbp_l=15, cbp_c=1, dc=full16, ac={0: b0[:15], 1: full15}, cdc=[[5, 4, 3, 2], [0, 0, 0, 0]]))
        # every total_zeros table at its largest value: block i holds i + 1 levels at the high end; the last block a run_before of 14
        tz = {i: [0] * (15 - i) + [2 + i] * (i + 1) for i in range(15)}
        tz[15] = [3] + [0] * 14 + [-2]
        pmbs.append(H.p16(cbp_l=15, cbp_c=1, luma=tz, cdc=[[0, 0, 0, 1], [0, 0, 2, 1]]))
        pmbs.append(H.p16(cbp_l=0, cbp_c=1, cdc=[[0, 3, 1, 1], [0, 0, 0, 0]]))
        # total_coeff above 10 with 0, 1 and 2 trailing ones (suffixLength starts at 1)
        for t1 in range(3):
            imbs.append(H.i16(dc=[3] * (12 - t1) + [1] * t1 + [0] * 4))
    n = max(len(imbs), len(pmbs))
    w = 8
    h = (n + w - 1) // w
    S = H.Synth(w, h, profile=100 if ext else 66)
    imbs += [H.i16()] * (w * h - len(imbs))
    pmbs += [H.skip(1)] * (w * h - len(pmbs))
    S.picture([dict(first_mb=k, type="I", qp=k % 6, mbs=[m]) for k, m in enumerate(imbs)], idr=True)
    S.picture([dict(first_mb=k, type="P", qp=(k + 3) % 6, mbs=[m]) for k, m in enumerate(pmbs)])
    return S


def align_bits():
    """2x1: slices that end their picture with 1..7 alignment bits behind the stop bit, all of them ones (a decoder stops at the last
    macroblock and never reads them; the container carries them in its pad-bit stream); the slice ends in a coded macroblock or a run"""
    S = H.Synth(2, 1)
    S.picture([dict(first_mb=0, type="I", qp=26, mbs=[H.i16(), H.i16()], align=0x7f)], idr=True)
    for tail in (H.p16(mvd=(1, 0)), H.skip(1)):
        seen = set()
        for nr in (None, 1):
            for qp in range(20, 34):
                T = copy.deepcopy(S)
                T.picture([dict(first_mb=0, type="P", qp=qp, num_ref=nr, mbs=[H.p16(mvd=(0, 1), cbp_l=1, luma={0: _one(2)}), tail], align=0x7f)])
                if T.last_align not in seen:
                    seen.add(T.last_align)
                    S = T
    return S


BUILDERS = {
    "align_bits": align_bits,
    "levels_ref": lambda: levels_stream(False),
    "levels_ext": lambda: levels_stream(True),
    "skip511": lambda: skip_stream(511),
    "skip512": lambda: skip_stream(512),
    "skip513": lambda: skip_stream(513),
    "skip_all": skip_all,
    "zero_run_4160": zero_run_4160,
    "nref_2_3_15_16": lambda: nref(18),
    "nref_2_3_15": lambda: nref(16),
    "mvd_edges": mvd_edges,
    "qp_edges": qp_edges,
    "pcm_zero": lambda: pcm_edges(0),
    "pcm_255": lambda: pcm_edges(255),
}


def build():
    out = {}
    for name, fn in BUILDERS.items():
        S = fn()
        S.count["mbs"] = S.n
        out[name] = (S.bytes(), S.count)
    return out


def sha1(b):
    return hashlib.sha1(b).hexdigest()


def reference_verdict(name, data, tmp, pictures, mbs, messages=False):
    """messages: keep what the restore said last when it did not end well (an assertion's text, without its source path)"""
    cli = os.path.join(ROOT, "oracle", "_ref", "h264dec")
    wd = os.path.join(tmp, name); os.makedirs(wd)
    src = os.path.join(wd, "in.264")
    open(src, "wb").write(data)

    def run(*args, log=None):
        try:
            return subprocess.call([cli] + list(args), cwd=wd, stdout=subprocess.DEVNULL, stderr=open(log, "wb") if log else subprocess.DEVNULL, timeout=900)
        except subprocess.TimeoutExpired:
            return -999
    rec = {"bytes": len(data), "sha1": sha1(data)}
    yuv = os.path.join(wd, "out.yuv")
    rec["compress_rc"] = run(src, os.path.join(wd, "out.pip"), yuv)
    rec["yuv_bytes"] = os.path.getsize(yuv) if os.path.exists(yuv) else 0
    rec["yuv_sha1"] = sha1(open(yuv, "rb").read()) if rec["yuv_bytes"] else None
    rec["pictures"] = pictures
    # decoded: the application ended well and wrote every picture the writer made (4:2:0, no cropping in these streams)
    rec["reference_decodes"] = bool(rec["compress_rc"] == 0 and rec["yuv_bytes"] == pictures * mbs * 384)
    files = {}
    p = os.path.join(wd, "out.pip")
    if os.path.exists(p):
        b = open(p, "rb").read(); files["main"] = [len(b), sha1(b)]
    for q in glob.glob(p + ".*"):
        b = open(q, "rb").read(); files[q.rsplit(".", 1)[1]] = [len(b), sha1(b)]
    rec["files"] = files
    rec["restore_rc"] = run(p, os.path.join(wd, "back.264"), log=os.path.join(wd, "restore.log") if messages else None)
    back = os.path.join(wd, "back.264")
    rec["reference_roundtrip"] = bool(os.path.exists(back) and open(back, "rb").read() == data)
    if messages:
        rec["restore_bytes"] = os.path.getsize(back) if os.path.exists(back) else 0
        said = [ln for ln in open(os.path.join(wd, "restore.log"), errors="replace").read().splitlines() if ln.strip()]
        last = said[-1] if said and rec["restore_rc"] != 0 else ""
        rec["restore_message"] = re.sub(r"0x[0-9a-f]+", "0x..", re.sub(r"\S*/([\w.]+:\d+)", r"\1", re.sub(r"^\S*h264dec: ", "", last)))[:300]
    return rec


def main(only):
    """only: the streams to write and take the verdict on again (none named: all)"""
    os.makedirs(EDGE_DIR, exist_ok=True)
    streams = build()
    tmp = tempfile.mkdtemp(prefix="lh264_edge_")
    path = os.path.join(HERE, "edge_ref.json")
    out = json.load(open(path)) if only and os.path.exists(path) else {}
    for name, (data, count) in streams.items():
        if only and name not in only:
            continue
        open(os.path.join(EDGE_DIR, name + ".264"), "wb").write(data)
        out[name] = reference_verdict(name, data, tmp, count["pictures"], count["mbs"])
        print(name, len(data), "bytes; reference: rc", out[name]["compress_rc"], "decodes", out[name]["reference_decodes"],
              "roundtrip" if out[name]["reference_roundtrip"] else "NO roundtrip", flush=True)
    json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main(sys.argv[1:])
