#!/usr/bin/env python3
"""Fixtures for the concealment of lost slices in the decode direction (tests/test_conceal.py, tests/test_conceal_gpu.py).

Runs only where the reference lies.  It builds tests/conceal_client.cpp against the reference's own header and libraries into
oracle/_ref/conceal_client (the libraries come from oracle/Makefile), derives damaged streams from tests/golden/streams/ by dropping
slice NAL units, decodes each of them with the reference under every concealment method we provide - through DecodeFrame2, one NAL
unit per call: the reference's console application never shows a concealed picture - and writes DATA only, under
tests/golden/conceal/:

  <name>.264            the damaged stream (a few KB)
  planes.<sha1>.npz     the three planes of the first damaged picture as the reference delivers it (ref.json: `planes`)
  ref.json              per stream: size, the concealed macroblocks per picture (from first_mb_in_slice of the slices that stayed),
                        and per method the SHA-1 and the DECODING_STATE of every delivered picture, and `unstable`: the pictures
                        that come out differently when four other pictures are decoded in front of the stream.  There the
                        reference's result is no function of the stream: a received macroblock filtered its edge against whatever
                        the recycled picture buffer held where the lost neighbour lies.
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
REFOUT = os.path.join(ROOT, "oracle", "_ref")
CLIENT = os.path.join(REFOUT, "conceal_client")
OUT = os.path.join(HERE, "conceal")
sys.path.insert(0, HERE)

# our names (losslessh264_amd._lib.CONCEAL) -> the reference's ERROR_CON_IDC
METHODS = {"slice_copy": 2, "slice_copy_cross_idr": 4, "slice_copy_cross_idr_freeze": 5, "mv_copy": 6, "mv_copy_freeze": 7}


def build_client():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle"), "ref"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-DLH264_USE_REFERENCE_HEADER", "-I" + os.path.join(REF, "codec", "api", "svc"),
                           os.path.join(ROOT, "tests", "conceal_client.cpp"), "-o", CLIENT, "-L" + REFOUT,
                           "-Wl,--start-group", "-ldecoder", "-lencoder", "-lprocessing", "-lcommon", "-lconsole_common", "-Wl,--end-group", "-lpthread"])


def nal_units(b):
    """[(begin, end, nal_unit_type, first_mb_in_slice or None)]: begin includes the start code and its leading zero"""
    starts = [m.start() for m in re.finditer(b"\x00\x00\x01", b)]
    begins = [p - 1 if p > 0 and b[p - 1] == 0 else p for p in starts]
    out = []
    for i, p in enumerate(starts):
        end = begins[i + 1] if i + 1 < len(starts) else len(b)
        t = b[p + 3] & 31
        first_mb = None
        if t in (1, 5):
            bits = "".join(format(x, "08b") for x in b[p + 4:p + 12])
            z = bits.index("1")
            first_mb = int(bits[z:2 * z + 1], 2) - 1
        out.append((begins[i], end, t, first_mb))
    return out


def pictures(units):
    """slice NAL indices per picture: a picture begins at a slice with first_mb_in_slice 0 (true of every stream used here)"""
    pics = []
    for i, u in enumerate(units):
        if u[2] in (1, 5):
            if u[3] == 0 or not pics:
                pics.append([])
            pics[-1].append(i)
    return pics


def cut(b, n_pictures):
    """the stream up to and including its first n_pictures pictures"""
    units = nal_units(b)
    pics = pictures(units)
    if len(pics) <= n_pictures:
        return b
    return b[:units[pics[n_pictures][0]][0]]


def damage(b, drops, total_mbs):
    """drops: [(picture, slice index within the picture)] -> (bytes, {picture: lost macroblocks})"""
    units = nal_units(b)
    pics = pictures(units)
    gone, lost = set(), {}
    for p, s in drops:
        sl = pics[p]
        s %= len(sl)
        k = sl[s]
        nxt = units[sl[s + 1]][3] if s + 1 < len(sl) else total_mbs
        gone.add(k)
        lost[p] = lost.get(p, 0) + nxt - units[k][3]
    return b"".join(b[u[0]:u[1]] for i, u in enumerate(units) if i not in gone), lost


def run_ref(tmp, data, method, skip=0):
    src, dst = os.path.join(tmp, "in.264"), os.path.join(tmp, "out.yuv")
    open(src, "wb").write(data)
    txt = subprocess.check_output([CLIENT, src, dst, str(method), str(skip)]).decode()
    states = [int(m.group(1), 16) for m in re.finditer(r"^pic \d+ state=0x([0-9a-f]+) ", txt, re.M)]
    sizes = [(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"^pic \d+ state=\S+ (\d+)x(\d+)$", txt, re.M)]
    yuv = open(dst, "rb").read()
    frames, at = [], 0
    for w, h in sizes:
        frames.append(yuv[at:at + w * h * 3 // 2])
        at += w * h * 3 // 2
    assert at == len(yuv)
    return frames, states, sizes


def synth(tmp, idc):
    """a short stream from the reference's encoder as make_synth_streams.py makes them: 256x192 (the smallest size at which its
    encoder cuts a picture into 4 slices: 48 macroblocks a slice at least), IDR + 3 P"""
    import make_synth_streams as S
    W, H, N = 256, 192, 4
    d = tempfile.mkdtemp(prefix="syn_", dir=tmp)
    for f in ("welsenc.cfg", "layer2.cfg"):
        shutil.copy(os.path.join(REF, "testbin", f), d)
    cfg = open(os.path.join(d, "welsenc.cfg")).read()
    cfg, n = re.subn(r"(?m)^LoopFilterDisableIDC\s+\d+", "LoopFilterDisableIDC       %d" % idc, cfg)
    assert n == 1
    open(os.path.join(d, "welsenc.cfg"), "w").write(cfg)
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[0:H, 0:W]
    noise0 = rng.normal(0, 5, (H, W))
    with open(os.path.join(d, "a.yuv"), "wb") as f:
        for t in range(N):
            noise = np.roll(noise0, (2 * t, 3 * t), axis=(0, 1))
            y = (128 + 60 * np.sin((xx + 3 * t) / 11.0) + 50 * np.cos((yy + 2 * t) / 7.0) + noise).clip(0, 255).astype(np.uint8)
            u = (128 + 40 * np.sin((xx[::2, ::2] + 2 * t) / 13.0)).clip(0, 255).astype(np.uint8)
            v = (128 + 40 * np.cos((yy[::2, ::2] + t) / 9.0)).clip(0, 255).astype(np.uint8)
            f.write(y.tobytes()); f.write(u.tobytes()); f.write(v.tobytes())
    out = os.path.join(d, "o.264")
    S.encode(d, "a.yuv", W, H, N, out, 16, ["-slcmd", "0", "1", "-slcnum", "0", "4"])
    return open(out, "rb").read()


def main():
    build_client()
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="lh264_conceal_")
    streams = os.path.join(HERE, "streams")
    rd = lambda n: open(os.path.join(streams, n), "rb").read()
    sva = rd("SVA_Base_B.264")
    # name -> (clean bytes, [(picture, slice)], macroblocks of a picture, kind).  kind "trailing": only slices at a picture's end are
    # lost, "idc12": the filter does not cross slice edges or is off - the reference's result is the stream's; "idc0": it is not
    cases = {
        "sva_tail5": lambda: (sva, [(5, -1)], "trailing"),
        "sva_mid5": lambda: (sva, [(5, 1)], "idc0"),
        "sva_head5": lambda: (sva, [(5, 0)], "idc0"),
        "sva_idr_tail": lambda: (sva, [(0, -1)], "trailing"),
        "sva_tail56": lambda: (sva, [(5, -1), (6, -1)], "trailing"),
        "cvfc1_tail": lambda: (cut(rd("CVFC1_Sony_C.jsv"), 4), [(2, -1)], "trailing"),
        # (picture 21: the first whose list 0 does not begin with the previous picture - the vector goes through the POC scaling)
        "mr1bt_tail": lambda: (cut(rd("MR1_BT_A.h264"), 23), [(21, -1)], "trailing"),
        "syn_idc2_mid": lambda: (synth(tmp, 2), [(2, 1)], "idc12"),
        "syn_idc1_mid": lambda: (synth(tmp, 1), [(2, 2)], "idc12"),
        "error_i_p": lambda: (rd("Error_I_P.264"), [], "asis"),
    }
    # (a decode with the reference takes seconds whatever the stream: `make_conceal_streams.py NAME...` renews the named cases only)
    todo = sys.argv[1:] or list(cases)
    lead = cut(sva, 4)
    path = os.path.join(OUT, "ref.json")
    ref = json.load(open(path)) if sys.argv[1:] and os.path.exists(path) else {}
    n_lead = {}
    sys.path.insert(0, ROOT)
    import losslessh264_amd as lh
    for name in todo:
        clean, drops, kind = cases[name]()
        first = lh.parse_file(clean)[0][0]
        mbs = first.mb_w * first.mb_h
        data, lost = damage(clean, drops, mbs) if drops else (clean, {})
        if name != "error_i_p":
            open(os.path.join(OUT, name + ".264"), "wb").write(data)
        entry = {"kind": kind, "bytes": len(data), "lost": {str(k): v for k, v in lost.items()}, "methods": {}}
        for mname, mid in METHODS.items():
            frames, states, sizes = run_ref(tmp, data, mid)
            # the same stream behind four other pictures of its own size (QCIF: of SVA_Base_B, else its own first four): the recycled
            # buffers hold something else.  The two runs are aligned from the end: how many pictures the lead delivers depends on what
            # follows it (at the end of a stream the reference does not deliver a damaged last picture)
            own_lead = lead if sizes and sizes[0] == (176, 144) else cut(clean, 4)
            frames2 = run_ref(tmp, own_lead + data, mid)[0]
            frames2 = frames2[len(frames2) - len(frames):] if len(frames2) >= len(frames) else []
            unstable = [k for k in range(len(frames)) if not frames2 or frames[k] != frames2[k]]
            m = {"sha1": [hashlib.sha1(f).hexdigest() for f in frames], "states": states, "unstable": unstable}
            if len(set(sizes)) <= 1:
                m["size"] = list(sizes[0]) if sizes else None
            else:
                m["sizes"] = [list(z) for z in sizes]
            concealed = [k for k, s in enumerate(states) if s & 0x20]
            m["first_concealed"] = concealed[0] if concealed else -1
            m["planes"] = None
            if concealed and name != "error_i_p":
                k = concealed[0]
                w, h = sizes[k]
                a = np.frombuffer(frames[k], np.uint8)
                m["planes"] = "planes.%s.npz" % m["sha1"][k][:10]        # (methods and streams that agree share a file)
                np.savez_compressed(os.path.join(OUT, m["planes"]), y=a[:w * h].reshape(h, w),
                                    u=a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), v=a[w * h * 5 // 4:].reshape(h // 2, w // 2))
            entry["methods"][mname] = m
            print("%-14s %-28s %2d pictures, first concealed %2d, unstable %s" % (name, mname, len(frames), m["first_concealed"], unstable))
        ref[name] = entry
    with open(path, "w") as f:          # a line per stream
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(ref[k], sort_keys=True, separators=(",", ":")) for k in sorted(ref)) + "\n}\n")
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
