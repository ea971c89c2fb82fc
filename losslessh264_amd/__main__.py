"""Command line with the reference console application's calling convention (codec/console/dec/src/h264dec.cpp:150-178,
79-104): the file names decide the mode.

    python -m losslessh264_amd in.264  out.pip [out.yuv]    compress: out.pip = default stream, out.pip.<tag> = tagged streams
    python -m losslessh264_amd in.pip  out.264              restore the original bytes from in.pip + in.pip.<tag>
    python -m losslessh264_amd in.264  out.lhp              compress into ONE file (LHPIP1 container, include/lh264.h); the result is
                                                            restored and compared before it is written, and a stream the round trip
                                                            cannot carry (I_PCM, damaged or unsupported syntax) is stored verbatim
    python -m losslessh264_amd in.lhp  out.264              restore from the container
    python -m losslessh264_amd --segment-mbs N in.264 out.pip   compress through lh264_compress_batch_opts: a stream of more than N
                                                            macroblocks is coded in segments of whole pictures (a stream of any
                                                            length: memory follows the segment, the bytes are the same)
    python -m losslessh264_amd --escapes ...                (first) a stream with an mb_skip_run above 511 or 16 active references is
                                                            compressed with the escape stream, tag 71, beside it (out.pip.71, or in
                                                            the container) instead of being refused or stored verbatim
    python -m losslessh264_amd --tolerant ...               (first) through lh264_compress_batch_opts with LH264_COMPRESS_TOLERANT: NAL
                                                            units the format drops (delimiters, filler, ...) are kept, pictures with
                                                            lost slices are compressed; out.lhp is still restored and compared
                                                            before it is written, with the verbatim fallback behind it
    python -m losslessh264_amd --decode [--device-parse | --device-parse-cabac] [--nv12] [--conceal METHOD] out_dir in.264...   decode through ONE lh264_decode_batch call:
                                                            out_dir/<name>.yuv holds the cropped pictures as I420 (or NV12), appended
                                                            by a sink run by run.  METHOD: lost slices are concealed as the reference's
                                                            decoder does (slice_copy | slice_copy_cross_idr | mv_copy |
                                                            slice_copy_cross_idr_freeze | mv_copy_freeze) instead of ending the stream
    python -m losslessh264_amd --decode --motion | --motion-only ...   beside the pictures (--motion-only: and no picture file) every stream's
                                                            motion fields, out_dir/<name>.mv (int16: dx, dy, pictures back per 4x4 block) and
                                                            <name>.mbi (uint8: kind, qp, cbp, flags, sub types per macroblock) of its
                                                            delivered pictures, gathered on the device (decode_batch (motion=True))
    python -m losslessh264_amd --decode --sha1 [--nv12] [--conceal METHOD] out_dir in.264...   digests only, no .yuv: out_dir/<name>.sha1
                                                            holds a line `index width height frame_num idr hex` per picture and a last
                                                            line `stream hex`, the SHA-1 of all pictures in order (computed on the device)
    python -m losslessh264_amd --decode [--sha1] --scale N ...   N = 1 | 2 | 3: reduced-size pictures, the means of 2x2 / 4x4 / 8x8
                                                            blocks computed on the device (decode_batch (scale=N)); 0 = full size
    python -m losslessh264_amd --decode [--sha1] --at SPEC ...   only the pictures with the given numbers (decode order from 0) are
                                                            delivered: SPEC is a,b,c or start:stop:step (decode_batch (select=...));
                                                            of the stream only what they need is decoded, nothing behind the last
                                                            of them is read.  One SPEC for all files.  Not with --pick or --conceal
    python -m losslessh264_amd --decode [--sha1] --pick intra|idr ...   only the pictures whose slices are all I slices / the IDR pictures
                                                            are decoded and written (decode_batch (pick=...)); the index column of a
                                                            .sha1 file is the picture's number in the stream.  Not with --conceal
    python -m losslessh264_amd --decode [--sha1] --size WxH ...   every picture of every stream is written W x H (both even, 2..4096),
                                                            resampled on the device by an exact area average (decode_batch
                                                            (size=(W, H))); the aspect ratio is not kept.  Not with a non-zero --scale
    python -m losslessh264_amd --decode [--sha1] --size WxH --filter area|bilinear|bicubic ...   the filter of the resampling
                                                            (decode_batch (filter=...)): area (the default), or an antialiased
                                                            triangle / Catmull-Rom kernel.  bilinear and bicubic need --size
    python -m losslessh264_amd --decode [--sha1] --rgb rgb24|rgbp [--matrix auto|bt601|bt709] [--range auto|limited|full] ...   RGB pictures,
                                                            colour-converted on the device (decode_batch (colour=...)): out_dir/<name>.rgb
                                                            holds R, G, B per pixel (rgb24) or three planes per picture (rgbp); the
                                                            matrix and range come from the stream's SPS unless named.  Not with --nv12
    python -m losslessh264_amd --decode [--sha1] --rgb rgb24|rgbp --sample f32|f16|bf16 [--mul a,b,c] [--add a,b,c] ...   float RGB pictures,
                                                            cast and normalised on the device in the same pass (decode_batch (dtype=...,
                                                            mul=..., add=...)): element = fma (byte, mul[channel], add[channel]) in
                                                            binary32, rounded to the type; out_dir/<name>.f32 | .f16 | .bf16, little-endian
    python -m losslessh264_amd --decode [--sha1] [--crop x,y,w,h] [--size WxH --fit cover|contain [--fill y,cb,cr]] ...   fitted views
                                                            (decode_batch (crop=..., fit=..., fill=...)): --crop takes a rectangle of every
                                                            picture's window (four even numbers) in the window's place; --fit cover
                                                            resamples the largest centred part of it with the size's aspect, --fit contain
                                                            the whole of it into the largest centred part of the size, the rest filled
                                                            with y,cb,cr (default 16,128,128).  --fit needs --size, --fill --fit contain

Compress runs the host front end and the HIP context-index + coder kernels (needs the GPU); the optional YUV dump runs the
HIP reconstruct kernel and writes the cropped I420 pictures like the reference's decoder.  Restore is host code.
"""
import glob
import os
import sys

import numpy as np


def compress_single(src, dst, escapes=False, tolerant=False):
    import losslessh264_amd as lh
    data = open(src, "rb").read()
    blob = None
    why = ""
    try:
        # the streams of the container: through the library's whole compress call under --tolerant (the flag lives there), else through
        # the sessions
        main = tags = None
        if tolerant:
            (main, tags, err), = lh.compress_batch([data], escapes=escapes, tolerant=True)
            if err:
                main, why = None, err
        else:
            frames, err, main, pcm, esc = lh.parse_file(data, pcm=True, escapes=True)
            if err or not frames:
                main, why = None, err or "no picture"
            else:
                ctx = lh.CtxSession([frames])
                ctx.run()
                coder = lh.CoderSession(ctx, hash_cap=1 << 18, out_cap=max(1 << 16, 2 * len(data)))
                coder.run()
                ctx.synchronize()
                tags = coder.tags(0)
                if pcm:
                    tags[70] = pcm          # LH264_TAG_PCM: the samples of the I_PCM macroblocks travel as they are
                if escapes and esc:
                    tags[71] = esc          # LH264_TAG_ESC (--escapes): what the SKIPRUN / NUMREF trees drop of a value above their range
        if main is not None:
            if lh.restore(main, tags) == data:
                blob = lh.pack(main, tags)
            else:
                why = "the restored stream differs"
    except RuntimeError as e:
        why = str(e)
    if blob is None or len(blob) >= len(data) + 32:
        blob = lh.pack(data, {}, lh.VERBATIM)
        why = why or "no gain"
    with open(dst, "wb") as f:
        f.write(blob)
    print("%s: %d bytes -> %d bytes (%.4f)%s" % (src, len(data), len(blob), len(blob) / max(1, len(data)), "  [verbatim: %s]" % why if why else ""))


def restore_single(src, dst):
    import losslessh264_amd as lh
    out = lh.restore_file(open(src, "rb").read())
    with open(dst, "wb") as f:
        f.write(out)
    print("%s -> %s: %d bytes" % (src, dst, len(out)))


def compress_segmented(src, dst, segment_mbs, escapes=False, tolerant=False):
    import losslessh264_amd as lh
    data = open(src, "rb").read()
    b = lh.compress_batch_handles([data], segment_mbs=segment_mbs, escapes=escapes, tolerant=tolerant)
    main, tags, err = b.result(0)
    segs = b.segments(0)
    b.free()
    if err:
        raise SystemExit("cannot compress %s: %s" % (src, err))
    with open(dst, "wb") as f:
        f.write(main)
    for t, x in tags.items():
        with open("%s.%d" % (dst, t), "wb") as f:
            f.write(x)
    total = len(main) + sum(len(x) for x in tags.values())
    print("%s: %d bytes -> %d bytes (%.4f), %d segments" % (src, len(data), total, total / max(1, len(data)), segs))


def compress(src, dst, yuv=None, escapes=False):
    import losslessh264_amd as lh
    data = open(src, "rb").read()
    frames, err, main, pcm, esc = lh.parse_file(data, pcm=True, escapes=True)
    if err:
        raise SystemExit("cannot compress %s: %s" % (src, err))
    ctx = lh.CtxSession([frames])
    ctx.run()
    coder = lh.CoderSession(ctx, hash_cap=1 << 18, out_cap=max(1 << 16, 2 * len(data)))
    coder.run()
    ctx.synchronize()
    tags = coder.tags(0)
    if pcm:
        tags[70] = pcm                  # LH264_TAG_PCM (the reference writes no such file: its own restore fails on I_PCM streams)
    if escapes and esc:
        tags[71] = esc                  # LH264_TAG_ESC
    with open(dst, "wb") as f:
        f.write(main)
    for t, b in tags.items():
        with open("%s.%d" % (dst, t), "wb") as f:
            f.write(b)
    total = len(main) + sum(len(b) for b in tags.values())
    print("%s: %d bytes -> %d bytes (%.4f), %d pictures" % (src, len(data), total, total / max(1, len(data)), len(frames)))
    if yuv:
        sess = lh.ReconSession([frames])
        sess.run()
        sess.synchronize()
        with open(yuv, "wb") as f:
            for i, fr in enumerate(frames):
                pl = sess.picture(0, i)
                for p in range(3):
                    s = 1 if p else 0
                    f.write(np.ascontiguousarray(pl[p][fr.crop_y >> s:(fr.crop_y + fr.crop_h) >> s, fr.crop_x >> s:(fr.crop_x + fr.crop_w) >> s]).tobytes())


def restore(src, dst):
    import losslessh264_amd as lh
    main = open(src, "rb").read()
    tags = {}
    for p in glob.glob(glob.escape(src) + ".*"):
        ext = p[len(src) + 1:]
        if ext.isdigit():
            tags[int(ext)] = open(p, "rb").read()
    out = lh.restore(main, tags)
    with open(dst, "wb") as f:
        f.write(out)
    print("%s (+%d tagged streams) -> %s: %d bytes" % (src, len(tags), dst, len(out)))


SIZE_USAGE = "--size: WxH, both even, 2..4096; not with a non-zero --scale"
FILTER_USAGE = "--filter: area | bilinear | bicubic; bilinear and bicubic with --size only"
RGB_USAGE = "--rgb: rgb24 | rgbp, not with --nv12; --matrix: auto | bt601 | bt709 and --range: auto | limited | full, with --rgb only"
SAMPLE_USAGE = "--sample: f32 | f16 | bf16, with --rgb only; --mul and --add: three finite numbers a,b,c (R, G, B), with --sample only"
VIEW_USAGE = "--fit: cover | contain, with --size only; --fill: y,cb,cr in 0..255, with --fit contain only; --crop: x,y,w,h, four even numbers, x, y >= 0, w, h >= 2"
SAMPLE_NAMES = {"f32": "float32", "f16": "float16", "bf16": "bfloat16"}


def parse_three(text):
    """"a,b,c" -> three floats that are finite as binary32, or None"""
    import numpy as np
    parts = text.split(",")
    try:
        v = [float(x) for x in parts]
    except ValueError:
        return None
    with np.errstate(over="ignore"):
        ok = len(v) == 3 and all(x.strip() == x and x for x in parts) and bool(np.all(np.isfinite(np.asarray(v, dtype=np.float64).astype(np.float32))))
    return tuple(v) if ok else None


def parse_ints(text, n, top):
    """"a,b,.." -> n ints in 0..top, or None"""
    import re
    if not re.fullmatch(r"[0-9]{1,5}(,[0-9]{1,5}){%d}" % (n - 1), text):
        return None
    v = tuple(int(x) for x in text.split(","))
    return v if all(x <= top for x in v) else None


def parse_size(text):
    """"WxH" -> (W, H), or None where it is not a pair of even numbers in 2..4096"""
    import re
    m = re.fullmatch(r"([0-9]{1,4})x([0-9]{1,4})", text)
    if not m:
        return None
    w, h = int(m.group(1)), int(m.group(2))
    return (w, h) if all(2 <= v <= 4096 and v % 2 == 0 for v in (w, h)) else None


AT_USAGE = "--at: a,b,c (strictly increasing picture numbers) | start:stop:step (stop, step optional); not with --pick or --conceal"


def parse_at(text):
    """--at SPEC -> a list of numbers or a slice, as decode_batch (select=) takes them; None: not a spec"""
    import re
    if ":" in text:
        m = re.fullmatch(r"(\d{1,9})?:(\d{1,9})?(?::(\d{1,9})?)?", text)
        if not m or (m.group(3) is not None and int(m.group(3)) < 1):
            return None
        return slice(int(m.group(1) or 0), None if m.group(2) is None else int(m.group(2)), int(m.group(3) or 1))
    if not re.fullmatch(r"\d{1,9}(,\d{1,9})*", text):
        return None
    nums = [int(v) for v in text.split(",")]
    return nums if all(b > a for a, b in zip(nums, nums[1:])) else None


def decode(argv):
    import losslessh264_amd as lh
    at = None
    nv12, conceal, sha1, parse, scale, pick, size = False, None, False, "host", 0, "all", None
    colour, matrix, crange = None, None, None
    dtype, mul, add = None, None, None
    fit, fill, crop = None, None, None
    motion = 0      # 1: --motion, 2: --motion-only
    filt = "area"
    while argv and argv[0] in ("--filter", "--motion", "--motion-only", "--fit", "--fill", "--crop", "--nv12", "--conceal", "--sha1", "--device-parse", "--device-parse-cabac", "--scale", "--pick", "--at", "--size", "--rgb", "--matrix", "--range", "--sample", "--mul", "--add"):
        if argv[0] in ("--fit", "--fill", "--crop"):
            value = None
            if len(argv) >= 2:
                value = (argv[1] if argv[1] in ("cover", "contain") else None) if argv[0] == "--fit" else parse_ints(argv[1], 3, 255) if argv[0] == "--fill" else parse_ints(argv[1], 4, 16384)
            if argv[0] == "--crop" and value is not None and (any(x & 1 for x in value) or value[2] < 2 or value[3] < 2):
                value = None
            if value is None:
                print(VIEW_USAGE)
                return 2
            if argv[0] == "--fit":
                fit = value
            elif argv[0] == "--fill":
                fill = value
            else:
                crop = value
            argv = argv[2:]
            continue
        if argv[0] in ("--sample", "--mul", "--add"):
            value = None if len(argv) < 2 else SAMPLE_NAMES.get(argv[1]) if argv[0] == "--sample" else parse_three(argv[1])
            if value is None:
                print(SAMPLE_USAGE)
                return 2
            if argv[0] == "--sample":
                dtype = value
            elif argv[0] == "--mul":
                mul = value
            else:
                add = value
            argv = argv[2:]
            continue
        if argv[0] in ("--rgb", "--matrix", "--range"):
            allowed = {"--rgb": ("rgb24", "rgbp"), "--matrix": tuple(lh._lib.MATRIX), "--range": tuple(lh._lib.RANGE)}[argv[0]]
            if len(argv) < 2 or argv[1] not in allowed:
                print(RGB_USAGE)
                return 2
            if argv[0] == "--rgb":
                colour = argv[1]
            elif argv[0] == "--matrix":
                matrix = argv[1]
            else:
                crange = argv[1]
            argv = argv[2:]
            continue
        if argv[0] == "--size":
            size = parse_size(argv[1]) if len(argv) >= 2 else None
            if size is None:
                print(SIZE_USAGE)
                return 2
            argv = argv[2:]
            continue
        if argv[0] == "--filter":
            if len(argv) < 2 or argv[1] not in lh._lib.FILTER:
                print(FILTER_USAGE)
                return 2
            filt, argv = argv[1], argv[2:]
            continue
        if argv[0] == "--at":
            at = parse_at(argv[1]) if len(argv) >= 2 else None
            if at is None:
                print(AT_USAGE)
                return 2
            argv = argv[2:]
            continue
        if argv[0] == "--pick":
            if len(argv) < 2 or argv[1] not in ("intra", "idr"):
                print("--pick: intra | idr")
                return 2
            pick, argv = argv[1], argv[2:]
            continue
        if argv[0] in ("--device-parse", "--device-parse-cabac"):
            parse, argv = ("device" if argv[0] == "--device-parse" else "device+cabac"), argv[1:]
            continue
        if argv[0] == "--scale":
            if len(argv) < 2 or argv[1] not in ("0", "1", "2", "3"):
                print("--scale: 0 | 1 | 2 | 3")
                return 2
            scale, argv = int(argv[1]), argv[2:]
            continue
        if argv[0] in ("--motion", "--motion-only"):
            motion, argv = max(motion, 1 if argv[0] == "--motion" else 2), argv[1:]
            continue
        if argv[0] == "--nv12":
            nv12, argv = True, argv[1:]
        elif argv[0] == "--sha1":
            sha1, argv = True, argv[1:]
        else:
            if len(argv) < 2 or argv[1] not in lh._lib.CONCEAL:
                print("--conceal: one of " + " | ".join(lh._lib.CONCEAL))
                return 2
            conceal, argv = argv[1], argv[2:]
    if size is not None and scale != 0:
        print(SIZE_USAGE)
        return 2
    if (colour is not None and nv12) or (colour is None and (matrix is not None or crange is not None)):
        print(RGB_USAGE)
        return 2
    if (dtype is not None and colour is None) or (dtype is None and (mul is not None or add is not None)):
        print(SAMPLE_USAGE)
        return 2
    if (fit is not None and size is None) or (fill is not None and fit != "contain"):
        print(VIEW_USAGE)
        return 2
    if filt != "area" and size is None:
        print(FILTER_USAGE)
        return 2
    if motion and sha1:
        print("--motion, --motion-only: not with --sha1")
        return 2
    if at is not None and (pick != "all" or conceal not in (None, "off")):
        print(AT_USAGE)
        return 2
    vkw = dict(fit=fit or "stretch", fill=fill, crop=crop, select=at, filter=filt)
    ckw = dict(vkw, colour=colour, matrix=matrix or "auto", colour_range=crange or "auto", dtype=dtype or "uint8", mul=mul, add=add)
    if len(argv) < 2 or (pick != "all" and conceal not in (None, "off")):      # (--pick with --conceal: nothing to copy from)
        print(__doc__)
        return 2
    ret = 0
    if sha1:
        for name, status, err, pics, total in lh.decode_to_sha1_files(argv[1:], argv[0], fmt="nv12" if nv12 else "i420", conceal=conceal, parse=parse, scale=scale, pick=pick, size=size, **ckw):
            print("%s: %d pictures, stream %s%s" % (name, pics, total, "  [stopped: %s]" % err if status else ""))
            ret = ret or (1 if status else 0)
        return ret
    for name, status, err, pics, nbytes in lh.decode_to_files(argv[1:], argv[0], fmt="nv12" if nv12 else "i420", conceal=conceal, parse=parse, scale=scale, pick=pick, size=size, motion=motion, **ckw):
        print("%s: %d pictures, %d bytes%s" % (name, pics, nbytes, "  [stopped: %s]" % err if status else ""))
        ret = ret or (1 if status else 0)
    return ret


def main(argv):
    escapes = tolerant = False
    while len(argv) >= 2 and argv[1] in ("--escapes", "--tolerant"):      # the options that go first, in any order
        escapes, tolerant = escapes or argv[1] == "--escapes", tolerant or argv[1] == "--tolerant"
        argv = argv[:1] + argv[2:]
    if len(argv) >= 4 and argv[1] == "--decode":
        return decode(argv[2:])
    if len(argv) >= 5 and argv[1] == "--segment-mbs":
        compress_segmented(argv[3], argv[4], int(argv[2]), escapes, tolerant)
        return 0
    if len(argv) < 3:
        print(__doc__)
        return 2
    if argv[1].endswith(".lhp"):
        restore_single(argv[1], argv[2])
    elif argv[2].endswith(".lhp"):
        compress_single(argv[1], argv[2], escapes, tolerant)
    elif ".pip" in os.path.basename(argv[1]):      # as the reference decides (h264dec.cpp:167-173)
        restore(argv[1], argv[2])
    elif tolerant:                                 # (the library's whole compress call: 0 = no cut below its default)
        if len(argv) > 3:
            raise SystemExit("--tolerant writes no YUV dump through this command line (lh264dec --tolerant does)")
        compress_segmented(argv[1], argv[2], 0, escapes, True)
    else:
        compress(argv[1], argv[2], argv[3] if len(argv) > 3 else None, escapes)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
