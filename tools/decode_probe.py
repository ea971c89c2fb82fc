#!/usr/bin/env python3
"""lh264_decode_batch end to end on N copies of one stream: host bytes -> host bytes and host bytes -> device bytes, three runs each
(arenas warm after the first): MB/s of .264, pictures/s, the split per stage (lh264_decode_last_timing), the arena's size, and
lh264_parse_batch_discard - the host front end alone - on the same batch in the same process.

    tools/decode_probe.py [streams] [stream file] [--runs N] [--nv12] [--sha1] [--modes host,device,digests,parse] [--parse device|device+cabac] [--scale N] [--pick all|intra|idr] [--size WxH] [--filter area|bilinear|bicubic] [--colour rgb24|rgbp] [--dtype float32|float16|bfloat16] [--fit cover|contain] [--crop x,y,w,h] [--motion] [--select SPEC]

--sha1 adds the digests-only call (sha1="both", pictures=False: SHA-1 per picture and per stream on the device, nothing downloaded);
--scale N (1..3) asks for reduced-size pictures (decode_batch (scale=N)) and adds "scale" to the rows;
--size WxH asks for pictures of that size (decode_batch (size=(W, H)), both even, 2..4096, not with --scale) and adds "size" to the rows;
--filter area|bilinear|bicubic names the filter of that resampling (decode_batch (filter=...), the latter two with --size only); every
row carries "filter", "area" where none was named;
--colour rgb24|rgbp asks for RGB pictures (decode_batch (colour=...), not with --nv12) and adds "colour" to the rows;
--dtype float32|float16|bfloat16 asks for float RGB pictures (decode_batch (dtype=...), with --colour only; the factors are
normalise of the ImageNet means and deviations) and adds "dtype" to the rows;
--fit cover|contain asks for a fitted view (decode_batch (fit=...), with --size only; contain fills with 16, 128, 128) and --crop x,y,w,h
for a rectangle of every picture's window (decode_batch (crop=...)); they add "fit" and "crop" to the rows;
--motion asks for the motion fields beside the pictures (decode_batch (motion=True)) and adds "motion", the field bytes and the
milliseconds of decode_pack_motion_kernel (lh264_decode_last_motion) to the rows; the mode motion_only (--modes ...,motion_only) is the
call with pictures=False: nothing is reconstructed;
--pick intra|idr decodes the selected pictures only (decode_batch (pick=...)) and adds "pick" to the rows; every row carries
parsed_slices (the slices whose data was parsed, all streams) and the launch shape of the call (rounds, chains, jobs);
--select SPEC (a,b,c or start:stop:step, as --at of the command lines) asks for the pictures with those numbers of every stream
(decode_batch (select=...)) and adds "select" to the rows; every row carries chain_pictures too (the pictures reconstructed, all streams);
--modes picks the measurements (default host,device,parse; with --sha1 host,device,digests,parse).

One JSON line per measurement."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import losslessh264_amd as lh
from losslessh264_amd import _lib as L


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    runs = int(argv[argv.index("--runs") + 1]) if "--runs" in argv else 3
    if "--runs" in argv:
        args.remove(argv[argv.index("--runs") + 1])
    modes = ["host", "device"] + (["digests"] if "--sha1" in argv else []) + ["parse"]
    if "--modes" in argv:
        modes = argv[argv.index("--modes") + 1].split(",")
        args.remove(argv[argv.index("--modes") + 1])
    fmt = "nv12" if "--nv12" in argv else "i420"
    parse = "host"
    if "--parse" in argv:
        parse = argv[argv.index("--parse") + 1]
        args.remove(parse)
    scale = {}
    if "--scale" in argv:
        scale = {"scale": int(argv[argv.index("--scale") + 1])}
        args.remove(argv[argv.index("--scale") + 1])
    if "--pick" in argv:
        scale = dict(scale, pick=argv[argv.index("--pick") + 1])
        args.remove(argv[argv.index("--pick") + 1])
    if "--size" in argv:
        text = argv[argv.index("--size") + 1]
        scale = dict(scale, size=tuple(int(v) for v in text.split("x")))
        args.remove(text)
    filt = "area"
    if "--filter" in argv:
        filt = argv[argv.index("--filter") + 1]
        args.remove(filt)
    scale = dict(scale, filter=filt)
    if "--colour" in argv:
        scale = dict(scale, colour=argv[argv.index("--colour") + 1])
        args.remove(argv[argv.index("--colour") + 1])
    if "--dtype" in argv:
        mul, add = lh.normalise((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
        scale = dict(scale, dtype=argv[argv.index("--dtype") + 1])
        args.remove(argv[argv.index("--dtype") + 1])
    if "--fit" in argv:
        scale = dict(scale, fit=argv[argv.index("--fit") + 1])
        args.remove(argv[argv.index("--fit") + 1])
    if "--crop" in argv:
        text = argv[argv.index("--crop") + 1]
        scale = dict(scale, crop=tuple(int(v) for v in text.split(",")))
        args.remove(text)
    select, select_row = {}, {}
    if "--select" in argv:
        from losslessh264_amd.__main__ import parse_at
        text = argv[argv.index("--select") + 1]
        select, select_row = {"select": parse_at(text)}, {"select": text}
        if select["select"] is None:
            raise SystemExit("--select: a,b,c | start:stop:step")
        args.remove(text)
    motion = "--motion" in argv
    streams = int(args[0]) if args else 512
    path = args[1] if len(args) > 1 else os.path.join(ROOT, "tests", "golden", "streams", "BA_MW_D.264")
    data = open(path, "rb").read()
    datas = [data] * streams
    lib = L.lib()
    mb = streams * len(data) / 1e6
    base = {"stream": os.path.basename(path), "streams": streams, "input_MB": round(mb, 3), "format": fmt}
    for mode in [m for m in modes if m != "parse"]:
        for r in range(runs):
            t0 = time.perf_counter()
            factors = dict(select, **(dict(mul=mul, add=add) if "dtype" in scale else {}))
            if mode == "motion_only":
                b = lh.decode_batch(datas, fmt=fmt, motion=True, pictures=False, parse=parse, **scale, **factors)
            elif mode == "digests":
                b = lh.decode_batch(datas, fmt=fmt, sha1="both", pictures=False, parse=parse, **scale, **factors)
            else:
                b = lh.decode_batch(datas, fmt=fmt, device_out=mode == "device", parse=parse, motion=motion, **scale, **factors)
            dt = time.perf_counter() - t0
            ms = (C.c_double * 6)()
            lib.lh264_decode_last_timing(ms)
            pt = (C.c_double * 2)()
            lib.lh264_decode_last_parse_timing(pt)
            route = {} if parse == "host" else {"parse": parse, "routes": sorted(set(b.parse_path(i) for i in range(streams))), "device_parse_ms": round(pt[0], 1), "device_parse_slices": int(pt[1])}
            ch = (C.c_longlong * 3)()
            lib.lh264_decode_last_chains(ch)
            shape = {"parsed_slices": sum(b.parsed_slices(i) for i in range(streams)), "chain_pictures": sum(b.chain_pictures(i) for i in range(streams)), "rounds": int(ch[0]), "chains": int(ch[1]), "jobs": int(ch[2])}
            pics = sum(len(b.pictures(i)) for i in (0, streams - 1)) // 2 * streams
            bad = [i for i in range(streams) if b.status(i) != 0]
            extra = {"stream_sha1": b.stream_sha1(0).hex(), "same_digests": len(set(b.stream_sha1(i) for i in range(streams))) == 1} if mode == "digests" else {}
            if motion or mode == "motion_only":
                mms, mbytes = C.c_double(0), C.c_ulonglong(0)
                lib.lh264_decode_last_motion(C.byref(mms), C.byref(mbytes))
                extra = dict(extra, motion=True, field_MB=round(mbytes.value / 1e6, 1), motion_kernel_ms=round(mms.value, 3))
            out_bytes = 0 if mode == "motion_only" else sum(p[5] for p in b.pictures(0)) * streams
            b.free()
            dev, pin = lh.decode_arena_bytes()
            print(json.dumps(dict(base, what="decode_batch", out=mode, run=r, seconds=round(dt, 4), MBps=round(mb / dt, 1), pictures_per_s=round(pics / dt),
                                  output_MB=round(out_bytes / 1e6, 1), failed=len(bad),
                                  ms={"call": round(ms[0], 1), "parse": round(ms[1], 1), "staging": round(ms[2], 1), "enqueue": round(ms[3], 1),
                                      "wait_device": round(ms[4], 1), "delivery": round(ms[5], 1)},
                                  arena_device_MB=round(dev / 1e6, 1), arena_pinned_MB=round(pin / 1e6, 1), **shape, **extra, **route, **scale, **select_row)), flush=True)
    for r in range(runs if "parse" in modes else 0):
        dt, pics = lh.parse_batch_time(datas, threads=0, keep=False)
        print(json.dumps(dict(base, what="parse_batch_discard", run=r, seconds=round(dt, 4), MBps=round(mb / dt, 1), pictures_per_s=round(pics / dt))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
