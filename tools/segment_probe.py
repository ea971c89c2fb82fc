"""What a long stream costs: BA_MW_D.264 concatenated K times (a valid stream, tests/test_segments_gpu.py) through
lh264_compress_batch_opts, alone and beside a batch of short streams.

    python tools/segment_probe.py [K] [segment_mbs] [runs]      defaults: 256 copies, segments of 100 pictures (9,900 macroblocks), 3 runs

Prints, per run: the long stream alone (seconds, segments, MB/s of input), 511 short streams alone, and the 511 beside the long one;
then the buffers the library holds (lh264_compress_arena_bytes).  With LH264_TRACE_COMPRESS=1 the library adds, behind a long stream's
last segment, how full its prior table is (entries in use of hash_cap x 8) - the next limit a longer stream meets."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import losslessh264_amd as lh                                                   # noqa: E402
from losslessh264_amd import _lib as L                                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(datas, segment_mbs):
    t0 = time.perf_counter()
    b = lh.compress_batch_handles(datas, 16, segment_mbs=segment_mbs)
    dt = time.perf_counter() - t0
    bad = [i for i in range(b.n) if b.status(i) != 0]
    assert not bad, "streams %s failed" % bad
    segs = max(b.segments(i) for i in range(b.n))
    b.free()
    return dt, segs


def main(argv):
    K = int(argv[1]) if len(argv) > 1 else 256
    seg = int(argv[2]) if len(argv) > 2 else 9900
    runs = int(argv[3]) if len(argv) > 3 else 3
    one = open(os.path.join(ROOT, "tests", "golden", "streams", "BA_MW_D.264"), "rb").read()
    long_stream, short = one * K, [one] * 511
    run(short[:64], None)                                                       # (the first call allocates the buffers)
    for r in range(runs):
        a, sa = run([long_stream], seg)
        s, _ = run(short, seg)
        m, sm = run(short + [long_stream], seg)
        print("run %d: long stream alone %.3f s (%d segments, %.1f MB/s); 511 short streams %.3f s; together %.3f s (%d segments): +%.3f s" %
              (r, a, sa, len(long_stream) / a / 1e6, s, m, sm, m - s), flush=True)
    dev, pin = C.c_size_t(0), C.c_size_t(0)
    L.check(L.lib().lh264_compress_arena_bytes(C.byref(dev), C.byref(pin)))
    print("K = %d copies (%d bytes), segment_mbs = %d: buffers held %.1f MB on the device, %.1f MB page-locked" % (K, len(long_stream), seg, dev.value / 1e6, pin.value / 1e6))


if __name__ == "__main__":
    main(sys.argv)
