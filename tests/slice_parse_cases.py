"""Inputs of the slice-data tests (test_slice_parse.py, test_slice_parse_gpu.py): where the committed streams lie, and the damaged
streams - BA_MW_D.264 with one slice NAL unit cut short or with bytes of its slice data flipped, 20 seeded cases."""
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DIRS = ("streams", "edge", "cabac_edge", "escape", "slice_parse", "uncoded_t8")


def committed():
    """-> [(name, path)] of every committed stream, 'dir/file'"""
    out = []
    for d in DIRS:
        for f in sorted(os.listdir(os.path.join(GOLDEN, d))):
            out.append((d + "/" + f, os.path.join(GOLDEN, d, f)))
    return out


def read(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def nal_spans(data):
    """-> [(first byte behind the start code, end)] of the NAL units of an Annex-B stream"""
    at = []
    i = 0
    while True:
        i = data.find(b"\0\0\1", i)
        if i < 0:
            break
        at.append(i + 3)
        i += 3
    spans = []
    for k, a in enumerate(at):
        e = at[k + 1] - 3 if k + 1 < len(at) else len(data)
        while e > a and data[e - 1] == 0:
            e -= 1
        spans.append((a, e))
    return spans


def head(data, n_nals):
    """the stream up to and without its NAL unit n_nals"""
    spans = nal_spans(data)
    return data if n_nals >= len(spans) else data[:spans[n_nals][0] - 3].rstrip(b"\0")


def damaged_cases():
    """-> [(label, bytes)]: the first 24 NAL units of BA_MW_D.264 with one slice damaged.  10 cuts (the NAL unit keeps its first L bytes,
    L from a few bytes behind the header up to one byte short) and 10 flips (1 to 3 bytes of slice data xor-ed with a nonzero value)"""
    base = head(read("streams/BA_MW_D.264"), 24)
    spans = [(a, e) for a, e in nal_spans(base) if base[a] & 31 in (1, 5) and e - a > 40]
    rng = random.Random(264)
    out = []
    for k in range(20):
        a, e = spans[rng.randrange(len(spans))]
        if k < 10:
            keep = (8, 12, 20, 33, (e - a) // 2, e - a - 1)[k % 6] + rng.randrange(3)
            keep = min(keep, e - a - 1)
            d = base[:a + keep] + base[e:]
            out.append(("cut%02d_%d_of_%d" % (k, keep, e - a), d))
        else:
            b = bytearray(base)
            for _ in range(1 + k % 3):
                b[rng.randrange(a + 6, e)] ^= rng.randrange(1, 256)
            out.append(("flip%02d" % k, bytes(b)))
    return out
