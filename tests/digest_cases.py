"""The SHA-1 vectors of the digest tests, shared by the host and the device test: padding edges at every start offset, a message
fed in spans, and a launch of many messages of different lengths.  hashlib is the reference."""
import ctypes as C
import hashlib

import numpy as np

EDGE_LENGTHS = [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 38016]     # padding edges; 38,016 = a QCIF picture = 594 blocks
OFFSETS = list(range(8))
SPAN_MESSAGE = 75600                                                         # a CVFC1_Sony_C picture: not a multiple of 64
SPAN_CUTS = [1, 63, 64, 0, 65]                                               # then the rest, and the reverse: the rest cut at 75,599

_pool = np.random.default_rng(20).integers(0, 256, 1 << 19, dtype=np.uint8)


def pool():
    return _pool


def run(lib, spans, n_messages, on_device, buf=None):
    """lh264_debug_sha1 over the pool -> [20-byte digests]"""
    buf = _pool if buf is None else buf
    sp = np.ascontiguousarray(np.array(spans, dtype=np.uint64).reshape(-1, 3))
    out = np.zeros(20 * max(n_messages, 1), np.uint8)
    rc = lib.lh264_debug_sha1(buf.ctypes.data_as(C.c_void_p), sp.ctypes.data_as(C.c_void_p), len(sp), n_messages, on_device, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return [out[20 * m:20 * m + 20].tobytes() for m in range(n_messages)]


def want(off, ln, buf=None):
    buf = _pool if buf is None else buf
    return hashlib.sha1(buf[off:off + ln].tobytes()).digest()


def edge_vectors():
    """every edge length at every start offset as ONE call of single-span messages -> (spans, [expected])"""
    spans, exp = [], []
    at = 0
    for ln in EDGE_LENGTHS:
        for off in OFFSETS:
            start = (at + 7) // 8 * 8 + off
            spans.append((len(exp), start, ln))
            exp.append(want(start, ln))
            at = start + ln
    assert at <= len(_pool)
    return spans, exp


def span_vectors():
    """the 75,600-byte message at offsets 0..7 cut three ways (message k of each way starts at offset k) -> (spans, n_messages, [expected])"""
    spans, exp = [], []
    ways = [SPAN_CUTS + [SPAN_MESSAGE - sum(SPAN_CUTS)], [SPAN_MESSAGE - 1, 0, 1], [64 * 100, 64 * 1000, SPAN_MESSAGE - 64 * 1100]]
    for way in ways:
        for off in (0, 1, 2, 3, 6):
            m, at = len(exp), off
            for ln in way:
                spans.append((m, at, ln))
                at += ln
            assert at - off == SPAN_MESSAGE
            exp.append(want(off, SPAN_MESSAGE))
    return spans, len(exp), exp


def many_vectors():
    """200 messages of pairwise different lengths from 0 to 20 kB at mixed offsets, one span each: lanes of a wave that end at different
    blocks, a wave that is not full (200 = 3 * 64 + 8), an empty message"""
    rng = np.random.default_rng(5)
    lens = [0, 20000] + sorted(int(x) for x in rng.choice(np.arange(1, 20000), 198, replace=False))
    rng.shuffle(lens)
    spans, exp = [], []
    for m, ln in enumerate(lens):
        start = int(rng.integers(0, len(_pool) - ln))
        spans.append((m, start, ln))
        exp.append(want(start, ln))
    assert len(set(lens)) == 200 and len(set(s[1] & 3 for s in spans)) == 4
    return spans, exp
