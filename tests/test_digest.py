"""The digests of decoded pictures without a device: the SHA-1 code of sha1_spans_kernel stepped on the host (lh264_debug_sha1 with
on_device = 0) against hashlib, the argument rules of the new lh264_decode_batch flags, the exports and the constants."""
import ctypes as C
import os
import re

import pytest

import digest_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")


def _lib():
    import __graft_entry__ as g
    g.build()
    from losslessh264_amd import _lib as L
    return L, L.lib()


def test_padding_edges_at_every_offset_on_the_host():
    L, lib = _lib()
    spans, exp = D.edge_vectors()
    assert len(exp) == 13 * 8
    got = D.run(lib, spans, len(exp), 0)
    for s, g, w in zip(spans, got, exp):
        assert g == w, "length %d at offset %d" % (s[2], s[1] & 7)


def test_a_message_fed_in_spans_on_the_host():
    L, lib = _lib()
    spans, n, exp = D.span_vectors()
    assert D.run(lib, spans, n, 0) == exp
    # a message without a span is the empty message; no message at all is no work
    assert D.run(lib, [(1, 5, 3)], 2, 0) == [D.want(0, 0), D.want(5, 3)]
    assert D.run(lib, [], 0, 0) == []


def test_many_messages_on_the_host():
    L, lib = _lib()
    spans, exp = D.many_vectors()
    assert D.run(lib, spans, len(exp), 0) == exp


def test_debug_entry_refuses_bad_arguments():
    L, lib = _lib()
    import numpy as np
    sp = np.array([2, 0, 1], dtype=np.uint64)
    out = np.zeros(40, np.uint8)
    buf = D.pool()
    assert lib.lh264_debug_sha1(buf.ctypes.data, sp.ctypes.data, 1, 2, 0, out.ctypes.data) == L.E_ARG      # message 2 of 2
    assert lib.lh264_debug_sha1(buf.ctypes.data, sp.ctypes.data, 1, 3, 0, None) == L.E_ARG
    assert lib.lh264_debug_sha1(buf.ctypes.data, None, 1, 3, 0, out.ctypes.data) == L.E_ARG
    assert lib.lh264_debug_sha1(buf.ctypes.data, sp.ctypes.data, -1, 3, 0, out.ctypes.data) == L.E_ARG


def _opts(L, **kw):
    o = L.DecodeOpts()
    o.struct_bytes = C.sizeof(L.DecodeOpts)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_flag_rules_are_checked_before_the_device():
    import torch
    L, lib = _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    ptrs = (C.c_char_p * 1)(data)
    lens = (C.c_size_t * 1)(len(data))
    sentinel = 0x5a5a5a5a
    outs = (C.c_void_p * 1)(sentinel)

    @L.DECODE_SINK_FN
    def sink(*a):
        return 0
    P, S, N, DEV = L.DECODE_SHA1_PICTURES, L.DECODE_SHA1_STREAM, L.DECODE_NO_PICTURES, L.DECODE_DEVICE_OUT
    bad = [dict(flags=N), dict(flags=N | DEV), dict(flags=N | P | DEV), dict(flags=N | S | DEV), dict(flags=N | P | S | DEV),
           dict(flags=N | P, sink=sink), dict(flags=N | S, sink=sink), dict(flags=N | P | S, sink=sink), dict(flags=N, sink=sink),
           dict(flags=16), dict(flags=16 | P), dict(flags=2), dict(flags=2 | P), dict(flags=2 | N | S), dict(flags=64 | P), dict(flags=16 | N | S), dict(flags=128 | P | S), dict(flags=0x80000000 | P),
           dict(flags=P | DEV, sink=sink)]
    for kw in bad:
        assert lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(_opts(L, **kw)), outs) == L.E_ARG, kw
        assert outs[0] == sentinel
    if torch.cuda.is_available():
        return                       # (with a device the valid combinations decode: tests/test_digest_gpu.py)
    good = [dict(flags=P), dict(flags=S), dict(flags=P | S), dict(flags=P | DEV), dict(flags=S | DEV), dict(flags=P | S | DEV),
            dict(flags=P, sink=sink), dict(flags=S, sink=sink), dict(flags=P | S, sink=sink),
            dict(flags=N | P), dict(flags=N | S), dict(flags=N | P | S), dict(flags=N | P | S, format=L.FMT_NV12),
            dict(flags=P | S, struct_bytes=L.DECODE_OPTS_BYTES_V1)]
    for kw in good:
        assert lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(_opts(L, **kw)), outs) == L.E_NODEVICE, kw
        assert outs[0] == sentinel
    import losslessh264_amd as lh
    with pytest.raises(RuntimeError):
        lh.decode_batch([data], sha1="both", pictures=False)


def test_python_refuses_what_the_library_refuses():
    import losslessh264_amd as lh
    for kw in (dict(pictures=False), dict(pictures=False, sha1="stream", device_out=True), dict(pictures=False, sha1="both", sink=lambda *a: 0),
               dict(sha1="all")):
        with pytest.raises(ValueError):
            lh.decode_batch([b""], **kw)


def test_exports_and_constants():
    L, lib = _lib()
    for name in ("lh264_decoded_picture_sha1", "lh264_decoded_stream_sha1", "lh264_debug_sha1"):
        assert hasattr(lib, name) and name in L.EXPORTS, name
    txt = open(os.path.join(ROOT, "include", "lh264.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(LH264_DECODE_[A-Z0-9_]+)\s+(\d+)u\b", txt)}
    assert defs["LH264_DECODE_DEVICE_OUT"] == L.DECODE_DEVICE_OUT == 1
    assert defs["LH264_DECODE_SHA1_PICTURES"] == L.DECODE_SHA1_PICTURES == 4
    assert defs["LH264_DECODE_SHA1_STREAM"] == L.DECODE_SHA1_STREAM == 8
    assert defs["LH264_DECODE_NO_PICTURES"] == L.DECODE_NO_PICTURES == 32
    # the getters refuse a null handle / output
    import numpy as np
    out = np.zeros(20, np.uint8)
    assert lib.lh264_decoded_picture_sha1(None, 0, out.ctypes.data) == L.E_ARG
    assert lib.lh264_decoded_stream_sha1(None, out.ctypes.data) == L.E_ARG
