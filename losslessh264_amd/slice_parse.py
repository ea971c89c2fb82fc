"""Slice data apart from the header walk: the parser's deferred mode and the code that parses slice data for the device
(csrc/lh264_slice.h for CAVLC, csrc/lh264_slice_cabac.h for CABAC), stepped on the host or run by slice_parse_kernel /
slice_parse_cabac_kernel.  Checks and probes; not a decode path."""
import ctypes as C

import numpy as np

from . import _lib as L
from .parse import _read_frame


class ParsedFile:
    """frames, error text, file status, error_pictures; in deferred mode per picture the (slice index, ok, stop bit) of its deferred
    slices, and in deferred_cabac per picture whether each of them is a CABAC slice"""


def parse_file_plain(data, deferred=False, cabac=False):
    """the host front end over a whole file.  deferred=True: every CAVLC slice is deferred (lh264_parser_set_defer_slice_data) and then
    parsed by lh264_parser_parse_deferred, picture by picture and slice by slice: what comes out must be what deferred=False gives.
    cabac=True (with deferred=True): the CABAC slices are deferred as well (lh264_parser_set_defer_cabac)"""
    lib = L.lib()
    p = lib.lh264_parser_create()
    try:
        if deferred:
            L.check(lib.lh264_parser_set_defer_slice_data(p, 1))
        if cabac:
            L.check(lib.lh264_parser_set_defer_cabac(p, 1))
        lib.lh264_parser_feed_file(p, bytes(data), len(data))
        r = ParsedFile()
        r.deferred, r.deferred_cabac = [], []
        n = lib.lh264_parser_frame_count(p)
        for i in range(n):
            got = []
            r.deferred_cabac.append([lib.lh264_parser_frame_deferred_cabac(p, i, s) == 1 for s in range(lib.lh264_parser_frame_deferred(p, i))])
            for s in range(lib.lh264_parser_frame_deferred(p, i)):
                out = (C.c_int32 * 2)()
                ok = lib.lh264_parser_parse_deferred(p, i, s, out)
                got.append((int(out[0]), ok == 1, int(out[1])))
            r.deferred.append(got)
        r.frames = [_read_frame(lib, p, i) for i in range(n)]
        r.error = lib.lh264_parser_error(p).decode()
        r.status = lib.lh264_parser_file_status(p)
        r.error_pictures = int(lib.lh264_parser_error_pictures(p))
        return r
    finally:
        lib.lh264_parser_destroy(p)


class SlicePicture:
    pass


def slice_parse(data, on_device=False, threads=0, tweak=None, cabac=False):
    """lh264_debug_slice_parse_opts -> (pictures, guards intact, the header walk's error text).  A picture has mb_w, mb_h, mbs, coeffs
    (n x 384), slices and results: per slice (deferred, status, n_mbs, stop_bit).  tweak: (picture, slice, limit_mb) or (picture, slice,
    limit_mb, the task's entropy-mode byte).  cabac=True: CABAC slices are deferred and walked too (csrc/lh264_slice_cabac.h)"""
    lib = L.lib()
    h = C.c_void_p()
    tw = (C.c_int32 * 4)(*(tuple(tweak) + (-1,))[:4]) if tweak is not None else None
    flags = (L.SLICE_PARSE_ON_DEVICE if on_device else 0) | (L.SLICE_PARSE_CABAC if cabac else 0)
    rc = lib.lh264_debug_slice_parse_opts(bytes(data), len(data), flags, threads, tw, C.byref(h))
    if rc != 0:
        raise RuntimeError("lh264_debug_slice_parse_opts: error %d" % rc)
    try:
        pics = []
        for i in range(lib.lh264_slice_dump_pictures(h)):
            info = (C.c_int32 * 4)()
            L.check(lib.lh264_slice_dump_picture(h, i, info))
            q = SlicePicture()
            q.mb_w, q.mb_h, ns, q.n_deferred = [int(x) for x in info]
            n = q.mb_w * q.mb_h

            def arr(ptr, nbytes, dtype):
                return np.frombuffer(C.string_at(ptr, nbytes), dtype=dtype).copy() if nbytes else np.zeros(0, dtype)
            q.mbs = arr(lib.lh264_slice_dump_mbs(h, i), n * 128, L.MB_DTYPE)
            q.coeffs = arr(lib.lh264_slice_dump_coeffs(h, i), n * 768, "<i2").reshape(n, 384)
            q.slices = arr(lib.lh264_slice_dump_slices(h, i), ns * 232, L.SLICE_DTYPE)
            q.results = arr(lib.lh264_slice_dump_results(h, i), ns * 16, "<i4").reshape(ns, 4)
            pics.append(q)
        return pics, lib.lh264_slice_dump_guards_ok(h) == 1, lib.lh264_slice_dump_error(h).decode()
    finally:
        lib.lh264_slice_dump_free(h)
