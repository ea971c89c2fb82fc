"""Host front end binding: Annex-B bytes -> list of frames (numpy views of the parser's records)."""
import ctypes as C

import numpy as np

from . import _lib as L


class ParsedFrame:
    pass


def parse_file(data, strict=False, pcm=False, escapes=False, conceal=None, tolerant=False):
    """A whole Annex-B file fed chunk by chunk as the reference's console application does.
    -> (frames, error_text, main_stream): main_stream is the recompressor's default stream (the '.pip' file itself).
    pcm=True: a fourth element, the samples of the stream's I_PCM macroblocks (stream LH264_TAG_PCM of the container).
    escapes=True: one more element at the end, the stream's escape stream (LH264_TAG_ESC, see escapes()).
    conceal: a name of decode_batch's conceal= (lh264_parser_set_conceal): macroblocks no slice covers get concealment records, and
    every frame says how many (concealed), from which picture (conceal_src, -1: 128s), whether it is withheld (frozen) and what the
    vector was made of (conceal_info, see lh264_parser_frame_conceal).  For the decode direction only.
    tolerant=True: lh264_parser_set_tolerant - the default stream keeps the payload of every NAL unit that is no slice (not_kept())."""
    return parse_stream(data, strict, _file=True, _pcm=pcm, _esc=escapes, _conceal=conceal, _tolerant=tolerant)


def parse_batch_time(datas, threads=0, keep=True):
    """parse a batch of Annex-B files on host threads and throw the records away -> (seconds, pictures parsed).
    keep=True: C ABI lh264_parse_batch (all pictures of all streams stay in memory until the end); keep=False:
    lh264_parse_batch_discard (a picture is released when complete: the steady state of a pipeline).  For bench.py."""
    import time
    lib = L.lib()
    n = len(datas)
    ptrs = (C.c_char_p * n)(*[bytes(d) for d in datas])
    lens = (C.c_size_t * n)(*[len(d) for d in datas])
    if not keep:
        pics = (C.c_int64 * n)()
        t0 = time.perf_counter()
        L.check(lib.lh264_parse_batch_discard(ptrs, lens, n, threads, pics))
        return time.perf_counter() - t0, int(sum(pics))
    outs = (C.c_void_p * n)()
    t0 = time.perf_counter()
    L.check(lib.lh264_parse_batch(ptrs, lens, n, threads, outs))
    dt = time.perf_counter() - t0
    pics = 0
    for i in range(n):
        pics += lib.lh264_parser_frame_count(outs[i])
        lib.lh264_parser_destroy(outs[i])
    return dt, pics


def _read_frame(lib, p, i):
    """picture i of parser p as a ParsedFrame"""
    info = np.zeros(1, dtype=L.FRAME_INFO_DTYPE)
    L.check(lib.lh264_parser_frame_info(p, i, info.ctypes.data_as(C.c_void_p)))
    fi = info[0]
    f = ParsedFrame()
    f.id, f.mb_w, f.mb_h, f.frame_num = int(fi["id"]), int(fi["mb_w"]), int(fi["mb_h"]), int(fi["frame_num"])
    f.crop_x, f.crop_y, f.crop_w, f.crop_h = int(fi["crop_x"]), int(fi["crop_y"]), int(fi["crop_w"]), int(fi["crop_h"])
    f.is_ref, f.idr = bool(fi["is_ref"]), bool(fi["idr"])
    f.ref_ids = [int(x) for x in fi["ref_ids"][:int(fi["n_refs"])]]
    n, ns = f.mb_w * f.mb_h, int(fi["n_slices"])

    def arr(ptr, nbytes, dtype):
        return np.frombuffer(C.string_at(ptr, nbytes), dtype=dtype).copy()
    f.mbs = arr(lib.lh264_parser_frame_mbs(p, i), n * 128, L.MB_DTYPE)
    f.coeffs = arr(lib.lh264_parser_frame_coeffs(p, i), n * 768, "<i2").reshape(n, 384)
    f.levels = arr(lib.lh264_parser_frame_levels(p, i), n * 768, "<i2").reshape(n, 384)
    f.slices = arr(lib.lh264_parser_frame_slices(p, i), ns * 232, L.SLICE_DTYPE)
    f.covered = arr(lib.lh264_parser_frame_covered(p, i), n, np.uint8)
    f.syn = arr(lib.lh264_parser_frame_syntax(p, i), n * 116, L.MBSYN_DTYPE)
    f.slice_syn = arr(lib.lh264_parser_frame_slice_syntax(p, i), ns * 16, "<i4").reshape(ns, 4)
    cnt = C.c_int(0)
    ptr = lib.lh264_parser_frame_syn_symbols(p, i, C.byref(cnt))
    f.syn_syms = arr(ptr, cnt.value * 8, L.CTX_SYM_DTYPE) if cnt.value else np.zeros(0, L.CTX_SYM_DTYPE)
    f.syn_off = arr(lib.lh264_parser_frame_syn_offsets(p, i), (n + 1) * 4, "<u4")
    ci = np.zeros(12, dtype="<i4")
    L.check(lib.lh264_parser_frame_conceal(p, i, ci.ctypes.data_as(C.c_void_p)))
    f.concealed, f.conceal_src, f.frozen, f.conceal_info, f.poc = int(ci[0]), int(ci[1]), bool(ci[2]), ci, int(ci[11])
    return f


def parse_stream(data, strict=False, _file=False, _pcm=False, _esc=False, _conceal=None, _tolerant=False):
    """-> (frames, error_text).  frames have the attributes ReconSession / CtxSession expect."""
    lib = L.lib()
    p = lib.lh264_parser_create()
    try:
        if _conceal is not None:
            if _conceal not in L.CONCEAL:
                raise ValueError("conceal must be one of %s" % ", ".join(sorted(L.CONCEAL)))
            L.check(lib.lh264_parser_set_conceal(p, L.CONCEAL[_conceal]))
        if _tolerant:
            L.check(lib.lh264_parser_set_tolerant(p, 1))
        if _file:
            rc = lib.lh264_parser_feed_file(p, bytes(data), len(data))
        else:
            rc = lib.lh264_parser_feed(p, bytes(data), len(data), 1)
        err = lib.lh264_parser_error(p).decode()
        if rc != 0 and strict:
            raise RuntimeError("h264 parse error: " + err)
        frames = [_read_frame(lib, p, i) for i in range(lib.lh264_parser_frame_count(p))]
        if _file:
            ln = C.c_size_t(0)
            ptr = lib.lh264_parser_main_stream(p, C.byref(ln))
            main = C.string_at(ptr, ln.value) if ln.value else b""
            out = (frames, err, main)
            if _pcm:
                ptr = lib.lh264_parser_pcm_samples(p, C.byref(ln))
                out += (C.string_at(ptr, ln.value) if ln.value else b"",)
            if _esc:
                ptr = lib.lh264_parser_escapes(p, C.byref(ln))
                out += (C.string_at(ptr, ln.value) if ln.value else b"",)
            return out
        return frames, err
    finally:
        lib.lh264_parser_destroy(p)


def out_of_range(data):
    """'' or why compress_batch refuses a stream that parses: the first syntax value the container's prior tables cannot carry
    (lh264_parser_out_of_range), e.g. "mb_skip_run 687 is outside the container's range 0..511".  No device is needed."""
    lib = L.lib()
    p = lib.lh264_parser_create()
    try:
        lib.lh264_parser_feed_file(p, bytes(data), len(data))
        return lib.lh264_parser_out_of_range(p).decode()
    finally:
        lib.lh264_parser_destroy(p)


def pick(data, which):
    """the decode-order indices of the pictures decode_batch (pick=which) selects from one Annex-B stream, up to the first failure of the
    header walk (lh264_parser_pick): which = "all" | "intra" (every slice an I slice) | "idr".  Headers only; no device is needed."""
    if which not in L.PICK:
        raise ValueError("which must be 'all', 'intra' or 'idr'")
    lib = L.lib()
    data = bytes(data)
    n = C.c_int(0)
    L.check(lib.lh264_parser_pick(data, len(data), L.PICK[which], None, 0, C.byref(n)))
    idx = (C.c_int32 * max(1, n.value))()
    L.check(lib.lh264_parser_pick(data, len(data), L.PICK[which], idx, n.value, C.byref(n)))
    return [int(idx[k]) for k in range(n.value)]


def stream_colour(data):
    """what the first SPS of an Annex-B stream says about colour (lh264_parser_colour; no device is needed) -> (matrix_coefficients,
    full_range, present): matrix_coefficients 2 (unspecified) and full_range False where the SPS carries none; present bit 0 = its VUI
    has a video_signal_type, bit 1 = a colour description.  None: no SPS that parses"""
    data = bytes(data)
    mc, fr, pr = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = L.lib().lh264_parser_colour(data, len(data), C.byref(mc), C.byref(fr), C.byref(pr))
    if rc == L.E_UNSUPPORTED:
        return None
    L.check(rc)
    return mc.value, bool(fr.value), pr.value


def _file_text(data, query, tolerant=False):
    lib = L.lib()
    p = lib.lh264_parser_create()
    try:
        if tolerant:
            L.check(lib.lh264_parser_set_tolerant(p, 1))
        lib.lh264_parser_feed_file(p, bytes(data), len(data))
        return getattr(lib, query)(p).decode()
    finally:
        lib.lh264_parser_destroy(p)


def not_kept(data):
    """'' or a text naming the first NAL unit whose bytes the default stream does not keep without tolerant=True (lh264_parser_not_kept):
    compress_batch answers LH264_OK for such a stream and the result does not restore; with tolerant=True it does.  No device is needed."""
    return _file_text(data, "lh264_parser_not_kept")


def not_carried(data):
    """'' or a text naming the first NAL unit that the default stream cannot carry even with tolerant=True (lh264_parser_not_carried): a
    slice in front of its parameter sets, a unit with the forbidden bit set.  compress_batch(tolerant=True) refuses the stream with it."""
    return _file_text(data, "lh264_parser_not_carried", True)


def escapes(data):
    """b'' or the escape stream of a stream that parses (lh264_parser_escapes): tag 71 of the container, the part of every mb_skip_run
    above 511 and of 16 active references that the prior tables drop.  Empty when out_of_range(data) is, and when the stream has a value the
    escape stream cannot carry (more than 16 references, a value of another table: such a stream stays refused).  No device is needed."""
    lib = L.lib()
    p = lib.lh264_parser_create()
    try:
        lib.lh264_parser_feed_file(p, bytes(data), len(data))
        ln = C.c_size_t(0)
        ptr = lib.lh264_parser_escapes(p, C.byref(ln))
        return C.string_at(ptr, ln.value) if ln.value else b""
    finally:
        lib.lh264_parser_destroy(p)


def parse_file_segments(data, segment_mbs):
    """a file parsed in pieces (lh264_parser_begin_file / lh264_parser_feed_file_some / lh264_parser_drop_frames): yields lists of
    frames - whole pictures, at most segment_mbs macroblocks a list but one picture at least - and at last the tuple
    (error text, default stream).  The parser never holds more than a segment and a picture"""
    lib = L.lib()
    p = lib.lh264_parser_create()
    data = bytes(data)
    try:
        L.check(lib.lh264_parser_begin_file(p, data, len(data)))
        done = False
        while True:
            if not done:
                done = lib.lh264_parser_feed_file_some(p, segment_mbs) == 1
            n = lib.lh264_parser_frame_count(p)
            if n == 0:
                if done:
                    break
                continue
            seg, m = [], 0
            for i in range(n):
                f = _read_frame(lib, p, i)
                if seg and m + f.mb_w * f.mb_h > segment_mbs:
                    break
                seg.append(f)
                m += f.mb_w * f.mb_h
            L.check(lib.lh264_parser_drop_frames(p, len(seg)))
            yield seg
        ln = C.c_size_t(0)
        ptr = lib.lh264_parser_main_stream(p, C.byref(ln))
        yield lib.lh264_parser_error(p).decode(), (C.string_at(ptr, ln.value) if ln.value else b"")
    finally:
        lib.lh264_parser_destroy(p)
