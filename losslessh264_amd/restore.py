"""Restore direction: default stream + tagged streams -> the original H.264 bytes (C ABI
lh264_pip_restore; host code, see csrc/host/pip_restore.h)."""
import ctypes as C

from . import _lib as L

N_TAG_IDS = 72


def restore(main, tags, size_hint=None):
    """main: bytes of the default stream; tags: {tag id: bytes}.  Returns the restored Annex-B stream."""
    lib = L.lib()
    ptrs = (C.c_char_p * N_TAG_IDS)()
    lens = (C.c_size_t * N_TAG_IDS)()
    for t, b in tags.items():
        if 0 <= t < N_TAG_IDS:
            ptrs[t] = bytes(b)
            lens[t] = len(b)
    cap = size_hint or (4 * (len(main) + sum(len(b) for b in tags.values())) + 4096)
    for _ in range(2):
        out = C.create_string_buffer(cap)
        n = C.c_size_t(0)
        rc = lib.lh264_pip_restore(bytes(main), len(main), ptrs, lens, N_TAG_IDS, out, cap, C.byref(n))
        if rc == 0:
            return out.raw[:n.value]
        if rc == -2 and n.value > cap:
            cap = n.value
            continue
        break
    raise RuntimeError("restore failed: " + lib.lh264_restore_error().decode())


RESTORE_ITEM = None


def _item_type():
    global RESTORE_ITEM
    if RESTORE_ITEM is None:
        class Item(C.Structure):
            _fields_ = [("main_stream", C.c_char_p), ("main_len", C.c_size_t), ("tags", C.POINTER(C.c_char_p)), ("tag_len", C.POINTER(C.c_size_t)),
                        ("n_tags", C.c_int32), ("status", C.c_int32), ("out", C.c_void_p), ("out_cap", C.c_size_t), ("out_len", C.c_size_t)]
        RESTORE_ITEM = Item
    return RESTORE_ITEM


def restore_batch(items, threads=0, out_cap=None):
    """items: list of (main bytes, {tag: bytes}) -> list of restored byte strings (None where a restore failed), one host
    thread per stream (C ABI lh264_pip_restore_batch)."""
    lib = L.lib()
    Item = _item_type()
    arr = (Item * len(items))()
    keep = []
    for i, (main, tags) in enumerate(items):
        ptrs = (C.c_char_p * N_TAG_IDS)()
        lens = (C.c_size_t * N_TAG_IDS)()
        for t, b in tags.items():
            if 0 <= t < N_TAG_IDS:
                ptrs[t] = bytes(b)
                lens[t] = len(b)
        cap = out_cap or (4 * (len(main) + sum(len(b) for b in tags.values())) + 4096)
        buf = C.create_string_buffer(cap)
        keep.append((ptrs, lens, buf))
        it = arr[i]
        it.main_stream, it.main_len, it.tags, it.tag_len, it.n_tags = bytes(main), len(main), ptrs, lens, N_TAG_IDS
        it.out, it.out_cap = C.addressof(buf), cap
    L.check(lib.lh264_pip_restore_batch(C.byref(arr), len(items), threads))
    return [keep[i][2].raw[:arr[i].out_len] if arr[i].status == 0 else None for i in range(len(items))]


PATH_DEVICE, PATH_HOST, PATH_FALLBACK = 0, 1, 2


def _restore_items(items, out_cap):
    Item = _item_type()
    arr = (Item * len(items))()
    keep = []
    for i, (main, tags) in enumerate(items):
        ptrs = (C.c_char_p * N_TAG_IDS)()
        lens = (C.c_size_t * N_TAG_IDS)()
        for t, b in tags.items():
            if 0 <= t < N_TAG_IDS:
                ptrs[t] = bytes(b)
                lens[t] = len(b)
        cap = out_cap or (4 * (len(main) + sum(len(b) for b in tags.values())) + 4096)
        buf = C.create_string_buffer(cap)
        keep.append((ptrs, lens, buf))
        it = arr[i]
        it.main_stream, it.main_len, it.tags, it.tag_len, it.n_tags = bytes(main), len(main), ptrs, lens, N_TAG_IDS
        it.out, it.out_cap = C.addressof(buf), cap
    return arr, keep


def _restore_batch_paths(name, items, threads, out_cap, statuses, cabac_device):
    """name: the C call without options, taken when no option is asked for; name + "_opts" otherwise"""
    arr, keep = _restore_items(items, out_cap)
    paths = (C.c_int32 * max(1, len(items)))()
    if cabac_device:
        opts = L.RestoreOpts(C.sizeof(L.RestoreOpts), threads, L.RESTORE_CABAC_DEVICE)
        L.check(getattr(L.lib(), name + "_opts")(C.byref(arr), len(items), C.byref(opts), paths))
    else:
        L.check(getattr(L.lib(), name)(C.byref(arr), len(items), threads, paths))
    outs = [keep[i][2].raw[:arr[i].out_len] if arr[i].status == 0 else None for i in range(len(items))]
    if statuses:
        return outs, [paths[i] for i in range(len(items))], [(arr[i].status, arr[i].out_len) for i in range(len(items))]
    return outs, [paths[i] for i in range(len(items))]


def restore_batch_device(items, threads=0, out_cap=None, statuses=False, cabac_device=False):
    """restore_batch on the current device (C ABI lh264_pip_restore_batch_device): CAVLC streams are decoded and written by the
    kernel, streams with CABAC slices by the host restore beside it - or, with cabac_device=True (lh264_pip_restore_batch_device_opts
    with LH264_RESTORE_CABAC_DEVICE), by the kernel too.  Returns (outs, paths): outs as restore_batch gives them, paths[i] one of
    PATH_DEVICE / PATH_HOST / PATH_FALLBACK.  statuses=True adds a third list of (status, out_len) per item.  Raises without a device."""
    return _restore_batch_paths("lh264_pip_restore_batch_device", items, threads, out_cap, statuses, cabac_device)


def restore_batch_cpu_check(items, threads=0, out_cap=None, statuses=False, cabac_device=False):
    """the kernel's code stepped on the host (lh264_debug_restore_cpu, lh264_debug_restore_cpu_opts): the same plan and results as
    restore_batch_device, for checking the device chain without a device"""
    return _restore_batch_paths("lh264_debug_restore_cpu", items, threads, out_cap, statuses, cabac_device)


def dp_update_device(words, bits):
    """the restore kernel's probability update on the device (lh264_debug_dp_update): uint32 words and 0 / 1 decisions -> uint32 words"""
    import numpy as np
    w = np.ascontiguousarray(words, dtype=np.uint32)
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    assert w.shape == b.shape and w.ndim == 1
    out = np.zeros(len(w), dtype=np.uint32)
    L.check(L.lib().lh264_debug_dp_update(w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(w)))
    return out


def restore_timing():
    """(pass 1, device stage, kernel, pass 2) in ms of the last restore_batch_device call"""
    ms = (C.c_double * 4)()
    L.check(L.lib().lh264_restore_last_timing(ms))
    return tuple(ms)


def restore_release():
    """frees the device and page-locked buffers restore_batch_device keeps between calls"""
    L.lib().lh264_restore_release()


VERBATIM = 1


def pack(main, tags, flags=0):
    """default stream + tagged streams (or, with VERBATIM, the input itself as `main`) -> one LHPIP1 container (C ABI lh264_pip_pack)"""
    lib = L.lib()
    ptrs = (C.c_char_p * N_TAG_IDS)()
    lens = (C.c_size_t * N_TAG_IDS)()
    for t, b in tags.items():
        if 0 <= t < N_TAG_IDS:
            ptrs[t] = bytes(b)
            lens[t] = len(b)
    cap = lib.lh264_pip_pack_bound(len(main), lens, N_TAG_IDS)
    out = C.create_string_buffer(cap)
    n = C.c_size_t(0)
    L.check(lib.lh264_pip_pack(bytes(main), len(main), ptrs, lens, N_TAG_IDS, flags, out, cap, C.byref(n)))
    return out.raw[:n.value]


def restore_file(blob, size_hint=None):
    """LHPIP1 container -> the original stream (C ABI lh264_pip_restore_file)"""
    lib = L.lib()
    cap = size_hint or (4 * len(blob) + 4096)
    for _ in range(2):
        out = C.create_string_buffer(cap)
        n = C.c_size_t(0)
        rc = lib.lh264_pip_restore_file(bytes(blob), len(blob), out, cap, C.byref(n))
        if rc == 0:
            return out.raw[:n.value]
        if rc == -2 and n.value > cap:
            cap = n.value
            continue
        break
    raise RuntimeError("restore failed: " + lib.lh264_restore_error().decode())


class CompressedBatch:
    """the handles lh264_compress_batch returned: results are copied out stream by stream on demand (the C call itself does not touch
    Python objects: `seconds` is its wall time)"""

    def __init__(self, handles, n, seconds):
        self._h, self.n, self.seconds = handles, n, seconds

    def result(self, i):
        """-> (main bytes, {tag: bytes}, error text or None) of stream i"""
        lib = L.lib()
        h = self._h[i]
        ln = C.c_size_t(0)
        p = lib.lh264_compressed_main(h, C.byref(ln))
        main = C.string_at(p, ln.value) if ln.value else b""
        tags = {}
        for t in range(N_TAG_IDS):
            p = lib.lh264_compressed_tag(h, t, C.byref(ln))
            if p:
                tags[t] = C.string_at(p, ln.value)
        err = None if lib.lh264_compressed_status(h) == 0 else lib.lh264_compressed_error(h).decode()
        return main, tags, err

    def status(self, i):
        return L.lib().lh264_compressed_status(self._h[i])

    def pictures(self, i):
        return L.lib().lh264_compressed_pictures(self._h[i])

    def segments(self, i):
        """in how many segments stream i was coded (1: whole; more: it was longer than segment_mbs)"""
        return L.lib().lh264_compressed_segments(self._h[i])

    def decisions(self, i, tag):
        """binary decisions coded into stream i's tag `tag`, summed over its segments"""
        return int(L.lib().lh264_compressed_decisions(self._h[i], tag))

    def free(self):
        lib = L.lib()
        for i in range(self.n):
            if self._h[i]:
                lib.lh264_compressed_free(self._h[i])
                self._h[i] = None
        self.n = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def compress_batch_handles(datas, threads=0, devices=None, segment_mbs=None, escapes=False, tolerant=False):
    """lh264_compress_batch_opts / lh264_compress_batch_devices_opts -> CompressedBatch (call .free() when done).  segment_mbs: streams of
    more macroblocks are coded in segments of at most that many (whole pictures); None: the library's default.  escapes: a stream with
    an mb_skip_run above 511 or 16 active references is compressed and gets the escape stream, tag 71 (LH264_COMPRESS_ESCAPES), instead
    of being refused.  tolerant: LH264_COMPRESS_TOLERANT - the default stream keeps the payload of every NAL unit that is no slice (see
    not_kept()), and a picture with macroblocks no slice covers is compressed instead of refusing the stream"""
    import time
    lib = L.lib()
    n = len(datas)
    ptrs = (C.c_char_p * n)(*[bytes(d) for d in datas])
    lens = (C.c_size_t * n)(*[len(d) for d in datas])
    outs = (C.c_void_p * n)()
    t0 = time.perf_counter()
    opts = L.CompressOpts(C.sizeof(L.CompressOpts), (L.COMPRESS_ESCAPES if escapes else 0) | (L.COMPRESS_TOLERANT if tolerant else 0), int(segment_mbs or 0))
    if devices:
        devs = (C.c_int * len(devices))(*devices)
        rc = lib.lh264_compress_batch_devices_opts(ptrs, lens, n, threads, devs, len(devices), C.byref(opts), outs)
    else:
        rc = lib.lh264_compress_batch_opts(ptrs, lens, n, threads, C.byref(opts), outs)
    dt = time.perf_counter() - t0
    L.check(rc)
    return CompressedBatch(outs, n, dt)


def compress_batch(datas, threads=0, devices=None, segment_mbs=None, escapes=False, tolerant=False):
    """the whole compress direction behind one C call (lh264_compress_batch): list of Annex-B byte strings ->
    list of (main bytes, {tag: bytes}, error text or None).  devices: list of device indices to shard the batch over
    (lh264_compress_batch_devices); default: the current device.  segment_mbs, escapes, tolerant: see compress_batch_handles"""
    b = compress_batch_handles(datas, threads, devices, segment_mbs, escapes, tolerant)
    res = [b.result(i) for i in range(b.n)]
    b.free()
    return res
