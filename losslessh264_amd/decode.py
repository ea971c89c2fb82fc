"""The decode direction behind one C call (lh264_decode_batch): Annex-B streams -> their pictures, cropped and packed as I420 or
NV12, as host bytes, as device tensors or through a sink.  ctypes only; torch is device-buffer plumbing."""
import ctypes as C
import os

import numpy as np

from . import _lib as L

_FORMATS = {"i420": L.FMT_I420, "nv12": L.FMT_NV12}
_SHA1 = {None: 0, "pictures": L.DECODE_SHA1_PICTURES, "stream": L.DECODE_SHA1_STREAM, "both": L.DECODE_SHA1_PICTURES | L.DECODE_SHA1_STREAM}


class _DevSpan:
    """a run of device bytes owned by a decode handle, described the way torch.as_tensor reads it"""

    def __init__(self, ptr, n, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None}


class DecodedBatch:
    """the handles of one decode_batch call; free() gives them back (device tensors made by tensor() are copies or views, see there)"""

    def __init__(self, lib, handles, device_out, sink_keepalive=None, size=None, colour=None, dtype="uint8", affine=None, motion=False, filter="area"):
        self._lib, self._h, self.device_out, self._keep, self.size, self.colour = lib, handles, device_out, sink_keepalive, size, colour
        self.filter = filter                   # the filter= of the call: "area" | "bilinear" | "bicubic"
        self.has_motion = bool(motion)
        # dtype: the dtype= of the call; affine: the six binary32 values it passed, ((mul R, G, B), (add R, G, B)), None with "uint8"
        self.dtype, self.affine = dtype, affine

    def __len__(self):
        return len(self._h)

    def status(self, i):
        return self._lib.lh264_decoded_status(self._h[i])

    def parse_path(self, i):
        """how stream i's slice data was parsed: "host" | "device" | "fallback" (decode_batch (parse="device"): a slice got a status from
        the kernel, its round was parsed again by the host parser and the stream stayed there)"""
        return L.PARSE_PATH[self._lib.lh264_decoded_parse_path(self._h[i])]

    def device_slices(self, i):
        """how many slices of stream i slice_parse_kernel parsed (0 on the host route)"""
        return int(self._lib.lh264_decoded_device_slices(self._h[i]))

    def device_cabac_slices(self, i):
        """... and how many of them were CABAC slices, parsed by slice_parse_cabac_kernel (parse="device+cabac")"""
        return int(self._lib.lh264_decoded_device_cabac_slices(self._h[i]))

    def parsed_slices(self, i):
        """the distinct slices of stream i whose slice data was parsed, by the host front end or by a kernel: with pick= the slices of
        the selected pictures only (an unselected picture is walked by its headers)"""
        return int(self._lib.lh264_decoded_parsed_slices(self._h[i]))

    def chain_pictures(self, i):
        """the pictures of stream i that were reconstructed, delivered or not: with select= the needed pictures (0 in the motion-only call)"""
        return int(self._lib.lh264_decoded_chain_pictures(self._h[i]))

    def picture_indices(self, i):
        """per delivered picture of stream i: its number among all pictures of the stream, in decode order from 0 (with pick="all" and
        nothing withheld: 0, 1, 2, ...)"""
        return [self._lib.lh264_decoded_picture_index(self._h[i], k) for k in range(self._lib.lh264_decoded_pictures(self._h[i]))]

    def error(self, i):
        return self._lib.lh264_decoded_error(self._h[i]).decode()

    def pictures(self, i):
        """[(width, height, frame_num, idr, offset, bytes)] of stream i, in decode order"""
        n = self._lib.lh264_decoded_pictures(self._h[i])
        out = []
        rec = np.zeros(1, dtype=L.DECODED_PIC_DTYPE)
        for k in range(n):
            L.check(self._lib.lh264_decoded_picture(self._h[i], k, rec.ctypes.data_as(C.c_void_p)))
            r = rec[0]
            out.append((int(r["width"]), int(r["height"]), int(r["frame_num"]), int(r["idr"]), int(r["offset"]), int(r["bytes"])))
        return out

    def concealed(self, i):
        """per delivered picture of stream i: the number of its macroblocks that were concealed (all 0 without conceal=)"""
        return [self._lib.lh264_decoded_concealed(self._h[i], k) for k in range(self._lib.lh264_decoded_pictures(self._h[i]))]

    def source_sizes(self, i):
        """[(width, height)] per delivered picture of stream i: its cropped window before scaling (= its size with scale=0)"""
        out = []
        w, h = C.c_int32(0), C.c_int32(0)
        for k in range(self._lib.lh264_decoded_pictures(self._h[i])):
            L.check(self._lib.lh264_decoded_picture_source_size(self._h[i], k, C.byref(w), C.byref(h)))
            out.append((w.value, h.value))
        return out

    def views(self, i):
        """[(src, dst)] per delivered picture of stream i, each an (x, y, w, h): the source rectangle in the picture's window - the
        caller's crop, narrowed by fit="cover" - and the destination rectangle in the delivered picture (the letterboxed part under
        fit="contain").  Without crop= and fit=: (0, 0, w, h) of the window and (0, 0, width, height) of what is delivered"""
        out = []
        s, d = L.Rect(), L.Rect()
        for k in range(self._lib.lh264_decoded_pictures(self._h[i])):
            L.check(self._lib.lh264_decoded_picture_view(self._h[i], k, C.byref(s), C.byref(d)))
            out.append(((s.x, s.y, s.w, s.h), (d.x, d.y, d.w, d.h)))
        return out

    def colours(self, i):
        """colour="rgb24" | "rgbp": [(matrix, colour_range)] per delivered picture of stream i, the standard that was applied to it -
        matrix "bt601" | "bt709", colour_range "limited" | "full" (what the stream's SPS says, or what the call named)"""
        if self.colour is None:
            raise RuntimeError("decode_batch was not called with colour=")
        out = []
        m, f = C.c_uint32(0), C.c_int32(0)
        for k in range(self._lib.lh264_decoded_pictures(self._h[i])):
            L.check(self._lib.lh264_decoded_picture_colour(self._h[i], k, C.byref(m), C.byref(f)))
            out.append(("bt709" if m.value == L.MATRIX["bt709"] else "bt601", "full" if f.value else "limited"))
        return out

    def picture_sha1(self, i):
        """sha1="pictures" | "both": the SHA-1 of every delivered picture of stream i, as delivered (20-byte bytes objects)"""
        out = []
        buf = (C.c_uint8 * 20)()
        for k in range(self._lib.lh264_decoded_pictures(self._h[i])):
            L.check(self._lib.lh264_decoded_picture_sha1(self._h[i], k, buf))
            out.append(bytes(buf))
        return out

    def stream_sha1(self, i):
        """sha1="stream" | "both": the SHA-1 of all delivered pictures of stream i, one behind the other (20 bytes)"""
        buf = (C.c_uint8 * 20)()
        L.check(self._lib.lh264_decoded_stream_sha1(self._h[i], buf))
        return bytes(buf)

    def data(self, i):
        """the packed pictures of stream i as bytes (empty with device_out=True, a sink or pictures=False)"""
        ln = C.c_size_t(0)
        ptr = self._lib.lh264_decoded_bytes(self._h[i], C.byref(ln))
        return C.string_at(ptr, ln.value) if ptr and ln.value else b""

    def tensor(self, i):
        """device_out=True: the packed pictures of stream i as a torch.uint8 tensor on the device.  Zero-copy where torch.as_tensor
        takes __cuda_array_interface__ (it does on the torch this was written against, ROCm builds included): the tensor is a VIEW of
        the handle's memory, valid until free() - clone() it to keep it longer.  Where torch refuses the interface the bytes are
        copied device-to-device into a fresh tensor (lh264_decoded_copy_dev); `zero_copy` tells which happened last."""
        import torch
        if not self.device_out:
            raise RuntimeError("decode_batch was not called with device_out=True")
        ln = C.c_size_t(0)
        ptr = self._lib.lh264_decoded_bytes_dev(self._h[i], C.byref(ln))
        dev = torch.device("cuda", torch.cuda.current_device())
        if not ptr or not ln.value:
            return torch.empty(0, dtype=torch.uint8, device=dev)
        try:
            t = torch.as_tensor(_DevSpan(ptr, ln.value, self), device=dev)
            self.zero_copy = t.data_ptr() == ptr
            return t
        except (TypeError, RuntimeError, ValueError):
            t = torch.empty(ln.value, dtype=torch.uint8, device=dev)
            L.check(self._lib.lh264_decoded_copy_dev(self._h[i], t.data_ptr(), ln.value))
            self.zero_copy = False
            return t

    def frames(self, i):
        """device_out=True together with size=(W, H): the pictures of stream i as a (pictures, H * 3 // 2, W) torch.uint8 view of
        tensor(i) - rows 0..H-1 of a picture are its luma plane, the H / 2 rows behind them its chroma bytes as packed (I420: Cb then
        Cr, two chroma rows per row of the view; NV12: the interleaved rows).  Every stream of the batch has the same picture shape.
        With colour="rgb24" the view is (pictures, H, W, 3), with colour="rgbp" (pictures, 3, H, W); with a float dtype= it has that
        dtype (torch.float32 | float16 | bfloat16): tensor(i) stays the uint8 bytes, this is tensor(i).view(dtype) in the same shape"""
        if not self.device_out or self.size is None:
            raise RuntimeError("frames() needs decode_batch (device_out=True, size=(W, H))")
        w, h = self.size
        t = self.tensor(i)
        if self.dtype != "uint8":
            import torch
            t = t.view({"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[self.dtype])
        if self.colour == "rgb24":
            return t.view(t.numel() // (w * h * 3), h, w, 3)
        if self.colour == "rgbp":
            return t.view(t.numel() // (w * h * 3), 3, h, w)
        return t.view(t.numel() // (w * h * 3 // 2), h * 3 // 2, w)      # (a stream that delivered nothing: 0 pictures)

    def motion_geometry(self, i):
        """motion=True: [(mb_w, mb_h, crop_x, crop_y, motion_offset, info_offset)] per delivered picture of stream i: the coded picture in
        macroblocks, where the delivered window begins in it (luma sample (x, y) of the window lies in cell ((crop_x + x) >> 2,
        (crop_y + y) >> 2)), and the byte offsets of the picture's two blocks in the stream's two buffers"""
        if not self.has_motion:
            raise RuntimeError("decode_batch was not called with motion=True")
        out = []
        g = L.DecodedMotion()
        for k in range(self._lib.lh264_decoded_pictures(self._h[i])):
            L.check(self._lib.lh264_decoded_picture_motion(self._h[i], k, C.byref(g)))
            out.append((g.mb_w, g.mb_h, g.crop_x, g.crop_y, int(g.motion_offset), int(g.info_offset)))
        return out

    def _field_buffers(self, i):
        """stream i's two field buffers: numpy int16 / uint8 arrays (copies) on the host, torch views of the handle's device memory
        (copies where torch refuses the interface) under device_out=True"""
        if not self.has_motion:
            raise RuntimeError("decode_batch was not called with motion=True")
        mp, ip, mn, inn = C.c_void_p(0), C.c_void_p(0), C.c_size_t(0), C.c_size_t(0)
        if not self.device_out:
            L.check(self._lib.lh264_decoded_motion(self._h[i], C.byref(mp), C.byref(mn), C.byref(ip), C.byref(inn)))
            mot = np.frombuffer(C.string_at(mp.value, mn.value), dtype="<i2") if mp.value and mn.value else np.zeros(0, "<i2")
            mbi = np.frombuffer(C.string_at(ip.value, inn.value), dtype=np.uint8) if ip.value and inn.value else np.zeros(0, np.uint8)
            return mot, mbi
        import torch
        L.check(self._lib.lh264_decoded_motion_dev(self._h[i], C.byref(mp), C.byref(mn), C.byref(ip), C.byref(inn)))
        dev = torch.device("cuda", torch.cuda.current_device())
        if not mp.value or not mn.value:
            return torch.empty(0, dtype=torch.int16, device=dev), torch.empty(0, dtype=torch.uint8, device=dev)
        try:
            mot = torch.as_tensor(_DevSpan(mp.value, mn.value, self), device=dev)
            mbi = torch.as_tensor(_DevSpan(ip.value, inn.value, self), device=dev)
        except (TypeError, RuntimeError, ValueError):
            mot, mbi = self.motion_copy(i)
        return mot.view(torch.int16), mbi

    def motion_copy(self, i):
        """motion=True with device_out=True: stream i's two field buffers copied device-to-device into fresh torch.uint8 tensors
        (lh264_decoded_motion_copy_dev) -> (motion bytes, macroblock bytes)"""
        import torch
        if not self.has_motion or not self.device_out:
            raise RuntimeError("motion_copy() needs decode_batch (motion=True, device_out=True)")
        mn, inn = C.c_size_t(0), C.c_size_t(0)
        L.check(self._lib.lh264_decoded_motion_dev(self._h[i], None, C.byref(mn), None, C.byref(inn)))
        dev = torch.device("cuda", torch.cuda.current_device())
        mot, mbi = torch.empty(mn.value, dtype=torch.uint8, device=dev), torch.empty(inn.value, dtype=torch.uint8, device=dev)
        L.check(self._lib.lh264_decoded_motion_copy_dev(self._h[i], mot.data_ptr() if mn.value else None, mn.value, mbi.data_ptr() if inn.value else None, inn.value))
        return mot, mbi

    def _field_list(self, i, which):
        mot, mbi = self._field_buffers(i)
        out = []
        for (mb_w, mb_h, _cx, _cy, mo, io) in self.motion_geometry(i):
            if which == 0:
                out.append(mot[mo // 2:mo // 2 + 48 * mb_w * mb_h].reshape(3, 4 * mb_h, 4 * mb_w))
            else:
                out.append(mbi[io:io + 8 * mb_w * mb_h].reshape(8, mb_h, mb_w))
        return out

    def motion(self, i):
        """motion=True: per delivered picture of stream i a (3, 4 * mb_h, 4 * mb_w) int16 array over the CODED picture's 4x4 blocks -
        [0] dx, [1] dy in quarter-pel (the final vectors, for P_Skip the inferred one), [2] how many pictures back in decode order the
        block predicts from (-1: no decoded picture); all three 0 in intra and uncovered macroblocks.  numpy on the host, torch views of
        the handle's device memory (valid until free()) under device_out=True.  The definition: include/lh264.h at lh264_decode_batch_ex4"""
        return self._field_list(i, 0)

    def mb_info(self, i):
        """motion=True: per delivered picture of stream i an (8, mb_h, mb_w) uint8 array - [0] kind (0 not covered, 1 I4x4, 2 I8x8,
        3 I16x16, 4 I_PCM, 5 P_Skip, 6 P16x16, 7 P16x8, 8 P8x16, 9 P8x8, 10 P8x8ref0), [1] qp_y, [2] cbp, [3] flags (bit 0 the 8x8
        transform, bit 1 concealed), [4..7] the sub-macroblock types of kinds 9 and 10"""
        return self._field_list(i, 1)

    def _field_frames(self, i, which):
        geo = self.motion_geometry(i)
        if len({(g[0], g[1]) for g in geo}) > 1:
            raise ValueError("stream %d changes its size: use motion(i) / mb_info(i)" % i)
        mot, mbi = self._field_buffers(i)
        mb_w, mb_h = (geo[0][0], geo[0][1]) if geo else (0, 0)
        if which == 0:
            return mot.reshape(len(geo), 3, 4 * mb_h, 4 * mb_w)
        return mbi.reshape(len(geo), 8, mb_h, mb_w)

    def motion_frames(self, i):
        """motion=True: motion(i) as one (pictures, 3, 4 * mb_h, 4 * mb_w) array or device view; ValueError where the stream changes size"""
        return self._field_frames(i, 0)

    def mb_info_frames(self, i):
        """motion=True: mb_info(i) as one (pictures, 8, mb_h, mb_w) array or device view; ValueError where the stream changes size"""
        return self._field_frames(i, 1)

    def free(self):
        for h in self._h:
            self._lib.lh264_decoded_free(h)
        self._h = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def decode_batch(datas, fmt="i420", threads=0, device_out=False, round_pictures=None, group_mbs=None, sink=None, conceal=None, sha1=None, pictures=True, parse="host", scale=0, pick="all", size=None, colour=None, matrix="auto", colour_range="auto", dtype="uint8", mul=None, add=None, fit="stretch", fill=None, crop=None, motion=False, select=None, filter="area"):
    """decode a batch of Annex-B streams on the current device -> DecodedBatch.
    fmt: "i420" | "nv12".  device_out=True: the pictures stay in device memory (tensor(i)).  sink: a callable
    (stream, first_picture, pictures, data) -> falsy to go on, called with runs of consecutive pictures of one stream (pictures as in
    DecodedBatch.pictures, data a bytes object); the handles then keep no bytes.  round_pictures / group_mbs: the cuts of the work
    (None = the library's defaults); the bytes do not depend on them.
    conceal: None / "off" (a picture with macroblocks no slice covers stops its stream) or how such macroblocks are concealed, as the
    reference's decoder does under the ERROR_CON_IDC of that name: "slice_copy" | "slice_copy_cross_idr" | "mv_copy" (slice MV copy
    across IDR) | "slice_copy_cross_idr_freeze" | "mv_copy_freeze" (the FREEZE_RES_CHANGE variants: pictures are withheld until the
    first whole IDR picture).  DecodedBatch.concealed(i) counts the concealed macroblocks per picture.
    sha1: None | "pictures" | "stream" | "both": SHA-1 digests computed on the device, of every delivered picture
    (DecodedBatch.picture_sha1) and / or of all delivered pictures of a stream in order (stream_sha1: for "i420" the number the
    reference's decoder test keeps per stream).  pictures=False (with sha1): digests only, no picture leaves the device.
    parse: "host" (the default) | "device": CAVLC slice data is parsed on the device by slice_parse_kernel, one wave per slice; the host
    walks headers only.  "device+cabac": CABAC slice data as well, by slice_parse_cabac_kernel, so that a stream stays on the device route
    through its CABAC pictures.  The bytes are the same; DecodedBatch.parse_path(i) tells the route each stream took.
    scale: 0 (full size) | 1 | 2 | 3 = s: reduced-size pictures, averaged on the device (decode_pack_scaled_kernel).  B = 1 << s.  For a
    picture whose cropped window is w x h (both even), cw = w / 2 and ch = h / 2: the delivered chroma size is ocw = ceil (cw / B),
    och = ceil (ch / B), the delivered luma size ow = 2 * ocw, oh = 2 * och.  Delivered luma sample (X, Y) =
    (sum + (1 << (2*s - 1))) >> (2*s), sum over the B x B window samples at x = min (X*B + i, w - 1), y = min (Y*B + j, h - 1),
    0 <= i, j < B; Cb and Cr: the same rule on their cw x ch planes.  Coordinates are clamped to the cropped window, never to the padded
    picture.  The planes are averaged independently; chroma siting is not modelled.  Packing as ever with ow, oh in place of w, h;
    DecodedBatch.pictures describes what is delivered, source_sizes the windows before scaling.  QCIF at scale=3: 22 x 18, 594 bytes.
    pick: "all" (the default) | "intra" | "idr": only the selected pictures are decoded and delivered - "intra": the pictures whose
    slices are all I slices, "idr": the IDR pictures.  Each is byte for byte that picture of the full decode; of the others the front end
    walks the headers only and never sees the slice data, so damage there is neither seen nor reported.  DecodedBatch.picture_indices(i)
    gives the delivered pictures' numbers in the stream, parsed_slices(i) what was parsed.  Not together with conceal.
    size: None | (W, H), both even ints in 2..4096, not together with scale: every delivered picture of every stream is W x H, resampled
    from its cropped window by an exact, integer area average on the device (decode_pack_resized_kernel).  Each plane on its own: luma
    from w x h to W x H, Cb and Cr from w/2 x h/2 to W/2 x H/2.  For a plane of w x h samples p[y][x] delivered as ow x oh: the weight of
    source column x for delivered column X is wx (X, x) = max (0, min ((x+1)*ow, (X+1)*w) - max (x*ow, X*w)) (non-zero for x in
    X*w // ow .. ((X+1)*w - 1) // ow, the weights of one X sum to w), wy (Y, y) the same with h, oh; S = the sum of wy * wx * p[y][x],
    D = w*h, delivered sample = (2*S + D) // (2*D): round half up, exact.  No coordinate leaves the window; the aspect ratio is not
    kept; chroma siting is not modelled.  size == the window gives the window, a window of B times the size (B = 2, 4, 8) the bytes of
    scale = 1, 2, 3; a larger size repeats samples and blends the seams.  pictures / the sink / the digests describe what is
    delivered, source_sizes the windows; with device_out=True, DecodedBatch.frames(i) is a (pictures, H * 3 // 2, W) view.
    colour: None | "rgb24" | "rgbp", with fmt="i420" only: RGB pictures, colour-converted on the device in the pack pass
    (decode_pack_rgb_kernel through lh264_decode_batch_ex; no I420 intermediate).  The conversion acts on the delivered planes - the
    window, its scale= means or its size= resampling, exactly as without colour - and converts every luma sample (X, Y) with the chroma
    sample (X >> 1, Y >> 1): the RGB bytes are an exact integer function (include/lh264.h, LH264_COLOUR_FACTORS) of the I420 bytes of
    the same call without colour.  "rgb24": H rows of W pixels stored R, G, B; "rgbp": three W x H planes R, G, B; 3*W*H bytes a
    picture, one behind the other.  matrix: "auto" (the SPS VUI's matrix_coefficients: 1 is BT.709; 5, 6, 2 or none BT.601; anything
    else stops the stream with LH264_E_UNSUPPORTED and a text naming the value) | "bt601" | "bt709".  colour_range: "auto" (the VUI's
    video_full_range_flag; absent: limited) | "limited" | "full".  DecodedBatch.colours(i) tells what was applied per picture;
    frames(i) is then (pictures, H, W, 3) or (pictures, 3, H, W).
    dtype: "uint8" (the default) | "float32" | "float16" | "bfloat16", a float dtype with colour= only: float RGB pictures, cast and
    normalised on the device in the same pack pass (decode_pack_sample_kernel through lh264_decode_batch_ex2; the uint8 RGB never
    reaches memory).  Element e of a picture is v = fma (float32 (c), mul[ch], add[ch]) - one binary32 fused multiply-add - of byte c
    at place e of the same call with dtype="uint8", ch its channel (0 R, 1 G, 2 B); "float32" delivers v, "float16" / "bfloat16" v
    rounded to nearest even (float16 overflows to infinity; no type flushes subnormals).  The layout is colour='s with elements in
    place of bytes, little-endian: 3*W*H*4 (or *2) bytes a picture; pictures, the sink, data, tensor and the digests are of those bytes.
    mul / add: None (1, 1, 1 / 0, 0, 0) or three finite numbers, rounded to binary32 once; normalise (mean, std) makes them.
    DecodedBatch.dtype is the dtype of the call, .affine the six binary32 values passed; frames(i) is the typed view.
    crop: None | (x, y, w, h) for every stream | a list with one entry per stream, each (x, y, w, h) or None: a rectangle in the
    coordinates of the picture's cropped window, all four even, x, y >= 0, w, h >= 2.  It takes the window's place in everything above:
    the copy, the scale= means (clamped to the crop), the size= resampling, colour and dtype; nothing outside it enters a delivered
    sample.  A crop that does not fit a picture's window stops that stream at that picture with LH264_E_ARG and a text naming the
    picture, the rectangle and the window; the pictures in front of it are delivered.  stream_window (data) gives a stream's window
    without decoding it.
    fit: "stretch" (the default) | "cover" | "contain", the latter two with size= only; w x h below is the window after crop=, OW x OH the
    size, all arithmetic in integers.  "cover": the largest centred sub-rectangle of the window with the size's aspect, resampled to the
    size - resize-to-cover plus centre crop in one pass.  "contain" (letterbox): the whole window resampled into the largest centred even
    rectangle of the size, every sample outside it fill = (y, cb, cr), default (16, 128, 128); with colour= a bar pixel is the conversion
    of the fill, with a float dtype its fma.  The rectangles are even and keep the aspect to the nearest even sample, not exactly:
    view_rects (w, h, crop, fit, size) is the rule (include/lh264.h at lh264_decode_batch_ex3), DecodedBatch.views(i) what was applied.
    source_sizes keeps giving the windows; frames(i) keeps its shapes.
    motion: False | True: beside the pictures, which are delivered exactly as without it, every delivered picture's motion field and
    macroblock data, gathered on the device from the records the parse left there (decode_pack_motion_kernel through
    lh264_decode_batch_ex4): DecodedBatch.motion(i), mb_info(i), motion_frames(i), mb_info_frames(i), motion_geometry(i).  They cover
    the coded picture, whatever scale, size, crop, fit, colour and dtype are.  With a sink the fields stay on the handles.
    pictures=False with motion=True and no sha1 is the motion-only call: nothing is reconstructed, no picture pool is used; the
    picture records are those of the digests-only call.
    select: None (every picture) | a slice (start, stop >= 0, step >= 1; stop None: to the stream's end) | a sequence of strictly
    increasing ints >= 0, for every stream | a list with one entry per stream, each one of those or None (every picture of that stream):
    THE PICTURES ASKED FOR BY NUMBER (decode order from 0, as picture_indices counts) are delivered, each byte for byte that picture of
    the call without select.  Of the stream only the runs from the last IDR picture (or picture 0) at or before a requested picture up
    to it are parsed and reconstructed - the pictures of a run that were not requested are reconstructed only - the others in front of
    the last requested picture are walked by their headers, and behind it the stream is not read: damage in what is not needed is
    neither seen nor reported.  A number the stream does not have delivers nothing and is no error.  The rule: include/lh264.h at
    lh264_decode_batch_ex5; plan (data, select) computes it without a device; chain_pictures(i) counts what was reconstructed.  Not
    together with pick or conceal.  With device_out=True, size= and a selection of equal length per stream, frames(i) is the (T, ...)
    clip of stream i, and torch.stack over the batch gives (N, T, ...).
    filter: "area" (the default: the area average of size=) | "bilinear" | "bicubic", the latter two with size= only: the window - after
    crop= and fit=, exactly as for the area average - is resampled by a triangle or a Catmull-Rom kernel, widened when shrinking
    (antialiased), as torchvision's and PIL's resize do; integer weights that sum to 2^14 per axis, built on the host, applied on the
    device by decode_pack_filtered_kernel and its RGB and float siblings through lh264_decode_batch_ex6, one rounding at the end.  The
    definition: include/lh264.h at that call; filter_taps (filter, src_len, dst_len) gives the weights without a device.  Colour and a
    float dtype act on the filtered planes; DecodedBatch.filter is the filter of the call."""
    lib = L.lib()
    if not isinstance(filter, str) or filter not in L.FILTER:
        raise ValueError("filter must be 'area', 'bilinear' or 'bicubic'")
    if filter != "area" and size is None:
        raise ValueError("a filter other than 'area' needs size=")
    sel, sel_keep = _select_struct(select, len(datas))
    if sel is not None and (pick != "all" or conceal not in (None, "off")):
        raise ValueError("select excludes pick and conceal")
    if not isinstance(dtype, str) or dtype not in L.SAMPLE:
        raise ValueError("dtype must be 'uint8', 'float32', 'float16' or 'bfloat16'")
    if dtype == "uint8":
        if mul is not None or add is not None:
            raise ValueError("mul and add need a float dtype")
        affine = None
    else:
        if colour is None:
            raise ValueError("a float dtype needs colour=")
        affine = (_three(mul, 1.0, "mul"), _three(add, 0.0, "add"))
    if colour not in L.COLOUR:
        raise ValueError("colour must be None, 'rgb24' or 'rgbp'")
    if matrix not in L.MATRIX or colour_range not in L.RANGE:
        raise ValueError("matrix must be 'auto', 'bt601' or 'bt709' and colour_range 'auto', 'limited' or 'full'")
    if colour is None and (matrix != "auto" or colour_range != "auto"):
        raise ValueError("matrix and colour_range need colour=")
    if colour is not None and fmt != "i420":
        raise ValueError("colour needs fmt='i420'")
    if fit not in L.FIT:
        raise ValueError("fit must be 'stretch', 'cover' or 'contain'")
    if fit != "stretch" and size is None:
        raise ValueError("fit needs size=")
    if fill is not None and fit != "contain":
        raise ValueError("fill needs fit='contain'")
    fill_word = 0
    if fit == "contain":
        f3 = (16, 128, 128) if fill is None else fill
        if not (isinstance(f3, (tuple, list)) and len(f3) == 3 and all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= 255 for v in f3)):
            raise ValueError("fill must be None or three ints (y, cb, cr) in 0..255")
        fill_word = f3[0] | f3[1] << 8 | f3[2] << 16
    crops = _crops(crop, len(datas))
    if size is not None:
        ok = isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and 2 <= v <= 4096 and v % 2 == 0 for v in size)
        if not ok:
            raise ValueError("size must be None or a pair (W, H) of even ints in 2..4096")
        if scale != 0:
            raise ValueError("size and scale exclude one another")
    if pick not in L.PICK:
        raise ValueError("pick must be 'all', 'intra' or 'idr'")
    if pick != "all" and conceal not in (None, "off"):
        raise ValueError("pick needs conceal off: concealment copies from the picture decoded before, which is not decoded")
    if scale not in (0, 1, 2, 3) or isinstance(scale, bool):
        raise ValueError("scale must be 0, 1, 2 or 3")
    if fmt not in _FORMATS:
        raise ValueError("fmt must be 'i420' or 'nv12'")
    if conceal is not None and conceal not in L.CONCEAL:
        raise ValueError("conceal must be one of %s" % ", ".join(sorted(L.CONCEAL)))
    if sha1 not in _SHA1:
        raise ValueError("sha1 must be None, 'pictures', 'stream' or 'both'")
    if parse not in L.PARSE_MODES:
        raise ValueError("parse must be 'host', 'device' or 'device+cabac'")
    if not pictures and sink is not None:
        raise ValueError("pictures=False excludes a sink")
    if not pictures and not motion and (sha1 is None or device_out):
        raise ValueError("pictures=False needs sha1= or motion=True, and device_out only with motion=True")
    n = len(datas)
    keep = [bytes(d) for d in datas]
    ptrs = (C.c_char_p * n)(*keep)
    lens = (C.c_size_t * n)(*[len(d) for d in keep])
    opts = L.DecodeOptsV6()
    opts.struct_bytes = C.sizeof(L.DecodeOptsV6)
    if size is not None:
        opts.out_width, opts.out_height = int(size[0]), int(size[1])
    opts.pick = L.PICK[pick]
    opts.scale_log2 = int(scale)
    opts.parse, opts.parse_flags = L.PARSE_MODES[parse]
    opts.format = _FORMATS[fmt]
    opts.flags = (L.DECODE_DEVICE_OUT if device_out else 0) | _SHA1[sha1] | (0 if pictures else L.DECODE_NO_PICTURES)
    opts.round_pictures = int(round_pictures or 0)
    opts.group_mbs = int(group_mbs or 0)
    opts.conceal = L.CONCEAL[conceal or "off"]
    cb = None
    if sink is not None:
        def _cb(user, stream, first, count, pics, data, ln):
            try:
                recs = np.frombuffer(C.string_at(pics, count * L.DECODED_PIC_DTYPE.itemsize), dtype=L.DECODED_PIC_DTYPE)
                lst = [(int(r["width"]), int(r["height"]), int(r["frame_num"]), int(r["idr"]), int(r["offset"]), int(r["bytes"])) for r in recs]
                return 1 if sink(stream, first, lst, C.string_at(data, ln)) else 0
            except Exception:      # an exception must not cross the C frames: the stream stops
                import traceback
                traceback.print_exc()
                return 1
        cb = L.DECODE_SINK_FN(_cb)
        opts.sink = cb
    outs = (C.c_void_p * n)()
    if fit != "stretch" or crops is not None or motion or sel is not None or filter != "area":
        # a view, the fields or a selection: every struct the call takes, the colour and sample ones where they are asked for
        view = None
        if fit != "stretch" or crops is not None:
            view = L.DecodeView()
            view.struct_bytes, view.fit, view.fill = C.sizeof(L.DecodeView), L.FIT[fit], fill_word
            if crops is not None:
                rects = (L.Rect * len(crops))(*[L.Rect(*c) for c in crops])
                view.n_crops, view.crops = len(crops), rects
        ext = sm = None
        if colour is not None:
            ext = L.DecodeExt()
            ext.struct_bytes, ext.colour, ext.matrix, ext.range = C.sizeof(L.DecodeExt), L.COLOUR[colour], L.MATRIX[matrix], L.RANGE[colour_range]
        if affine is not None:
            sm = L.DecodeSample()
            sm.struct_bytes, sm.type = C.sizeof(L.DecodeSample), L.SAMPLE[dtype]
            for k in range(3):
                sm.mul[k], sm.add[k] = affine[0][k], affine[1][k]
        ref = lambda st: C.byref(st) if st is not None else None
        mo = None
        if motion:
            mo = L.DecodeMotion()
            mo.struct_bytes, mo.fields = C.sizeof(L.DecodeMotion), L.MOTION_FIELDS
        if filter != "area":
            fl = L.DecodeFilter()
            fl.struct_bytes, fl.filter = C.sizeof(L.DecodeFilter), L.FILTER[filter]
            rc = lib.lh264_decode_batch_ex6(ptrs, lens, n, threads, C.byref(opts), ref(ext), ref(sm), ref(view), ref(mo), ref(sel), C.byref(fl), outs)
        elif sel is not None:
            rc = lib.lh264_decode_batch_ex5(ptrs, lens, n, threads, C.byref(opts), ref(ext), ref(sm), ref(view), ref(mo), C.byref(sel), outs)
        elif motion:
            rc = lib.lh264_decode_batch_ex4(ptrs, lens, n, threads, C.byref(opts), ref(ext), ref(sm), ref(view), C.byref(mo), outs)
        else:
            rc = lib.lh264_decode_batch_ex3(ptrs, lens, n, threads, C.byref(opts), ref(ext), ref(sm), C.byref(view), outs)
    elif colour is None:
        rc = lib.lh264_decode_batch(ptrs, lens, n, threads, C.byref(opts), outs)
    else:
        ext = L.DecodeExt()
        ext.struct_bytes, ext.colour, ext.matrix, ext.range = C.sizeof(L.DecodeExt), L.COLOUR[colour], L.MATRIX[matrix], L.RANGE[colour_range]
        if affine is None:
            rc = lib.lh264_decode_batch_ex(ptrs, lens, n, threads, C.byref(opts), C.byref(ext), outs)
        else:
            sm = L.DecodeSample()
            sm.struct_bytes, sm.type = C.sizeof(L.DecodeSample), L.SAMPLE[dtype]
            for k in range(3):
                sm.mul[k], sm.add[k] = affine[0][k], affine[1][k]
            rc = lib.lh264_decode_batch_ex2(ptrs, lens, n, threads, C.byref(opts), C.byref(ext), C.byref(sm), outs)
    if rc == L.E_NODEVICE:
        raise RuntimeError("losslessh264_amd: no GPU visible (there is no CPU fallback)")
    if rc != 0:
        raise RuntimeError("lh264_decode_batch: error %d" % rc)
    return DecodedBatch(lib, [outs[i] for i in range(n)], device_out, cb, tuple(size) if size is not None else None, colour, dtype, affine, motion, filter)


def _select_entry(s):
    """one stream's select= -> (numbers or None, first, count, step) of an lh264_select_t"""
    if s is None:
        return None, 0, 0, 1
    if isinstance(s, slice):
        start, stop, step = 0 if s.start is None else s.start, s.stop, 1 if s.step is None else s.step
        if not all(v is None or (isinstance(v, int) and not isinstance(v, bool)) for v in (start, stop, step)) or start < 0 or step < 1 or (stop is not None and stop < 0) or start >= 2 ** 31 or step >= 2 ** 31:
            raise ValueError("a select slice has start, stop >= 0 and step >= 1")
        if stop is None:
            return None, start, 0, step
        count = len(range(start, min(stop, 2 ** 31), step))
        return ([], 0, 0, 1) if count == 0 else (None, start, count, step)
    if isinstance(s, (list, tuple, range, np.ndarray)) and all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in s):
        nums = [int(v) for v in s]
        if any(v < 0 or v >= 2 ** 31 for v in nums) or any(b <= a for a, b in zip(nums, nums[1:])):
            raise ValueError("a select sequence holds strictly increasing ints >= 0")
        return nums, 0, 0, 1
    raise ValueError("select must be None, a slice, a sequence of ints, or a list with one of those per stream")


def _select_struct(select, n):
    """select= of decode_batch -> (None, None) or the lh264_decode_select_t the call passes and what keeps its arrays alive"""
    if select is None:
        return None, None
    per_stream = isinstance(select, list) and any(v is None or isinstance(v, (slice, list, tuple, range, np.ndarray)) for v in select)
    if per_stream and len(select) != n:
        raise ValueError("a list of selections has one entry per stream")
    entries = [_select_entry(s) for s in select] if per_stream else [_select_entry(select)]
    arr = (L.Select * max(1, len(entries)))()
    keep = [arr]
    for k, (nums, first, count, step) in enumerate(entries):
        if nums is not None:
            a = (C.c_int32 * max(1, len(nums)))(*nums)
            keep.append(a)
            arr[k].list, arr[k].n_list = a, len(nums)
        arr[k].first, arr[k].count, arr[k].step = first, count, step
    st = L.DecodeSelect()
    st.struct_bytes, st.n_selects, st.selects = C.sizeof(L.DecodeSelect), len(entries), arr
    if not entries:
        return None, None
    return st, keep


def plan(data, select):
    """(needed, delivered): the picture numbers decode_batch (select=select) reconstructs and delivers from one Annex-B stream, by the
    rule of include/lh264.h at lh264_decode_batch_ex5 (lh264_parser_plan): headers only, no device, no further than the last requested
    picture, up to the first failure of the header walk.  select: None | a slice | a sequence of ints, as one stream's select="""
    st, keep = _select_struct([select], 1)
    lib = L.lib()
    data = bytes(data)
    nn, nd = C.c_int(0), C.c_int(0)
    L.check(lib.lh264_parser_plan(data, len(data), C.byref(st.selects[0]), None, 0, C.byref(nn), None, 0, C.byref(nd)))
    a, b = (C.c_int32 * max(1, nn.value))(), (C.c_int32 * max(1, nd.value))()
    L.check(lib.lh264_parser_plan(data, len(data), C.byref(st.selects[0]), a, nn.value, C.byref(nn), b, nd.value, C.byref(nd)))
    return [int(a[k]) for k in range(nn.value)], [int(b[k]) for k in range(nd.value)]


def filter_taps(filter, src_len, dst_len):
    """the weights of filter= "bilinear" | "bicubic" for an axis of src_len samples delivered as dst_len -> [(first, weights)] per
    delivered coordinate: the index of the first source sample with a weight and the int weights from there, which sum to 16384.  The
    rule of include/lh264.h at lh264_decode_batch_ex6, computed by the library without a device (lh264_filter_taps); ValueError for
    "area", which has no such table, and for lengths outside 1..16384 and 1..4096"""
    if not isinstance(filter, str) or filter not in L.FILTER:
        raise ValueError("filter must be 'bilinear' or 'bicubic'")
    lib = L.lib()
    out = []
    first, n = C.c_int32(0), C.c_int(0)
    buf = (C.c_int16 * 64)()
    for X in range(max(1, int(dst_len))):
        rc = lib.lh264_filter_taps(L.FILTER[filter], int(src_len), int(dst_len), X, C.byref(first), buf, len(buf), C.byref(n))
        if rc == 0 and n.value > len(buf):
            buf = (C.c_int16 * n.value)()
            rc = lib.lh264_filter_taps(L.FILTER[filter], int(src_len), int(dst_len), X, C.byref(first), buf, len(buf), C.byref(n))
        if rc != 0:
            raise ValueError("filter_taps: a filter without a table, or a length or coordinate that is not defined")
        out.append((first.value, [int(buf[k]) for k in range(n.value)]))
    return out


def _rect(c):
    ok = isinstance(c, (tuple, list)) and len(c) == 4 and all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= 16384 and v % 2 == 0 for v in c) and c[2] >= 2 and c[3] >= 2
    if not ok:
        raise ValueError("a crop is (x, y, w, h): four even ints, x, y >= 0, w, h >= 2")
    return tuple(c)


def _crops(crop, n):
    """crop= of decode_batch -> None, or the rectangles the call passes: one for every stream, or one per stream ((0, 0, 0, 0): none)"""
    if crop is None:
        return None
    if isinstance(crop, list) and (len(crop) == 0 or crop[0] is None or isinstance(crop[0], (tuple, list))):
        if len(crop) != n:
            raise ValueError("a list of crops has one entry per stream")
        if all(c is None for c in crop):
            return None
        return [(0, 0, 0, 0) if c is None else _rect(c) for c in crop]
    return [_rect(crop)]


def view_rects(w, h, crop=None, fit="stretch", size=None):
    """the view of a w x h window under crop= / fit= / size= of decode_batch -> (src, dst), each (x, y, w, h): the source rectangle in
    the window and the destination rectangle in the delivered picture (without a size: the source's own size at (0, 0)).  The rule of
    include/lh264.h at lh264_decode_batch_ex3, computed by the library without a device; ValueError for what decode_batch refuses and
    for a crop that does not fit the window"""
    if fit not in L.FIT:
        raise ValueError("fit must be 'stretch', 'cover' or 'contain'")
    c = L.Rect(*_rect(crop)) if crop is not None else None
    s, d = L.Rect(), L.Rect()
    ow, oh = (0, 0) if size is None else (int(size[0]), int(size[1]))
    if L.lib().lh264_view_rects(int(w), int(h), C.byref(c) if c is not None else None, L.FIT[fit], ow, oh, C.byref(s), C.byref(d)) != 0:
        raise ValueError("view_rects: a window, crop, fit or size that is not defined, or a crop that does not fit the window")
    return (s.x, s.y, s.w, s.h), (d.x, d.y, d.w, d.h)


def stream_window(data):
    """(width, height) of the cropped window of the first SPS of an Annex-B file that parses - what its pictures deliver at full size,
    and the coordinates crop= is given in; None where no SPS parses.  Headers only, no device"""
    data = bytes(data)
    w, h = C.c_int32(0), C.c_int32(0)
    rc = L.lib().lh264_parser_window(data, len(data), C.byref(w), C.byref(h))
    if rc == L.E_UNSUPPORTED:
        return None
    L.check(rc)
    return w.value, h.value


def _three(v, default, name):
    """mul= / add= of decode_batch -> three Python floats that are binary32 values (rounded once, by numpy)"""
    if v is None:
        return (default,) * 3
    ok = isinstance(v, (tuple, list, np.ndarray)) and len(v) == 3 and all(isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_)) for x in v)
    if ok:
        with np.errstate(over="ignore"):
            r = np.asarray([float(x) for x in v], dtype=np.float64).astype(np.float32)
        ok = bool(np.all(np.isfinite(r)))
    if not ok:
        raise ValueError("%s must be None or three finite numbers (finite as binary32 too)" % name)
    return tuple(float(x) for x in r)


def normalise(mean, std):
    """(mul, add) for decode_batch (dtype=<a float type>, mul=, add=) from a per-channel mean and deviation in 0..1 units (R, G, B), so
    that an element is (c / 255 - mean) / std: mul = 1 / (255 * std), add = -mean / std, computed in float64 and rounded to binary32.
    These six ROUNDED values, not the real numbers, define the output: an element is fma (float32 (c), mul, add) of them, bit for bit,
    which differs from (c / 255 - mean) / std evaluated in any other order or precision by rounding error"""
    m, s = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    if m.shape != (3,) or s.shape != (3,) or not np.all(np.isfinite(m)) or not np.all(np.isfinite(s)) or np.any(s == 0):
        raise ValueError("mean and std must be three finite numbers each, std not 0")
    mul, add = (1.0 / (255.0 * s)).astype(np.float32), (-m / s).astype(np.float32)
    return tuple(float(x) for x in mul), tuple(float(x) for x in add)


def decode_arena_bytes():
    """(device bytes, page-locked host bytes) the decode call keeps on the current device"""
    d, p = C.c_size_t(0), C.c_size_t(0)
    L.check(L.lib().lh264_decode_arena_bytes(C.byref(d), C.byref(p)))
    return d.value, p.value


_SUFFIX = {"uint8": ".rgb", "float32": ".f32", "float16": ".f16", "bfloat16": ".bf16"}


def decode_to_files(paths, out_dir, fmt="i420", conceal=None, parse="host", scale=0, pick="all", size=None, colour=None, matrix="auto", colour_range="auto", dtype="uint8", mul=None, add=None, fit="stretch", fill=None, crop=None, motion=0, select=None, filter="area"):
    """out_dir/<basename>.yuv - with colour= <basename>.rgb, with a float dtype= <basename>.f32 | .f16 | .bf16 - for every input, through one decode_batch with a sink that appends to the
    files -> [(path, status, error, pictures, bytes)]; select (one entry, for every file), scale, pick, size, filter, colour, matrix, colour_range, dtype, mul, add, fit, fill and crop as in decode_batch.
    motion: 1: beside them <basename>.mv and <basename>.mbi, every stream's motion blocks and macroblock blocks as the handle holds them
    (decode_batch (motion=True)); 2: those two and no picture file, through the motion-only call (path and bytes are then the .mv file's
    and both files')"""
    datas = [open(p, "rb").read() for p in paths]
    os.makedirs(out_dir, exist_ok=True)
    if motion == 2:
        b = decode_batch(datas, fmt=fmt, conceal=conceal, parse=parse, scale=scale, pick=pick, size=size, colour=colour, matrix=matrix, colour_range=colour_range, dtype=dtype, mul=mul, add=add, fit=fit, fill=fill, crop=crop, motion=True, pictures=False, select=select, filter=filter)
        res = [_write_fields(b, i, os.path.join(out_dir, os.path.basename(p))) for i, p in enumerate(paths)]
        b.free()
        return res
    names = [os.path.join(out_dir, os.path.basename(p) + (".yuv" if colour is None else _SUFFIX.get(dtype, ".rgb"))) for p in paths]
    files = [open(q, "wb") for q in names]
    total = [0] * len(paths)

    def sink(stream, first, pics, data):
        files[stream].write(data)
        total[stream] += len(data)
        return 0
    try:
        b = decode_batch(datas, fmt=fmt, sink=sink, conceal=conceal, parse=parse, scale=scale, pick=pick, size=size, colour=colour, matrix=matrix, colour_range=colour_range, dtype=dtype, mul=mul, add=add, fit=fit, fill=fill, crop=crop, motion=bool(motion), select=select, filter=filter)
    finally:
        for f in files:
            f.close()
    if motion:
        for i, p in enumerate(paths):
            _write_fields(b, i, os.path.join(out_dir, os.path.basename(p)))
    res = [(names[i], b.status(i), b.error(i), len(b.pictures(i)), total[i]) for i in range(len(paths))]
    b.free()
    return res


def _write_fields(b, i, stem):
    """stem.mv and stem.mbi: stream i's two field buffers -> (stem.mv, status, error, pictures, bytes of both)"""
    mot, mbi = b._field_buffers(i)
    with open(stem + ".mv", "wb") as f:
        f.write(mot.tobytes())
    with open(stem + ".mbi", "wb") as f:
        f.write(mbi.tobytes())
    return stem + ".mv", b.status(i), b.error(i), len(b.pictures(i)), mot.nbytes + mbi.nbytes


def decode_to_sha1_files(paths, out_dir, fmt="i420", conceal=None, parse="host", scale=0, pick="all", size=None, colour=None, matrix="auto", colour_range="auto", dtype="uint8", mul=None, add=None, fit="stretch", fill=None, crop=None, select=None, filter="area"):
    """out_dir/<basename>.sha1 for every input, through one digests-only decode_batch: a line `index width height frame_num idr hex`
    per picture, then `stream hex` -> [(path, status, error, pictures, stream digest as hex)]; select (one entry, for every file), scale, pick, size, fit, fill and crop as in decode_batch (the digests are of the delivered bytes; index is the picture's number in the stream in decode
    order, which with pick="all" and nothing withheld counts the lines)"""
    datas = [open(p, "rb").read() for p in paths]
    os.makedirs(out_dir, exist_ok=True)
    b = decode_batch(datas, fmt=fmt, conceal=conceal, sha1="both", pictures=False, parse=parse, scale=scale, pick=pick, size=size, colour=colour, matrix=matrix, colour_range=colour_range, dtype=dtype, mul=mul, add=add, fit=fit, fill=fill, crop=crop, select=select, filter=filter)
    res = []
    try:
        for i, p in enumerate(paths):
            name = os.path.join(out_dir, os.path.basename(p) + ".sha1")
            st = b.status(i)
            pics = b.pictures(i) if st != L.E_HIP else []
            digs = b.picture_sha1(i) if pics else []
            index = b.picture_indices(i) if pics else []
            total = b.stream_sha1(i).hex() if st != L.E_HIP else ""
            with open(name, "w") as f:
                for k, (w, h, fn, idr, _off, _n) in enumerate(pics):
                    f.write("%d %d %d %d %d %s\n" % (index[k], w, h, fn, idr, digs[k].hex()))
                if st != L.E_HIP:
                    f.write("stream %s\n" % total)
            res.append((name, st, b.error(i), len(pics), total))
    finally:
        b.free()
    return res
