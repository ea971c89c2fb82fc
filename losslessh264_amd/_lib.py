"""ctypes binding of liblh264.so (the C ABI of include/lh264.h)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("LH264_SO", os.path.join(HERE, "liblh264.so"))   # LH264_SO: tuning experiments only


class LibraryMissing(RuntimeError):
    pass


# record layouts == include/lh264.h
MB_DTYPE = np.dtype([
    ("mb_type", "<u2"), ("cbp", "u1"), ("qp_y", "u1"), ("qp_c", "u1", (2,)), ("flags", "u1"),
    ("intra_avail", "u1"), ("intra_mode", "i1", (16,)), ("chroma_mode", "i1"), ("reserved0", "u1"),
    ("slice_id", "<u2"), ("sub_type", "u1", (4,)), ("ref_idx", "i1", (4,)), ("nzc", "u1", (24,)),
    ("mv", "<i2", (16, 2)), ("reserved1", "u1", (4,)),
])
SLICE_DTYPE = np.dtype([
    ("first_mb", "<i4"), ("n_mbs", "<i4"), ("slice_type", "u1"), ("deblock_idc", "u1"),
    ("alpha_c0_offset", "i1"), ("beta_offset", "i1"), ("weighted_pred", "u1"), ("luma_log2_denom", "u1"),
    ("chroma_log2_denom", "u1"), ("n_refs", "u1"),
    ("luma_weight", "<i2", (16,)), ("luma_offset", "<i2", (16,)),
    ("chroma_weight", "<i2", (16, 2)), ("chroma_offset", "<i2", (16, 2)),
    ("ref_slot", "i1", (16,)), ("luma_dc_weight", "u1"), ("reserved", "u1", (7,)),
])
JOB_DTYPE = np.dtype([
    ("mbs", "<u8"), ("coeffs", "<u8"), ("slices", "<u8"),
    ("dst", "<u8", (3,)), ("ref", "<u8", (16, 3)),
    ("mb_w", "<i4"), ("mb_h", "<i4"), ("stride_y", "<i4"), ("stride_c", "<i4"), ("n_slices", "<i4"), ("flags", "<i4"),
])
assert MB_DTYPE.itemsize == 128 and SLICE_DTYPE.itemsize == 232 and JOB_DTYPE.itemsize == 456

JOB_NO_EXPAND, JOB_NO_DEBLOCK = 1, 2
PAD_Y, PAD_C = 32, 16

_lib = None

_SIGS = {
    "lh264_abi_version": (C.c_int, []),
    "lh264_build_id": (C.c_char_p, []),
    "lh264_last_error": (C.c_char_p, []),
    "lh264_device_count": (C.c_int, []),
    "lh264_set_device": (C.c_int, [C.c_int]),
    "lh264_dev_malloc": (C.c_void_p, [C.c_size_t]),
    "lh264_dev_free": (C.c_int, [C.c_void_p]),
    "lh264_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lh264_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lh264_dev_memset": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "lh264_stream_sync": (C.c_int, [C.c_void_p]),
    "lh264_pic_bytes": (C.c_size_t, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lh264_recon_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "lh264_recon_chains": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "lh264_time_recon_chains": (C.c_double, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}
FRAME_INFO_DTYPE = np.dtype([("id", "<i4"), ("mb_w", "<i4"), ("mb_h", "<i4"), ("n_slices", "<i4"), ("n_refs", "<i4"), ("frame_num", "<i4"),
                             ("crop_x", "<i4"), ("crop_y", "<i4"), ("crop_w", "<i4"), ("crop_h", "<i4"), ("is_ref", "<i4"), ("idr", "<i4"),
                             ("ref_ids", "<i4", (16,))])
_SIGS.update({
    "lh264_parser_create": (C.c_void_p, []),
    "lh264_parser_destroy": (None, [C.c_void_p]),
    "lh264_parser_feed": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int]),
    "lh264_pip_restore": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lh264_restore_error": (C.c_char_p, []),
    "lh264_compress_batch": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "lh264_compress_batch_devices": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "lh264_compressed_status": (C.c_int, [C.c_void_p]),
    "lh264_compressed_error": (C.c_char_p, [C.c_void_p]),
    "lh264_compressed_main": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "lh264_compressed_tag": (C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "lh264_compressed_pictures": (C.c_int, [C.c_void_p]),
    "lh264_compressed_free": (None, [C.c_void_p]),
    "lh264_compress_release": (None, []),
    "lh264_pip_pack_bound": (C.c_size_t, [C.c_size_t, C.POINTER(C.c_size_t), C.c_int]),
    "lh264_pip_pack": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lh264_pip_restore_file": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lh264_parse_batch": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "lh264_parse_batch_discard": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "lh264_pip_restore_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "lh264_parser_feed_file": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "lh264_parser_main_stream": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "lh264_parser_pcm_samples": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "lh264_parser_frame_count": (C.c_int, [C.c_void_p]),
    "lh264_parser_frame_info": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lh264_parser_frame_mbs": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_coeffs": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_levels": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_slices": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_covered": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_syntax": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_slice_syntax": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_syn_symbols": (C.c_void_p, [C.c_void_p, C.c_int, C.c_void_p]),
    "lh264_parser_frame_syn_offsets": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_parser_error": (C.c_char_p, [C.c_void_p]),
    "lh264_parser_out_of_range": (C.c_char_p, [C.c_void_p]),
    "lh264_parser_set_tolerant": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_parser_not_kept": (C.c_char_p, [C.c_void_p]),
    "lh264_parser_not_carried": (C.c_char_p, [C.c_void_p]),
    "lh264_parser_escapes": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_size_t)]),
})
CODE_JOB_DTYPE = np.dtype([("syn_syms", "<u8"), ("syn_off", "<u8"), ("ctx_syms", "<u8"), ("ctx_n_syms", "<u8"), ("n_mbs", "<i4"), ("reserved", "<i4"),
                           ("ctx_sym_off", "<u8"), ("ctx_sym_base", "<u8")])
CODE_STREAM_DTYPE = np.dtype([("hash_keys", "<u8"), ("hash_cells", "<u8"), ("out", "<u8"), ("out_len", "<u8"), ("hash_cap", "<u4"), ("out_cap", "<u4")])
N_TAG_SLOTS = 40
assert CODE_JOB_DTYPE.itemsize == 56 and CODE_STREAM_DTYPE.itemsize == 40
_SIGS["lh264_code_chains"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p])
_SIGS["lh264_code_binarise_chains"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p])
_SIGS["lh264_code_finish_chains"] = (C.c_int, [C.c_void_p, C.c_int, C.c_void_p])
_SIGS["lh264_code_last_totals"] = (C.c_int, [C.c_void_p, C.c_void_p])
# resumable calls (a stream coded in segments): flags per stream, the size of a stream's carry block, its decision counts
CODE_SEG_FIRST, CODE_SEG_LAST = 1, 2
_SIGS["lh264_code_carry_bytes"] = (C.c_size_t, [C.c_uint32])
_SIGS["lh264_code_chains_resume"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p])
_SIGS["lh264_parser_begin_file"] = (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t])
_SIGS["lh264_parser_feed_file_some"] = (C.c_int, [C.c_void_p, C.c_uint64])
_SIGS["lh264_parser_drop_frames"] = (C.c_int, [C.c_void_p, C.c_int])
_SIGS["lh264_code_last_decisions"] = (C.c_int, [C.c_int, C.c_int, C.c_void_p])
COMPRESS_ESCAPES = 1
COMPRESS_TOLERANT = 2
TAG_ESC = 71
class CompressOpts(C.Structure):       # flags: the word include/lh264.h declares as `reserved`
    _fields_ = [("struct_bytes", C.c_uint32), ("flags", C.c_uint32), ("segment_mbs", C.c_uint64)]
_SIGS["lh264_compress_batch_opts"] = (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(CompressOpts), C.POINTER(C.c_void_p)])
_SIGS["lh264_compress_batch_devices_opts"] = (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(CompressOpts), C.POINTER(C.c_void_p)])
_SIGS["lh264_compressed_segments"] = (C.c_int, [C.c_void_p])
_SIGS["lh264_compressed_decisions"] = (C.c_uint64, [C.c_void_p, C.c_int])
_SIGS["lh264_compress_arena_bytes"] = (C.c_int, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)])
_SIGS["lh264_code_carry_decisions"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
# ---- the decode direction behind one call
FMT_I420, FMT_NV12 = 0, 1
DECODE_DEVICE_OUT, DECODE_SHA1_PICTURES, DECODE_SHA1_STREAM, DECODE_NO_PICTURES = 1, 4, 8, 32
E_NODEVICE, E_ARG, E_HIP, E_UNSUPPORTED = -1, -2, -3, -4
DECODED_PIC_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("frame_num", "<i4"), ("idr", "<i4"), ("offset", "<u8"), ("bytes", "<u8")])
DECODE_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
class DecodeOpts(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("format", C.c_uint32), ("flags", C.c_uint32), ("round_pictures", C.c_uint32),
                ("group_mbs", C.c_uint64), ("sink", DECODE_SINK_FN), ("user", C.c_void_p), ("conceal", C.c_uint32)]
DECODE_OPTS_BYTES_V1 = 40          # the struct before `conceal`: still accepted, concealment off
class DecodeOptsV3(C.Structure):   # the struct as it is now: `parse` behind what was the 48-byte struct's tail padding
    _fields_ = DecodeOpts._fields_ + [("reserved0", C.c_uint32), ("parse", C.c_uint32), ("parse_flags", C.c_uint32)]
DECODE_OPTS_BYTES_V2 = 48          # the struct before `parse` (DecodeOpts): still accepted, the host parses
PARSE = {"host": 0, "device": 1}
PARSE_FLAG_CABAC = 1
# decode_batch (parse=...): the strings of PARSE, and "device+cabac" = LH264_PARSE_DEVICE with LH264_PARSE_FLAG_CABAC
PARSE_MODES = {"host": (0, 0), "device": (1, 0), "device+cabac": (1, PARSE_FLAG_CABAC)}
SLICE_PARSE_ON_DEVICE, SLICE_PARSE_CABAC = 1, 2
PARSE_PATH = {0: "host", 1: "device", 2: "fallback"}
assert C.sizeof(DecodeOptsV3) == 56
class DecodeOptsV4(C.Structure):   # the struct before `pick`: `scale_log2` behind the 56-byte struct
    _fields_ = DecodeOptsV3._fields_ + [("scale_log2", C.c_uint32), ("reserved2", C.c_uint32)]
DECODE_OPTS_BYTES_V3 = 56          # the struct before `scale_log2` (DecodeOptsV3): still accepted, full size
assert C.sizeof(DecodeOptsV4) == 64
class DecodeOptsV5(C.Structure):   # the struct before `out_width`: `pick` behind the 64-byte struct
    _fields_ = DecodeOptsV4._fields_ + [("pick", C.c_uint32), ("reserved3", C.c_uint32)]
DECODE_OPTS_BYTES_V4 = 64          # the struct before `pick` (DecodeOptsV4): still accepted, every picture
assert C.sizeof(DecodeOptsV5) == 72
class DecodeOptsV6(C.Structure):   # the struct as it is now: the delivered size behind the 72-byte struct
    _fields_ = DecodeOptsV5._fields_ + [("out_width", C.c_uint32), ("out_height", C.c_uint32), ("reserved4", C.c_uint32), ("reserved5", C.c_uint32)]
DECODE_OPTS_BYTES_V5 = 72          # the struct before `out_width` (DecodeOptsV5): still accepted, no size
assert C.sizeof(DecodeOptsV6) == 88
PICK = {"all": 0, "intra": 1, "idr": 2}      # LH264_PICK_*
# LH264_CONCEAL_*: the values of the reference's ERROR_CON_IDC; the FRAME_COPY pair (1, 3) is not provided
CONCEAL = {"off": 0, "slice_copy": 2, "slice_copy_cross_idr": 4, "slice_copy_cross_idr_freeze": 5, "mv_copy": 6, "mv_copy_freeze": 7}
class PackJob(C.Structure):         # reserved: the job's scale_log2 (0 = the copy, 1..3 = the means)
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("dst", C.c_void_p),
                ("stride_y", C.c_int32), ("stride_c", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32),
                ("crop_w", C.c_int32), ("crop_h", C.c_int32), ("format", C.c_int32), ("reserved", C.c_int32)]
class DecodeExt(C.Structure):       # lh264_decode_ext_t: what lh264_decode_batch_ex takes beside the frozen options
    _fields_ = [("struct_bytes", C.c_uint32), ("colour", C.c_uint32), ("matrix", C.c_uint32), ("range", C.c_uint32),
                ("reserved0", C.c_uint32), ("reserved1", C.c_uint32)]
assert C.sizeof(DecodeExt) == 24
COLOUR = {None: 0, "rgb24": 1, "rgbp": 2}                # LH264_COLOUR_*
MATRIX = {"auto": 0, "bt601": 1, "bt709": 2}             # LH264_MATRIX_*
RANGE = {"auto": 0, "limited": 1, "full": 2}             # LH264_RANGE_*
class DecodeSample(C.Structure):    # lh264_decode_sample_t: what lh264_decode_batch_ex2 takes beside the two frozen structs
    _fields_ = [("struct_bytes", C.c_uint32), ("type", C.c_uint32), ("mul", C.c_float * 3), ("add", C.c_float * 3)]
assert C.sizeof(DecodeSample) == 32
SAMPLE = {"uint8": 0, "float32": 1, "float16": 2, "bfloat16": 3}      # LH264_SAMPLE_*
class Rect(C.Structure):            # lh264_rect_t
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]
class DecodeView(C.Structure):      # lh264_decode_view_t: what lh264_decode_batch_ex3 takes beside the three frozen structs
    _fields_ = [("struct_bytes", C.c_uint32), ("fit", C.c_uint32), ("fill", C.c_uint32), ("n_crops", C.c_uint32),
                ("crops", C.POINTER(Rect)), ("reserved0", C.c_uint32), ("reserved1", C.c_uint32)]
class PackPlace(C.Structure):       # lh264_pack_place_t: where a pack job's picture lies in the delivered one, and the bars' fill
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("fill", C.c_uint32), ("reserved", C.c_uint32)]
assert C.sizeof(Rect) == 16 and C.sizeof(DecodeView) == 32 and C.sizeof(PackPlace) == 24
FIT = {"stretch": 0, "cover": 1, "contain": 2}            # LH264_FIT_*
class DecodeMotion(C.Structure):    # lh264_decode_motion_t: what lh264_decode_batch_ex4 takes beside the four frozen structs
    _fields_ = [("struct_bytes", C.c_uint32), ("fields", C.c_uint32), ("reserved0", C.c_uint32), ("reserved1", C.c_uint32)]
class DecodedMotion(C.Structure):   # lh264_decoded_motion_t: a delivered picture's field geometry and where its two blocks begin
    _fields_ = [("mb_w", C.c_int32), ("mb_h", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("motion_offset", C.c_uint64), ("info_offset", C.c_uint64)]
class MotionJob(C.Structure):       # lh264_motion_job_t: one picture's records to gather into a motion block and a macroblock block
    _fields_ = [("mbs", C.c_void_p), ("slices", C.c_void_p), ("motion", C.c_void_p), ("info", C.c_void_p),
                ("mb_w", C.c_int32), ("mb_h", C.c_int32), ("n_slices", C.c_int32), ("reserved", C.c_int32), ("back", C.c_int16 * 16)]
assert C.sizeof(DecodeMotion) == 16 and C.sizeof(DecodedMotion) == 32 and C.sizeof(MotionJob) == 80
MOTION_FIELDS = 1                   # LH264_MOTION_FIELDS
class Select(C.Structure):          # lh264_select_t: one stream's requested pictures, a list or a range
    _fields_ = [("list", C.POINTER(C.c_int32)), ("n_list", C.c_uint32), ("first", C.c_uint32), ("count", C.c_uint32), ("step", C.c_uint32)]
class DecodeSelect(C.Structure):    # lh264_decode_select_t: what lh264_decode_batch_ex5 takes beside the five frozen structs
    _fields_ = [("struct_bytes", C.c_uint32), ("n_selects", C.c_uint32), ("selects", C.POINTER(Select)), ("reserved", C.c_uint64)]
assert C.sizeof(Select) == 24 and C.sizeof(DecodeSelect) == 24
class DecodeFilter(C.Structure):    # lh264_decode_filter_t: what lh264_decode_batch_ex6 takes beside the six frozen structs
    _fields_ = [("struct_bytes", C.c_uint32), ("filter", C.c_uint32), ("reserved0", C.c_uint32), ("reserved1", C.c_uint32)]
assert C.sizeof(DecodeFilter) == 16
FILTER = {"area": 0, "bilinear": 1, "bicubic": 2}         # LH264_FILTER_*
MOTION_CHUNK_MBS = 64               # LH264_MOTION_CHUNK_MBS: the macroblocks of a row one workgroup of decode_pack_motion_kernel handles
RESTORE_CABAC_DEVICE = 1
class RestoreOpts(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("threads", C.c_int32), ("flags", C.c_uint32)]
assert DECODED_PIC_DTYPE.itemsize == 32 and C.sizeof(DecodeOpts) == 48 and C.sizeof(PackJob) == 64 and C.sizeof(RestoreOpts) == 12
_SIGS.update({
    "lh264_decode_batch": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lh264_decode_batch_ex": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lh264_decode_batch_ex2": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lh264_decoded_sample_type": (C.c_int, [C.c_void_p]),
    "lh264_decode_batch_ex3": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lh264_decoded_picture_view": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "lh264_decode_batch_ex4": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lh264_decode_batch_ex5": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lh264_decode_batch_ex6": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lh264_decoded_filter": (C.c_int, [C.c_void_p]),
    "lh264_filter_taps": (C.c_int, [C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "lh264_debug_filter_cpu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    "lh264_debug_filter_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    "lh264_decoded_chain_pictures": (C.c_longlong, [C.c_void_p]),
    "lh264_parser_plan": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "lh264_decoded_picture_motion": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lh264_decoded_motion": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "lh264_decoded_motion_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "lh264_decoded_motion_copy_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "lh264_decode_last_motion": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)]),
    "lh264_debug_motion_cpu": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_debug_motion_dev": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_view_rects": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "lh264_parser_window": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lh264_debug_view_cpu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lh264_debug_view_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lh264_debug_sample_cpu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lh264_debug_sample_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "lh264_debug_sample_round": (C.c_int, [C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "lh264_decoded_picture_colour": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    "lh264_parser_colour": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lh264_debug_rgb_cpu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "lh264_debug_rgb_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "lh264_decoded_parse_path": (C.c_int, [C.c_void_p]),
    "lh264_decoded_device_slices": (C.c_longlong, [C.c_void_p]),
    "lh264_decoded_device_cabac_slices": (C.c_longlong, [C.c_void_p]),
    "lh264_decode_last_parse_timing": (C.c_int, [C.POINTER(C.c_double)]),
    "lh264_decoded_parsed_slices": (C.c_longlong, [C.c_void_p]),
    "lh264_decoded_picture_index": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_decode_last_chains": (C.c_int, [C.POINTER(C.c_longlong)]),
    "lh264_parser_pick": (C.c_int, [C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    "lh264_decoded_status": (C.c_int, [C.c_void_p]),
    "lh264_decoded_error": (C.c_char_p, [C.c_void_p]),
    "lh264_decoded_pictures": (C.c_int, [C.c_void_p]),
    "lh264_decoded_picture": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lh264_decoded_concealed": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_parser_set_conceal": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_conceal": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lh264_decoded_bytes": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "lh264_decoded_bytes_dev": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "lh264_decoded_copy_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "lh264_decoded_free": (None, [C.c_void_p]),
    "lh264_decode_arena_bytes": (C.c_int, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lh264_decode_release": (None, []),
    "lh264_decode_last_timing": (C.c_int, [C.POINTER(C.c_double)]),
    "lh264_debug_pack_cpu": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_debug_pack_dev": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_debug_resize_cpu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "lh264_debug_resize_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "lh264_decoded_picture_source_size": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lh264_decoded_picture_sha1": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lh264_decoded_stream_sha1": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lh264_debug_sha1": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "lh264_parser_set_sparse_coeffs": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_sparse_coeffs": (C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
})
# ---- CAVLC slice data apart from the header walk (csrc/lh264_slice.h)
SLICE_OK, SLICE_SYNTAX, SLICE_OVERRUN, SLICE_BAD_TASK = 0, 1, 2, 3
_SIGS.update({
    "lh264_parser_set_defer_slice_data": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_deferred": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_parser_set_defer_cabac": (C.c_int, [C.c_void_p, C.c_int]),
    "lh264_parser_frame_deferred_cabac": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "lh264_parser_parse_deferred": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "lh264_parser_error_pictures": (C.c_longlong, [C.c_void_p]),
    "lh264_parser_file_status": (C.c_int, [C.c_void_p]),
    "lh264_debug_slice_parse": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lh264_debug_slice_parse_opts": (C.c_int, [C.c_char_p, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "lh264_slice_dump_pictures": (C.c_int, [C.c_void_p]),
    "lh264_slice_dump_picture": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "lh264_slice_dump_mbs": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_slice_dump_coeffs": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_slice_dump_slices": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_slice_dump_results": (C.c_void_p, [C.c_void_p, C.c_int]),
    "lh264_slice_dump_guards_ok": (C.c_int, [C.c_void_p]),
    "lh264_slice_dump_error": (C.c_char_p, [C.c_void_p]),
    "lh264_slice_dump_free": (None, [C.c_void_p]),
})
EXPORTS = sorted(_SIGS)


def lib():
    """the loaded C-ABI library; raises LibraryMissing when it has not been built"""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise LibraryMissing("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % SO_PATH)
        try:
            import torch  # noqa: F401  -- load torch's bundled HIP runtime first so the process has exactly one
        except Exception:  # pragma: no cover
            pass
        L = C.CDLL(SO_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError("liblh264: error %d: %s" % (rc, lib().lh264_last_error().decode()))


def pic_geometry(mb_w, mb_h):
    sy, sc = C.c_int(), C.c_int()
    oy, ou, ov = C.c_size_t(), C.c_size_t(), C.c_size_t()
    total = lib().lh264_pic_bytes(mb_w, mb_h, C.byref(sy), C.byref(sc), C.byref(oy), C.byref(ou), C.byref(ov))
    return sy.value, sc.value, oy.value, ou.value, ov.value, total

def recon_geometry(max_mb_w, max_mb_h):
    """-> (status, waves, LDS bytes) of the reconstruct launch for pictures of at most this size (needs no device)"""
    nw, lds = C.c_int(), C.c_size_t()
    rc = lib().lh264_debug_recon_geometry(max_mb_w, max_mb_h, C.byref(nw), C.byref(lds))
    return rc, nw.value, lds.value


# ---- context-index (row a8) ----------------------------------------------------------------------------------
# row a10 syntax record (lh264_mbsyn_t, byte-packed)
MBSYN_DTYPE = np.dtype([
    ("have", "u1"), ("slice_type", "u1"), ("t8", "u1"), ("cbp_c", "u1"), ("cbp_l", "u1"), ("chroma_mode", "u1"),
    ("luma16_mode", "u1"), ("luma_qp", "u1"), ("mb_type", "<u4"), ("num_ref_idx_l0", "<u4"), ("skip_run", "<i4"),
    ("ref_idx", "i1", (4,)), ("sub_type", "u1", (4,)), ("pred_mode", "i1", (16,)), ("mvd", "<i2", (16, 2)),
    ("delta_qp", "<i4"), ("last_mb_qp", "<i4"),
])
assert MBSYN_DTYPE.itemsize == 116
CTX_SYM_DTYPE = np.dtype([("prior", "<u4"), ("value", "<i2"), ("kind", "u1"), ("pad", "u1")])
CTX_JOB_DTYPE = np.dtype([("mbs", "<u8"), ("levels", "<u8"), ("slices", "<u8"), ("nnz_past", "<u8"), ("nnz_cur", "<u8"),
                          ("syms", "<u8"), ("n_syms", "<u8"), ("mb_w", "<i4"), ("mb_h", "<i4"),
                          ("sym_off", "<u8"), ("sym_base", "<u8"), ("syms_cap", "<u8")])
CTX_MAX_SYMS = 432
assert CTX_SYM_DTYPE.itemsize == 8 and CTX_JOB_DTYPE.itemsize == 88
_SIGS["lh264_ctx_index_chains_keep"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p])
_SIGS["lh264_ctx_count_chains_keep"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p])
_SIGS["lh264_ctx_index_chains"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p])
_SIGS["lh264_ctx_count_chains"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p])
CODE_JOB_DTYPE = np.dtype([("syn_syms", "<u8"), ("syn_off", "<u8"), ("ctx_syms", "<u8"), ("ctx_n_syms", "<u8"), ("n_mbs", "<i4"), ("reserved", "<i4"),
                           ("ctx_sym_off", "<u8"), ("ctx_sym_base", "<u8")])
CODE_STREAM_DTYPE = np.dtype([("hash_keys", "<u8"), ("hash_cells", "<u8"), ("out", "<u8"), ("out_len", "<u8"), ("hash_cap", "<u4"), ("out_cap", "<u4")])
N_TAG_SLOTS = 40
assert CODE_JOB_DTYPE.itemsize == 56 and CODE_STREAM_DTYPE.itemsize == 40
_SIGS["lh264_code_chains"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p])
# ---- restore direction on the device
_SIGS["lh264_pip_restore_batch_device"] = (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p])
_SIGS["lh264_debug_restore_cpu"] = (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p])
_SIGS["lh264_pip_restore_batch_device_opts"] = (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
_SIGS["lh264_debug_restore_cpu_opts"] = (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p])
_SIGS["lh264_debug_dp_update"] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
_SIGS["lh264_restore_release"] = (None, [])
_SIGS["lh264_restore_last_timing"] = (C.c_int, [C.POINTER(C.c_double)])
_SIGS["lh264_debug_recon_geometry"] = (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t)])
EXPORTS = sorted(_SIGS)
