"""The host side of coding a stream in segments (no device): the new entry points are exported with the documented signatures, the
carry block's size follows the table's, the batch call with options answers as the call without where there is no device, and the
parser hands a file's pictures out segment by segment with the records, levels and symbol lists of the whole parse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lh264_code_carry_bytes", "lh264_code_chains_resume", "lh264_code_carry_decisions", "lh264_code_last_decisions",
       "lh264_compress_batch_opts", "lh264_compress_batch_devices_opts", "lh264_compressed_segments", "lh264_compressed_decisions",
       "lh264_compress_arena_bytes", "lh264_parser_begin_file", "lh264_parser_feed_file_some", "lh264_parser_drop_frames"]


def _lib():
    import __graft_entry__ as g
    g.build()
    from losslessh264_amd import _lib
    return _lib


def test_new_entry_points_are_declared_exported_and_bound():
    L = _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lh264.h")).read(), flags=re.S)
    lib = L.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared in include/lh264.h"
        assert hasattr(lib, name) and name in L.EXPORTS, name
    # the documented signatures, as the header spells them
    flat = " ".join(hdr.split())
    assert "size_t lh264_code_carry_bytes (uint32_t hash_cap);" in flat
    assert re.search(r"int lh264_code_chains_resume \(const lh264_code_job_t\* jobs_dev, const int32_t\* chain_first_dev, const lh264_code_stream_t\* "
                     r"streams_dev, void\* const\* carry_dev, const uint32_t\* flags_dev, int n_chains, int n_jobs, long long total_mbs, int "
                     r"max_mbs_per_frame, void\* hip_stream\);", flat)
    assert "typedef struct lh264_compress_opts { uint32_t struct_bytes; uint32_t reserved; uint64_t segment_mbs; } lh264_compress_opts_t;" in flat
    assert "uint64_t lh264_compressed_decisions (const lh264_compressed_t* c, int tag);" in flat
    assert "int lh264_compress_arena_bytes (size_t* device, size_t* pinned);" in flat
    assert C.sizeof(L.CompressOpts) == 16
    assert lib.lh264_abi_version() == 3                     # nothing an existing caller sees has changed


def test_carry_bytes_grow_with_the_table():
    lib = _lib().lib()
    sizes = [lib.lh264_code_carry_bytes(1 << k) for k in range(0, 21)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    assert all(s >= (64 << k) for k, s in enumerate(sizes))            # the block holds the table: hash_cap x 64 bytes
    assert sizes[20] - (64 << 20) == sizes[0] - 64 and sizes[0] - 64 < 4096      # ... and a fixed header of tag records


def test_batch_call_with_options_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib()
    lib = L.lib()
    data = open(os.path.join(golden_io.GOLDEN_DIR, "streams", "BA_MW_D.264"), "rb").read()
    n = 2
    ptrs = (C.c_char_p * n)(data, data)
    lens = (C.c_size_t * n)(len(data), len(data))
    for opts in (None, L.CompressOpts(C.sizeof(L.CompressOpts), 0, 0), L.CompressOpts(C.sizeof(L.CompressOpts), 0, 99)):
        outs = (C.c_void_p * n)()
        rc = lib.lh264_compress_batch_opts(ptrs, lens, n, 2, C.byref(opts) if opts else None, outs)
        outs0 = (C.c_void_p * n)()
        assert rc == lib.lh264_compress_batch(ptrs, lens, n, 2, outs0) == -1          # LH264_E_NODEVICE
        for a, b in zip(outs, outs0):
            assert lib.lh264_compressed_status(a) == lib.lh264_compressed_status(b) == -1
            assert lib.lh264_compressed_error(a) == lib.lh264_compressed_error(b)
            assert lib.lh264_compressed_segments(a) == 0 and lib.lh264_compressed_decisions(a, 2) == 0
            lib.lh264_compressed_free(a); lib.lh264_compressed_free(b)
    # a struct_bytes this library does not know
    for bad in (0, 8, 24):
        outs = (C.c_void_p * n)()
        opts = L.CompressOpts(bad, 0, 0)
        assert lib.lh264_compress_batch_opts(ptrs, lens, n, 2, C.byref(opts), outs) == -2         # LH264_E_ARG
        assert not any(outs)
    assert lib.lh264_code_chains_resume(None, None, None, None, None, 1, 1, 1, 1, None) == -1
    assert lib.lh264_code_last_decisions(0, 0, None) == -1
    assert lib.lh264_compress_arena_bytes(None, None) == -1


FIELDS = ["mbs", "levels", "slices", "covered", "syn", "slice_syn", "syn_syms", "syn_off"]


@pytest.mark.parametrize("name", ["BA_MW_D.264", "test_cif_P_CABAC_slice.264", "SVA_BA2_D.264", "syn720p_allI_4slices.264"])
def test_parser_hands_pictures_out_in_segments(name):
    """a CAVLC stream, a CABAC one with several slices a picture, and a 720p one with four: pictures, levels and symbol lists segment by
    segment equal those of the whole parse, as does the default stream; no segment is over its size except a single picture"""
    import losslessh264_amd as lh
    data = open(os.path.join(golden_io.GOLDEN_DIR, "streams", name), "rb").read()
    whole, err, main = lh.parse_file(data)
    assert err == "" and len(whole) > 1
    if "CABAC" in name or "4slices" in name:
        assert max(len(f.slices) for f in whole) > 1
    pic = whole[0].mb_w * whole[0].mb_h
    for seg_mbs in (1, pic, 3 * pic, 3 * pic + 5, 10 ** 9):
        got, sizes, tail = [], [], None
        for item in lh.parse_file_segments(data, seg_mbs):
            if isinstance(item, tuple):
                tail = item
            else:
                assert item, "an empty segment"
                sizes.append(sum(f.mb_w * f.mb_h for f in item))
                assert len(item) == 1 or sizes[-1] <= seg_mbs
                got += item
        assert tail == (err, main)
        assert len(got) == len(whole), (seg_mbs, len(got), len(whole))
        assert len(sizes) == (1 if seg_mbs == 10 ** 9 else len(whole) if seg_mbs <= pic else len(sizes))
        if seg_mbs == 3 * pic and all(f.mb_w * f.mb_h == pic for f in whole):
            assert len(sizes) == (len(whole) + 2) // 3
        for a, b in zip(got, whole):
            assert (a.id, a.mb_w, a.mb_h, a.frame_num, a.ref_ids, a.is_ref, a.idr) == (b.id, b.mb_w, b.mb_h, b.frame_num, b.ref_ids, b.is_ref, b.idr)
            for k in FIELDS:
                assert np.array_equal(getattr(a, k), getattr(b, k)), (name, seg_mbs, a.id, k)
