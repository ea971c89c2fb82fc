"""What tests/test_uncoded_t8.py and tests/test_uncoded_t8_gpu.py share: the committed streams of tests/golden/uncoded_t8/ (written by
tests/golden/make_uncoded_t8_streams.py), the reference's recorded verdict on them (tests/golden/uncoded_t8_ref.json), the host parser's
records of them and the oracle's pictures of those records."""
import functools
import hashlib
import json
import os

import numpy as np

import edge_cases as E
import golden_io
import oracle_lib as O
from losslessh264_amd import slice_parse as SP

DIR = os.path.join(golden_io.GOLDEN_DIR, "uncoded_t8")
REF = json.load(open(os.path.join(golden_io.GOLDEN_DIR, "uncoded_t8_ref.json")))
NAMES = sorted(REF)
STALE = "i8_cbp0_cavlc_i_stale"
# the one stream that may differ from the reference's pictures; nothing else may be added here
NOT_AS_THE_REFERENCE = (STALE,)
CABAC = [n for n in NAMES if n.endswith("_cabac")]
CAVLC = [n for n in NAMES if n not in CABAC]
MB_W, MB_H, N, PIC_BYTES = 4, 3, 12, 12 * 384
MB_I4, MB_I16, MB_I8, MB_P16x16, MB_P16x8, MB_P8x16, MB_P8x8, MB_SKIP, MB_IPCM = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x100, 0x200
CHROMA_QP = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]      # Table 8-15


def sha(b):
    return hashlib.sha1(bytes(b)).hexdigest()


def data(name):
    return E.data(name, DIR)


def made():
    return E.made("make_uncoded_t8_streams")


@functools.lru_cache(maxsize=None)
def parsed(name):
    """the host parser's pictures (records, coefficients, slice tables)"""
    return SP.parse_file_plain(data(name))


def cpu_compress(name):
    return E.cpu_compress(name, DIR)


def oracle_pictures(frames, qp_of=None):
    """the I420 bytes of every picture by the oracle's reconstruction of the records.  qp_of: {(picture, macroblock): (qp_y, qp_c)} to
    put in the place of what the records hold"""
    pics, out = {}, []
    for i, f in enumerate(frames):
        mbs = f.mbs
        if qp_of and any(p == i for p, _ in qp_of):
            mbs = mbs.copy()
            for (p, k), (qy, qc) in qp_of.items():
                if p == i:
                    mbs["qp_y"][k] = qy
                    mbs["qp_c"][k] = qc
        dst = O.HostPic(f.mb_w, f.mb_h)
        refs = [pics[r] if r in pics else dst for r in f.ref_ids]
        refs += [dst] * (16 - len(refs))
        O.recon_frame(mbs, f.coeffs, f.slices, dst, refs, 0)
        pics[f.id] = dst
        out.append(b"".join(np.ascontiguousarray(dst.plane(p)).tobytes() for p in range(3)))
    return out


@functools.lru_cache(maxsize=None)
def pictures(name):
    return oracle_pictures(parsed(name).frames)


def i8u(frames):
    """[(picture, macroblock)] of the I8x8 macroblocks without coefficients"""
    return [(i, int(k)) for i, f in enumerate(frames) for k in np.flatnonzero((f.mbs["mb_type"] == MB_I8) & (f.mbs["cbp"] == 0))]


def planes(picture):
    """one picture's I420 bytes as (Y, Cb, Cr) arrays"""
    a = np.frombuffer(picture, np.uint8)
    y, c = MB_W * 16 * MB_H * 16, MB_W * 8 * MB_H * 8
    return a[:y].reshape(MB_H * 16, MB_W * 16), a[y:y + c].reshape(MB_H * 8, MB_W * 8), a[y + c:].reshape(MB_H * 8, MB_W * 8)
