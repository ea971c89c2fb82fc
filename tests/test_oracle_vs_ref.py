"""Pin the oracle (oracle/liboracle.so, our C restatement) against the REFERENCE's own C kernels.

Same pattern as the reference's unit tests (random blocks vs. anchor): test/decoder/DecUT_IdctResAddPred.cpp:7-108,
DecUT_IntraPrediction.cpp, DecUT_DeblockCommon.cpp:258-415, test/encoder/EncUT_MotionCompensation.cpp:12-260,
test/common/ExpandPicture.cpp:111-199.  Bit-exact comparison (integer work): every case below feeds seeded inputs to the oracle
and, given the reference's kernels (oracle/_ref/libref_kernels.so, built by oracle/Makefile), to the reference as well.  The tests
compare the oracle's outputs with the SHA-1 of the reference's outputs on the same inputs, tests/golden/ref_kernels_sha1.json,
which tests/golden/make_golden_ref_kernels.py writes after comparing the two output by output.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as O

REF_SHA1 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kernels_sha1.json")


def _agree(h, a, b, what=None):
    """a: the oracle's output, b: the reference's on the same input (None: only the digest of the reference's outputs is known)"""
    if b is not None:
        assert np.array_equal(a, b), what
    h.update(np.ascontiguousarray(a).tobytes())


def _check(name, case, *args):
    h = hashlib.sha1()
    r = case(O.lib(), None, h, *args)
    assert h.hexdigest() == json.load(open(REF_SHA1))[name], "%s: the oracle's outputs differ from the reference's" % name
    return r


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the cases: (oracle, reference or None, digest) -> the oracle's outputs into the digest, compared with the reference's ----------
def _idct4x4(orc, ref, h):
    rng = np.random.default_rng(1)
    for it in range(2000):
        amp = [16, 256, 2048, 32767][it % 4]
        coef = rng.integers(-amp, amp + 1, 16).astype(np.int16)
        if it % 7 == 0:
            coef[rng.integers(0, 16, 12)] = 0
        a = rng.integers(0, 256, (4, 32)).astype(np.uint8)
        b = a.copy()
        orc.orc_idct4x4_add(_p(a), 32, _p(coef.copy()))
        if ref:
            ref.refk_idct4x4_add(_p(b), 32, _p(coef.copy()))
        _agree(h, a, b if ref else None)


def _idct8x8(orc, ref, h):
    rng = np.random.default_rng(2)
    for it in range(1000):
        amp = [16, 256, 2048, 32767][it % 4]
        coef = rng.integers(-amp, amp + 1, 64).astype(np.int16)
        a = rng.integers(0, 256, (8, 32)).astype(np.uint8)
        b = a.copy()
        orc.orc_idct8x8_add(_p(a), 32, _p(coef.copy()))
        if ref:
            ref.refk_idct8x8_add(_p(b), 32, _p(coef.copy()))
        _agree(h, a, b if ref else None)


def _dc_transforms(orc, ref, h):
    rng = np.random.default_rng(3)
    for it in range(1000):
        qp = int(rng.integers(0, 52))
        blk = rng.integers(-2048, 2048, 384).astype(np.int16)
        a, b = blk.copy(), blk.copy()
        orc.orc_luma_dc_dequant_idct(_p(a), orc.orc_luma_dc_qmul(qp, 16))
        if ref:
            ref.refk_luma_dc_dequant_idct(_p(b), qp)
        _agree(h, a, b if ref else None)
        a, b = blk.copy(), blk.copy()
        orc.orc_chroma_dc_idct(_p(a[256:]))
        if ref:
            ref.refk_chroma_dc_idct(_p(b[256:]))
        _agree(h, a, b if ref else None)


def _intra_pred(orc, ref, h, kind, nmodes, size):
    rng = np.random.default_rng(4)
    st = 64
    for it in range(300):
        for mode in range(nmodes):
            img = rng.integers(0, 256, (40, st)).astype(np.uint8)
            a, b = img.copy(), img.copy()
            off = 8 * st + 16
            getattr(orc, "orc_" + kind)(C.c_void_p(a.ctypes.data + off), st, mode)
            if ref:
                getattr(ref, "refk_" + kind)(C.c_void_p(b.ctypes.data + off), st, mode)
            _agree(h, a, b if ref else None, (kind, mode))


def _intra_pred8x8l(orc, ref, h):
    rng = np.random.default_rng(5)
    st = 64
    for it in range(200):
        for mode in range(14):
            for tl in (0, 1):
                for tr in (0, 1):
                    img = rng.integers(0, 256, (40, st)).astype(np.uint8)
                    a, b = img.copy(), img.copy()
                    off = 8 * st + 16
                    orc.orc_pred8x8l(C.c_void_p(a.ctypes.data + off), st, mode, tl, tr)
                    if ref:
                        ref.refk_pred8x8l(C.c_void_p(b.ctypes.data + off), st, mode, tl, tr)
                    _agree(h, a, b if ref else None, (mode, tl, tr))


def _mc(orc, ref, h):
    rng = np.random.default_rng(6)
    st = 64
    sizes = [(16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4)]
    for it in range(40):
        src = rng.integers(0, 256, (48, st)).astype(np.uint8)
        if it % 5 == 0:
            src[:] = rng.choice([0, 255], src.shape)      # saturating content
        for (w, hh) in sizes:
            for mvx in range(4):
                for mvy in range(4):
                    a = np.zeros((16, 32), np.uint8)
                    b = a.copy()
                    sp = C.c_void_p(src.ctypes.data + 8 * st + 8)
                    orc.orc_mc_luma(sp, st, _p(a), 32, mvx, mvy, w, hh)
                    if ref:
                        ref.refk_mc_luma(sp, st, _p(b), 32, mvx, mvy, w, hh)
                    _agree(h, a, b if ref else None, (w, hh, mvx, mvy))
            for mvx in range(8):
                for mvy in range(8):
                    a = np.zeros((16, 32), np.uint8)
                    b = a.copy()
                    sp = C.c_void_p(src.ctypes.data + 8 * st + 8)
                    orc.orc_mc_chroma(sp, st, _p(a), 32, mvx, mvy, w >> 1, hh >> 1)
                    if ref:
                        ref.refk_mc_chroma(sp, st, _p(b), 32, mvx, mvy, w >> 1, hh >> 1)
                    _agree(h, a, b if ref else None, (w, hh, mvx, mvy))


def _deblock_edge_filters(orc, ref, h):
    rng = np.random.default_rng(7)
    st = 32
    for it in range(3000):
        base = int(rng.integers(0, 256))
        spread = [2, 6, 20, 255][it % 4]
        img = np.clip(base + rng.integers(-spread, spread + 1, (24, st)), 0, 255).astype(np.uint8)
        alpha, beta = int(rng.integers(0, 256)), int(rng.integers(0, 19))
        tc = rng.integers(-1, 26, 4).astype(np.int8)
        vert = it & 1
        off = 8 * st + 8
        for name, args in (("luma_lt4", True), ("luma_eq4", False), ("chroma_lt4", True), ("chroma_eq4", False)):
            a, b = img.copy(), img.copy()
            xs, ys = (1, st) if vert else (st, 1)
            if args:
                getattr(orc, "orc_deblock_" + name)(C.c_void_p(a.ctypes.data + off), xs, ys, alpha, beta, _p(tc))
                if ref:
                    getattr(ref, "refk_deblock_" + name)(C.c_void_p(b.ctypes.data + off), st, vert, alpha, beta, _p(tc))
            else:
                getattr(orc, "orc_deblock_" + name)(C.c_void_p(a.ctypes.data + off), xs, ys, alpha, beta)
                if ref:
                    getattr(ref, "refk_deblock_" + name)(C.c_void_p(b.ctypes.data + off), st, vert, alpha, beta)
            _agree(h, a, b if ref else None, (name, vert))


def _deblock_macroblock_drivers(orc, ref, h):
    """-> the number of intra macroblocks with Cb QP != Cr QP (where the reference's stale iTc shows)"""
    import synth
    cases = [dict(seed=11, p_frames=False), dict(seed=12, p_frames=True), dict(seed=13, p_frames=True, t8=True),
             dict(seed=14, p_frames=True, n_slices=3, idc=3), dict(seed=15, p_frames=False, t8=True, n_slices=2, idc=2),
             dict(seed=16, p_frames=True, pcm=True)]
    n_stale = 0
    for kw in cases:
        seed = kw.pop("seed")
        for f in synth.make_stream(seed, 7, 5, 3, **kw):
            rng = np.random.default_rng(1000 + seed + f.id)
            a = O.HostPic(f.mb_w, f.mb_h, fill=0)
            base = rng.integers(40, 216)
            for p in range(3):      # smooth content with small steps at block edges: every branch of the filters is reached
                pl = a.plane(p)
                pl[:] = np.clip(base + rng.integers(-9, 10, pl.shape) + 6 * ((np.arange(pl.shape[1]) // 4) % 3)[None, :], 0, 255)
            b = O.HostPic(f.mb_w, f.mb_h, fill=0)
            b.buf[:] = a.buf
            mbs = np.ascontiguousarray(f.mbs); sl = np.ascontiguousarray(f.slices)
            sa = a.struct()
            for si in range(len(sl)):
                orc.orc_deblock_slice(_p(mbs), _p(sl), si, C.byref(sa), f.mb_w, f.mb_h)
            if ref:
                sb = b.struct()
                ref.refk_deblock_picture(_p(mbs), _p(sl), f.mb_w, f.mb_h, C.c_void_p(sb.y), C.c_void_p(sb.u), C.c_void_p(sb.v), sb.stride_y, sb.stride_c)
            for p in range(3):
                _agree(h, a.plane(p), b.plane(p) if ref else None, (seed, f.id, p))
            intra = (mbs["mb_type"] & 0x207) != 0
            n_stale += int(np.count_nonzero(intra & (mbs["qp_c"][:, 0] != mbs["qp_c"][:, 1])))
    return n_stale


def _expand(orc, ref, h):
    rng = np.random.default_rng(8)
    for (mb_w, mb_h) in [(1, 1), (3, 2), (11, 9), (20, 15)]:
        a = O.HostPic(mb_w, mb_h, fill=0)
        a.buf[:] = rng.integers(0, 256, a.buf.shape)
        b = O.HostPic(mb_w, mb_h, fill=0)
        b.buf[:] = a.buf
        sa = a.struct()
        orc.orc_expand_pic(C.byref(sa), mb_w, mb_h)
        if ref:
            sb = b.struct()
            ref.refk_expand_picture(C.c_void_p(sb.y), C.c_void_p(sb.u), C.c_void_p(sb.v), mb_w * 16, mb_h * 16, sb.stride_y, sb.stride_c)
        _agree(h, a.buf, b.buf if ref else None)


def _luma_dc_scaling_list(orc, ref, h):
    """WelsLumaDcDequantIdct with a scaling list (decode_slice.cpp:272: kiQMul = pDequant_coeff4x4[0][qp][0] >> 4), QP 0..50, weights
    1..255, amplitudes up to the bound that keeps f * kiQMul inside int32.  The reference keeps weight * dequant as uint16_t
    (decoder_context.h:446-448), so kiQMul is ((weight * dq) & 0xffff) >> 4: the oracle's transform is run with that factor, and
    orc_luma_dc_qmul must give it wherever the product fits 16 bits.  -> the number of inputs whose product does not fit.
    (Row 51 of the table is never written, decode_slice.cpp:1260: QP 51 is left out.)"""
    rng = np.random.default_rng(21)
    norm = [10, 11, 13, 14, 16, 18]
    had = [(1, 1, 1, 1), (1, 1, -1, -1), (1, -1, -1, 1), (1, -1, 1, -1)]
    blk_x, blk_y = [0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3], [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3]
    n_trunc = 0
    for it in range(1530):
        qp = it % 51
        weight = [1, 6, 15, 17, 64, 255][(it // 51) % 6] if it % 2 else int(rng.integers(1, 256))
        dq = norm[qp % 6] << (qp // 6)
        qmul = ((weight * dq) & 0xffff) >> 4
        if weight * dq < 65536:
            assert orc.orc_luma_dc_qmul(qp, weight) == qmul, (qp, weight)
        else:
            n_trunc += 1
        amp = min(32767, ((1 << 31) - 3) // (16 * max(qmul, 1)))
        blk = rng.integers(-amp, amp + 1, 384).astype(np.int16)
        if it % 5 == 0:                  # the sign patterns that put 16 * amp into one output
            for zb in range(16):
                blk[zb * 16] = amp * had[it % 4][blk_x[zb]] * had[(it // 4) % 4][blk_y[zb]] * (-1 if it & 16 else 1)
        a, b = blk.copy(), blk.copy()
        orc.orc_luma_dc_dequant_idct(_p(a), qmul)
        if ref:
            ref.refk_luma_dc_dequant_idct_weighted(_p(b), qp, weight)
        _agree(h, a, b if ref else None, (qp, weight, amp))
    return n_trunc


def _weight_prediction(orc, ref, h):
    """WeightPrediction (rec_mb.cpp:276-341) at the ends of its syntax: denominators 0, 1, 7, weights and offsets -128, -1, 0, 1, 127 and
    random ones, every partition size; the chroma quirk (only the top-left quarter is weighted) included"""
    from refdump import SLICE_DTYPE
    rng = np.random.default_rng(22)
    sizes = [(16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4)]
    ext = [-128, -1, 0, 1, 127]
    for it in range(1260):
        w, hh = sizes[it % 7]
        ld, cd = ([0, 1, 7][(it // 7) % 3], [0, 1, 7][(it // 21) % 3]) if it % 4 else (int(rng.integers(0, 8)), int(rng.integers(0, 8)))
        v = [int(rng.choice(ext)) if rng.random() < 0.6 else int(rng.integers(-128, 128)) for _ in range(6)]
        sl = np.zeros(1, dtype=SLICE_DTYPE)
        sl["weighted_pred"], sl["luma_log2_denom"], sl["chroma_log2_denom"] = 1, ld, cd
        sl["luma_weight"][0, 3], sl["luma_offset"][0, 3] = v[0], v[1]
        sl["chroma_weight"][0, 3], sl["chroma_offset"][0, 3] = v[2:4], v[4:6]
        planes = [rng.integers(0, 256, (16, 32)).astype(np.uint8), rng.integers(0, 256, (8, 16)).astype(np.uint8), rng.integers(0, 256, (8, 16)).astype(np.uint8)]
        if it % 6 == 0:
            planes = [np.where(rng.random(q.shape) < 0.5, 0, 255).astype(np.uint8) for q in planes]
        a, b = [q.copy() for q in planes], [q.copy() for q in planes]
        orc.orc_weight_pred(_p(a[0]), _p(a[1]), _p(a[2]), 32, 16, w, hh, _p(sl), 3)
        if ref:
            ref.refk_weight_prediction(_p(b[0]), _p(b[1]), _p(b[2]), 32, 16, w, hh, ld, cd, v[0], v[1], (C.c_int * 2)(*v[2:4]), (C.c_int * 2)(*v[4:6]))
        for q in range(3):
            _agree(h, a[q], b[q] if ref else None, (w, hh, ld, cd, v, q))


def _bs_thresholds(orc, ref, h):
    """the boundary-strength cases of tests/recon_directed.py (vectors 3 and 4 apart across every edge, reference indices, the
    8x8-transform remaps, P16x16, SKIP) through the reference's macroblock drivers: the unfiltered picture of each case, filtered by both"""
    import recon_directed as D
    for c in D.bs_thresholds():
        pics = {}
        for f in c.frames:
            refs = [pics[r] for r in f.ref_ids]
            pics[f.id] = O.HostPic(f.mb_w, f.mb_h)
            O.recon_frame(f.mbs, f.coeffs, f.slices, pics[f.id], refs, 0)
        a = O.HostPic(f.mb_w, f.mb_h)
        O.recon_frame(f.mbs, f.coeffs, f.slices, a, refs, O.NO_DEBLOCK | O.NO_EXPAND)
        b = O.HostPic(f.mb_w, f.mb_h)
        b.buf[:] = a.buf
        mbs = np.ascontiguousarray(f.mbs); sl = np.ascontiguousarray(f.slices)
        sa = a.struct()
        orc.orc_deblock_slice(_p(mbs), _p(sl), 0, C.byref(sa), f.mb_w, f.mb_h)
        if ref:
            sb = b.struct()
            ref.refk_deblock_picture(_p(mbs), _p(sl), f.mb_w, f.mb_h, C.c_void_p(sb.y), C.c_void_p(sb.u), C.c_void_p(sb.v), sb.stride_y, sb.stride_c)
        for p in range(3):
            _agree(h, a.plane(p), b.plane(p) if ref else None, (c.name, p))


def _deblock_directed(orc, ref, h):
    """the directed filter pictures of tests/deblock_directed.py (thresholds, table entries, the three QP lookups, the stale tc0, short
    cuts, order, slices): the unfiltered picture of each, filtered by the oracle's and by the reference's macroblock drivers"""
    import deblock_directed as DD
    n = 0
    for fam, scenes in DD.families().items():
        for s in scenes:
            frames = s.frames()
            pics = {}
            for f in frames:
                refs = [pics[r] for r in f.ref_ids]
                pics[f.id] = O.HostPic(f.mb_w, f.mb_h)
                O.recon_frame(f.mbs, f.coeffs, f.slices, pics[f.id], refs, 0)
                a = O.HostPic(f.mb_w, f.mb_h)
                O.recon_frame(f.mbs, f.coeffs, f.slices, a, refs, O.NO_DEBLOCK | O.NO_EXPAND)
                b = O.HostPic(f.mb_w, f.mb_h)
                b.buf[:] = a.buf
                mbs = np.ascontiguousarray(f.mbs); sl = np.ascontiguousarray(f.slices)
                sa = a.struct()
                for si in range(len(sl)):
                    orc.orc_deblock_slice(_p(mbs), _p(sl), si, C.byref(sa), f.mb_w, f.mb_h)
                for p in range(3):
                    assert np.array_equal(a.plane(p), pics[f.id].plane(p)), (s.name, f.id, p)   # slice by slice == the frame driver
                if ref:
                    sb = b.struct()
                    ref.refk_deblock_picture(_p(mbs), _p(sl), f.mb_w, f.mb_h, C.c_void_p(sb.y), C.c_void_p(sb.u), C.c_void_p(sb.v), sb.stride_y, sb.stride_c)
                for p in range(3):
                    _agree(h, a.plane(p), b.plane(p) if ref else None, (s.name, f.id, p))
                n += 1
    return n


def _intra_directed(orc, ref, h):
    """the predictors at the directed edge contents of tests/intra_directed.py, where uniform random images do not reach: binary
    samples, the steepest ramps of both signs in both directions (|H| = |V| = 9180: both clips of the plane predictors, negative sums
    under the arithmetic shift), gentle ramps, sums that all differ, and two neighbouring values (every residue of the roundings);
    every mode, for 8x8 every top-left and top-right setting.  -> the number of predictions"""
    import intra_directed as ID
    rng = np.random.default_rng(23)
    st, off = 64, 8 * 64 + 16
    n = 0
    for cls in list(ID.CLASSES) + ["ties"]:
        for it in range(12):
            for kind, nmodes, size in INTRA_PRED + [("pred8x8l", 14, 8)]:
                top, left = ID.edge_vectors(rng, cls, size)
                img = rng.integers(0, 256, (40, st)).astype(np.uint8)
                img[7, 15:15 + len(top)] = top              # p[-1..2 size - 1, -1] of the block at (16, 8)
                img[8:8 + size, 15] = left
                for mode in range(nmodes):
                    for tl, tr in ([(0, 0), (0, 1), (1, 0), (1, 1)] if kind == "pred8x8l" else [(None, None)]):
                        a, b = img.copy(), img.copy()
                        extra = () if tl is None else (tl, tr)
                        getattr(orc, "orc_" + kind)(C.c_void_p(a.ctypes.data + off), st, mode, *extra)
                        if ref:
                            getattr(ref, "refk_" + kind)(C.c_void_p(b.ctypes.data + off), st, mode, *extra)
                        _agree(h, a, b if ref else None, (cls, kind, mode, tl, tr))
                        n += 1
    return n


INTRA_PRED = [("pred4x4", 14, 4), ("pred16x16", 7, 16), ("predc8x8", 7, 8)]
# digest name -> (case, its arguments): what tests/golden/make_golden_ref_kernels.py runs against the reference
CASES = {"idct4x4": (_idct4x4, ()), "idct8x8": (_idct8x8, ()), "dc_transforms": (_dc_transforms, ()),
         **{"intra_pred[%s]" % k[0]: (_intra_pred, k) for k in INTRA_PRED}, "intra_pred8x8l": (_intra_pred8x8l, ()), "mc": (_mc, ()),
         "deblock_edge_filters": (_deblock_edge_filters, ()), "deblock_macroblock_drivers": (_deblock_macroblock_drivers, ()),
         "expand": (_expand, ()),
         "luma_dc_scaling_list": (_luma_dc_scaling_list, ()), "weight_prediction": (_weight_prediction, ()), "bs_thresholds": (_bs_thresholds, ()),
         "deblock_directed": (_deblock_directed, ()), "intra_directed": (_intra_directed, ())}


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def test_idct4x4():
    _check("idct4x4", _idct4x4)


def test_idct8x8():
    _check("idct8x8", _idct8x8)


def test_dc_transforms():
    _check("dc_transforms", _dc_transforms)


@pytest.mark.parametrize("kind,nmodes,size", INTRA_PRED)
def test_intra_pred(kind, nmodes, size):
    _check("intra_pred[%s]" % kind, _intra_pred, kind, nmodes, size)


def test_intra_pred8x8l():
    _check("intra_pred8x8l", _intra_pred8x8l)


def test_mc():
    _check("mc", _mc)


def test_deblock_edge_filters():
    _check("deblock_edge_filters", _deblock_edge_filters)


def test_deblock_macroblock_drivers():
    """WelsDeblockingMb / DeblockingIntraMb / DeblockingInterMb with the boundary-strength derivation (deblocking.cpp:160-352,
    568-862) over whole synthetic pictures (the pattern of test/decoder/DecUT_DeblockCommon.cpp:417-979): random macroblock types,
    QPs with Cb != Cr, coefficients, vectors, reference indices, 8x8 transform, non-zero alpha / beta offsets, several slices with
    disable_deblocking_filter_idc 0 / 1 / 2.  Includes the reference's stale-iTc inner chroma edge of intra macroblocks (:786-807)."""
    n_stale = _check("deblock_macroblock_drivers", _deblock_macroblock_drivers)
    assert n_stale > 50         # the quirk's precondition is exercised


def test_expand():
    _check("expand", _expand)


def test_luma_dc_scaling_list():
    n_trunc = _check("luma_dc_scaling_list", _luma_dc_scaling_list)
    assert n_trunc > 100        # products beyond 16 bits take part (see the case)


def test_weight_prediction():
    _check("weight_prediction", _weight_prediction)


def test_bs_thresholds():
    _check("bs_thresholds", _bs_thresholds)


def test_deblock_directed():
    assert _check("deblock_directed", _deblock_directed) > 300


def test_intra_directed():
    assert _check("intra_directed", _intra_directed) == 9 * 12 * (14 + 7 + 7 + 4 * 14)
