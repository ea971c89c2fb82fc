"""Float RGB pictures (lh264_decode_batch_ex2, a float sample type) where no device is present: the layout of lh264_decode_sample_t
and the arguments of the call and of Python; the factor sets the tests share and the edges each has to reach; the host stepping's
conversions to 16 bits at every boundary of both formats; the code of decode_pack_sample_kernel stepped on the host
(lh264_debug_sample_cpu) over the directed windows of tests/test_decode_rgb.py and windows of its own, against tests/sample_model.py
applied to the RGB bytes tests/rgb_model.py gives."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import rgb_model as M
import sample_model as SM
import scale_cases as SC
from test_decode_rgb import delivered_planes, directed, expect_rgb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
TYPES = ["float32", "float16", "bfloat16"]
LAYOUTS = ["rgb24", "rgbp"]
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def _lib():
    import __graft_entry__ as g
    g.build()
    from losslessh264_amd import _lib as L
    return L, L.lib()


# ---- the factor sets ------------------------------------------------------------------------------------------------------------------------
def factor_sets(type_name):
    """[(name, mul, add)] of binary32 triples, per type where a set's edge is one type's"""
    import losslessh264_amd as lh
    one, zero = (SM.f32(1),) * 3, (SM.f32(0),) * 3
    inv = SM.f32(1) / SM.f32(255)
    sets = [("identity", one, zero),
            ("imagenet",) + tuple(tuple(SM.f32(x) for x in t) for t in lh.normalise(*IMAGENET)),
            ("cancelling", (inv,) * 3, tuple(np.float32(-SM.f32(c0) * inv) for c0 in (37, 128, 200))),
            ("ties", one, (SM.f32(256 if type_name == "bfloat16" else 2048),) * 3),
            ("overflow", (SM.f32(300),) * 3, zero),
            ("half subnormals", (SM.f32(2.0 ** -20),) * 3, zero),
            ("single subnormals", (SM.f32(2.0 ** -140),) * 3, zero),
            ("minus, +0", (SM.f32(-1),) * 3, zero),
            ("minus, -0", (SM.f32(-1),) * 3, (SM.f32(-0.0),) * 3)]
    return sets


def test_normalise_and_the_factor_sets_reach_their_edges():
    """normalise is 1 / (255 * std) and -mean / std rounded once to binary32; and every shared factor set reaches the edge it is there
    for - a set that does not fails here"""
    import losslessh264_amd as lh
    mul, add = lh.normalise(*IMAGENET)
    for ch in range(3):
        m, s = IMAGENET[0][ch], IMAGENET[1][ch]
        assert mul[ch] == float(np.float32(1.0 / (255.0 * s))) and add[ch] == float(np.float32(-m / s))
    assert len(set(mul)) == 3 and len(set(add)) == 3                       # a swapped channel shows
    for bad in (((0, 0, 0), (1, 1, 0)), ((0, 0), (1, 1, 1)), ((0, 0, float("nan")), (1, 1, 1)), ((0, 0, 0), (1, float("inf"), 1))):
        with pytest.raises(ValueError):
            lh.normalise(*bad)
    sets = {t: {name: (mul, add) for name, mul, add in factor_sets(t)} for t in TYPES}
    c = np.arange(256)
    # identity: the bytes as floats, exact in all three types
    for t in TYPES:
        tab = SM.table(t, *sets[t]["identity"])
        want = np.arange(256, dtype=np.float32)
        want = want.view(np.uint32) if t == "float32" else SM.to_half_bits(want.view(np.uint32)) if t == "float16" else (want.view(np.uint32) >> 16).astype(np.uint16)
        assert all(np.array_equal(tab[ch], want) for ch in range(3)), t
    # cancelling: a multiply followed by an add gives other bits than the fused form in at least 32 of the 768 entries
    mul, add = sets["float32"]["cancelling"]
    fused = SM.table32(mul, add)
    split = np.stack([((c.astype(np.float32) * mul[ch]).astype(np.float32) + add[ch]).astype(np.float32).view(np.uint32) for ch in range(3)])
    assert int(np.count_nonzero(fused != split)) >= 32 and len(set(SM.bits_of(a) for a in add)) == 3
    # at c0 itself the split form cancels to +0; the fused form keeps what rounding -c0 * mul left over (nothing where c0 is a power of 2)
    assert all(split[ch][c0] == 0 for ch, c0 in enumerate((37, 128, 200))) and fused[1][128] == 0 and fused[0][37] != 0 and fused[2][200] != 0
    # ties: every odd result lies halfway between two values of the type, and goes to the even one
    for t, base in (("float16", 2048), ("bfloat16", 256)):
        tab = SM.table(t, *sets[t]["ties"])[0]
        val = tab.view(np.float16).astype(np.float64) if t == "float16" else (tab.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        odd = c[1::2]
        assert np.all(np.abs(val[odd] - (base + odd)) == 1) and np.all(val[::2] == base + c[::2])
        assert np.all((val[odd] / 2) % 2 == 0)                                      # the even mantissa of the two neighbours
    # overflow: binary16 is infinity from c = 219, finite below; the other types stay finite
    tab = SM.table("float16", *sets["float16"]["overflow"])[1]
    assert np.all(tab[219:] == 0x7c00) and np.all(tab[:219] < 0x7c00) and tab[218] == 0x7bfc
    assert np.all((SM.table("bfloat16", *sets["bfloat16"]["overflow"]) & 0x7f80) != 0x7f80)
    # subnormals: binary16 for 0 < c < 64 under 2^-20, binary32 and bfloat16 for every c > 0 under 2^-140 - and none is flushed
    tab = SM.table("float16", *sets["float16"]["half subnormals"])[2]
    assert np.all((tab[1:64] & 0x7c00) == 0) and np.all(tab[1:64] != 0) and np.all((tab[64:] & 0x7c00) != 0) and tab[1] == 0x0010
    tab = SM.table("float32", *sets["float32"]["single subnormals"])[0]
    assert np.all((tab[1:] & 0x7f800000) == 0) and np.all(tab[1:] != 0) and tab[1] == 1 << 9 and tab[255] == 255 << 9
    tab = SM.table("bfloat16", *sets["bfloat16"]["single subnormals"])[0]
    # (bfloat16's smallest subnormal is 2^-133: c = 64 and c = 192 are ties, to 0 and to 2 * 2^-133)
    assert np.all((tab[1:] & 0x7f80) == 0) and set(tab.tolist()) == {0, 1, 2} and [int(tab[k]) for k in (64, 65, 191, 192, 255)] == [0, 1, 1, 2, 2]
    assert np.all(SM.table("float16", *sets["float16"]["single subnormals"]) == 0)
    # the sign of zero at c = 0
    for t, top in (("float32", 31), ("float16", 15), ("bfloat16", 15)):
        assert SM.table(t, *sets[t]["minus, +0"])[0][0] == 0 and SM.table(t, *sets[t]["minus, -0"])[0][0] == 1 << top, t
        assert SM.table(t, *sets[t]["minus, +0"])[0][1] == SM.table(t, *sets[t]["minus, -0"])[0][1] != 0


def test_the_model_rounds_once():
    """the exact fused multiply-add against cases done by hand: a product that needs rounding, a float64 sum that would round twice"""
    assert SM.fma_bits(3, 1, 2048) == SM.bits_of(2051.0) and SM.fma_bits(255, 2.0 ** -140, 0) == 255 << 9
    m = np.float32(1 + 2.0 ** -23)                                          # 255 * m = 255 + 255 * 2^-23: 31 bits, rounded to 24
    assert SM.fma_bits(255, m, 0) == SM.bits_of(np.float32(255.0 * float(m)))
    # 3 * (1 + 2^-23) - 3 = 3 * 2^-23 exactly; a multiply rounded to binary32 first gives 2^-21 (3 + 3 * 2^-23 rounds to 3 + 2^-21)
    assert SM.fma_bits(3, m, -3.0) == SM.bits_of(3 * 2.0 ** -23)
    assert SM.bits_of(np.float32(np.float32(3) * m) + np.float32(-3)) == SM.bits_of(2.0 ** -21)
    assert SM.round_to_binary32(SM.F(2) ** 128 - SM.F(2) ** 103) == 0x7f800000 and SM.round_to_binary32(SM.F(2) ** 128 - SM.F(2) ** 103 - 1) == 0x7f7fffff
    assert SM.round_to_binary32(SM.F(1, 2 ** 150)) == 0 and SM.round_to_binary32(SM.F(3, 2 ** 150)) == 2 and SM.round_to_binary32(SM.F(3, 2 ** 151)) == 1 and SM.round_to_binary32(-SM.F(1, 2 ** 149)) == 0x80000001


# ---- the struct and the arguments of the call ---------------------------------------------------------------------------------------------
def test_layout_of_the_sample_struct():
    """sizeof 32 with struct_bytes, type, mul, add at 0, 4, 8, 20, by a C compiler and in the mirror; the constants; the frozen structs
    are still 88 and 24 bytes, the ABI version 3, and COLOUR / MATRIX / RANGE what they were"""
    L, lib = _lib()
    S = L.DecodeSample
    names = ["struct_bytes", "type", "mul", "add"]
    assert C.sizeof(S) == 32 and [getattr(S, n).offset for n in names] == [0, 4, 8, 20]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lh264.h"\nint main(void){ printf("%zu %zu %zu ", sizeof(lh264_decode_sample_t), sizeof(lh264_decode_ext_t), sizeof(lh264_decode_opts_t));\n' + \
          "".join('printf("%%zu ", offsetof(lh264_decode_sample_t, %s));\n' % n for n in names) + \
          'printf("%zu %u %u %u %u %d\\n", sizeof(((lh264_decode_sample_t*)0)->mul[0]), LH264_SAMPLE_U8, LH264_SAMPLE_F32, LH264_SAMPLE_F16, LH264_SAMPLE_BF16, LH264_ABI_VERSION); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    assert out == ["32", "24", "88", "0", "4", "8", "20", "4", "0", "1", "2", "3", "3"]
    assert L.SAMPLE == {"uint8": 0, "float32": 1, "float16": 2, "bfloat16": 3} and L.SAMPLE == dict(SM.TYPES, uint8=0)
    assert (L.COLOUR, L.MATRIX, L.RANGE) == ({None: 0, "rgb24": 1, "rgbp": 2}, {"auto": 0, "bt601": 1, "bt709": 2}, {"auto": 0, "limited": 1, "full": 2})
    assert lib.lh264_abi_version() == 3
    for name in ("lh264_decode_batch_ex2", "lh264_decoded_sample_type", "lh264_debug_sample_cpu", "lh264_debug_sample_dev"):
        assert hasattr(lib, name) and name in L.EXPORTS, name
    assert lib.lh264_decoded_sample_type(None) == L.E_ARG


def _sample(L, **kw):
    s = L.DecodeSample()
    s.struct_bytes = 32
    for k, v in kw.items():
        if k in ("mul", "add"):
            for q in range(3):
                getattr(s, k)[q] = v[q]
        else:
            setattr(s, k, v)
    return s


def test_arguments_are_checked_before_the_device():
    """every LH264_E_ARG case of the sample struct is reported on a machine without a device and leaves `out` alone; sample == NULL and
    type U8 with clear floats are accepted exactly as lh264_decode_batch_ex is, and so is every float type beside a colour"""
    L, lib = _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    ptrs, lens = (C.c_char_p * 1)(data), (C.c_size_t * 1)(len(data))
    outs = (C.c_void_p * 1)()
    sentinel = 0x4321

    def call(o, e, s):
        outs[0] = sentinel
        rc = lib.lh264_decode_batch_ex2(ptrs, lens, 1, 1, C.byref(o) if o is not None else None, C.byref(e) if e is not None else None, C.byref(s) if s is not None else None, outs)
        if rc == 0:
            lib.lh264_decoded_free(outs[0])
        else:
            assert outs[0] == sentinel
        return rc
    import torch
    accepted = 0 if torch.cuda.is_available() else L.E_NODEVICE
    o = L.DecodeOptsV6()
    o.struct_bytes = 88

    def ext(**kw):
        e = L.DecodeExt()
        e.struct_bytes = 24
        for k, v in kw.items():
            setattr(e, k, v)
        return e
    inf, nan = float("inf"), float("nan")
    one, zero = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    for opts in (None, o):
        for e in (None, ext(), ext(colour=1), ext(colour=2, matrix=2, range=1)):
            assert call(opts, e, None) == accepted and call(opts, e, _sample(L)) == accepted
        for colour in (1, 2):
            for t in (1, 2, 3):
                assert call(opts, ext(colour=colour), _sample(L, type=t, mul=one, add=zero)) == accepted, (colour, t)
                assert call(opts, ext(colour=colour), _sample(L, type=t, mul=(-0.0, 3e38, 1e-45), add=(-3e38, -0.0, 0.0))) == accepted      # finite is enough
        for nbytes in (0, 4, 8, 24, 28, 31, 33, 36, 40, 88):
            assert call(opts, ext(colour=1), _sample(L, struct_bytes=nbytes)) == L.E_ARG, nbytes
            assert call(opts, ext(colour=1), _sample(L, struct_bytes=nbytes, type=1, mul=one)) == L.E_ARG, nbytes
            assert call(opts, None, _sample(L, struct_bytes=nbytes)) == L.E_ARG, nbytes
        for t in (4, 5, 255, 0x80000000, 0xffffffff):
            assert call(opts, ext(colour=1), _sample(L, type=t, mul=one)) == L.E_ARG, t
        for k in range(3):                                              # U8 with a float that is not +0.0: -0.0 has a bit set
            for v in (1.0, -0.0, 1e-45, nan):
                for field in ("mul", "add"):
                    bad = [0.0] * 3
                    bad[k] = v
                    assert call(opts, ext(colour=1), _sample(L, **{field: bad})) == L.E_ARG, (field, k, v)
                    assert call(opts, None, _sample(L, **{field: bad})) == L.E_ARG, (field, k, v)
        for t in (1, 2, 3):                                             # a float type needs a colour
            assert call(opts, None, _sample(L, type=t, mul=one)) == L.E_ARG and call(opts, ext(), _sample(L, type=t, mul=one)) == L.E_ARG, t
            for k in range(3):
                for v in (inf, -inf, nan):
                    for field in ("mul", "add"):
                        bad = [1.0] * 3
                        bad[k] = v
                        assert call(opts, ext(colour=2), _sample(L, type=t, **{field: bad, "add" if field == "mul" else "mul": one})) == L.E_ARG, (t, field, k, v)
        # the other structs' rules hold beside a sample
        assert call(opts, ext(struct_bytes=20, colour=1), _sample(L, type=1, mul=one)) == L.E_ARG
        assert call(opts, ext(colour=3), _sample(L, type=1, mul=one)) == L.E_ARG and call(opts, ext(colour=1, reserved0=1), _sample(L, type=1, mul=one)) == L.E_ARG
    o.format = L.FMT_NV12
    assert call(o, ext(colour=1), _sample(L, type=1, mul=one)) == L.E_ARG and call(o, None, _sample(L)) == accepted
    o.format = L.FMT_I420
    o.reserved5 = 1
    assert call(o, ext(colour=1), _sample(L, type=2, mul=one)) == L.E_ARG
    o.reserved5 = 0
    o.flags = L.DECODE_SHA1_PICTURES | L.DECODE_SHA1_STREAM | L.DECODE_NO_PICTURES
    o.out_width, o.out_height, o.parse, o.parse_flags, o.pick = 224, 224, 1, L.PARSE_FLAG_CABAC, 2
    assert call(o, ext(colour=2, range=2), _sample(L, type=3, mul=one)) == accepted
    o.out_width = o.out_height = o.pick = 0
    o.scale_log2, o.conceal, o.flags = 3, L.CONCEAL["slice_copy"], L.DECODE_DEVICE_OUT
    assert call(o, ext(colour=1, matrix=2), _sample(L, type=2, mul=one)) == accepted
    for nbytes in (72, 64, 56, 48, 40):
        o.struct_bytes = nbytes
        assert call(o, ext(colour=1), _sample(L, type=1, mul=one)) == accepted, nbytes


def test_python_refuses_bad_sample_keywords():
    import losslessh264_amd as lh
    _lib()
    data = open(os.path.join(STREAMS, "BA_MW_D.264"), "rb").read()
    inf = float("inf")
    for kw in (dict(dtype="float32"), dict(dtype="float16", fmt="nv12", colour="rgb24"), dict(colour="rgb24", dtype="float64"), dict(colour="rgb24", dtype="half"),
               dict(colour="rgb24", dtype=None), dict(colour="rgb24", dtype=1), dict(colour="rgbp", dtype="uint8", mul=(1, 1, 1)), dict(colour="rgbp", add=(0, 0, 0)),
               dict(mul=(1, 1, 1)), dict(colour="rgb24", dtype="float32", mul=(1, 1)), dict(colour="rgb24", dtype="float32", mul=1.0), dict(colour="rgb24", dtype="float32", add=(0, 0, 0, 0)),
               dict(colour="rgb24", dtype="bfloat16", mul=(1, inf, 1)), dict(colour="rgb24", dtype="bfloat16", add=(0, 0, float("nan"))), dict(colour="rgb24", dtype="float16", mul=(1, 1e39, 1)),
               dict(colour="rgb24", dtype="float16", mul=("1", 1, 1)), dict(colour="rgb24", dtype="float16", add=(True, 0, 0)), dict(colour="rgb24", dtype="float32", mul="abc")):
        with pytest.raises(ValueError):
            lh.decode_batch([data], **kw)
    b = lh.DecodedBatch(None, [], True, None, (224, 224), "rgbp")
    assert b.dtype == "uint8" and b.affine is None
    from losslessh264_amd import decode as D
    assert D._three(None, 1.0, "mul") == (1.0, 1.0, 1.0) and D._three((0.1, 2, np.float32(3)), 0.0, "add") == (float(np.float32(0.1)), 2.0, 3.0)


# ---- the host stepping's conversions ------------------------------------------------------------------------------------------------------
def _round(L, lib, type_name, values):
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros(v.size, dtype=np.uint16)
    assert lib.lh264_debug_sample_round(L.SAMPLE[type_name], v.ctypes.data, v.size, out.ctypes.data) == 0
    return out


def test_the_host_conversions_are_nearest_even():
    """lh264_debug_sample_round against the model at every boundary of both 16-bit formats: for every pair of neighbouring values of
    the format the binary32 halfway between them, the binary32 values next to it on either side and the pair itself, in both signs;
    the zeros, everything below half of the smallest subnormal, the overflow threshold, infinity; and 2^20 random bit patterns"""
    L, lib = _lib()
    rng = np.random.default_rng(7)
    for t, conv in (("float16", SM.to_half_bits), ("bfloat16", SM.to_bfloat_bits)):
        pos = np.arange(0, 0x7c00 if t == "float16" else 0x7f80, dtype=np.uint32)       # every finite non-negative value of the format, in order
        as32 = pos.astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32) if t == "float16" else pos << 16
        lo, hi = as32[:-1].astype(np.uint64), as32[1:].astype(np.uint64)
        if t == "float16":
            mid = ((lo.astype(np.uint32).view(np.float32).astype(np.float64) + hi.astype(np.uint32).view(np.float32).astype(np.float64)) / 2).astype(np.float32).view(np.uint32).astype(np.uint64)
        else:
            mid = (lo + hi) // 2                                            # neighbouring bfloat16 patterns: the binary32 pattern between them
        top = np.uint64(SM.bits_of(65520.0) if t == "float16" else 0x7f7f8000)           # halfway between the largest value and 2^16 / 2^128
        cand = np.concatenate([lo, hi, mid, mid - 1, mid + 1, np.array([0, 1, 2, top - 1, top, top + 1, 0x7f7fffff, 0x7f800000], dtype=np.uint64),
                               rng.integers(0, 0x7f800000, 1 << 20, dtype=np.uint64)]).astype(np.uint32)
        cand = np.concatenate([cand, cand | np.uint32(0x80000000)])
        got, want = _round(L, lib, t, cand.view(np.float32)), conv(cand)
        assert np.array_equal(got, want), (t, [hex(x) for x in cand[np.flatnonzero(got != want)[:8]]])
        assert want[cand == top][0] == (0x7c00 if t == "float16" else 0x7f80) and want[cand == top - 1][0] == (0x7bff if t == "float16" else 0x7f7f)
    assert lib.lh264_debug_sample_round(0, None, 0, None) == L.E_ARG and lib.lh264_debug_sample_round(1, None, 0, None) == L.E_ARG and lib.lh264_debug_sample_round(2, None, 1, None) == L.E_ARG


# ---- directed windows through the kernel's code -----------------------------------------------------------------------------------------
JOBS = [(off, std) for off in (0, 4, 8, 12) for std in range(4)]      # one table: every destination offset from a 16-byte boundary with every standard


def windows():
    """the directed windows of tests/test_decode_rgb.py and, at full size, delivered widths 2..18 with height 2: a row that is only a
    tail, tails of one to three pairs behind one or two whole items, rows of whole items only (8, 16), rows that begin 4, 12, 20, .. bytes behind one another"""
    if not hasattr(windows, "memo"):
        windows.memo = directed() + [("%dx2" % w, SC.Case(w, 2, 0, 0, seed=61 + k), [("scale", 0)]) for k, w in enumerate((2, 4, 6, 10, 14, 18, 8, 16))]
    return windows.memo


def slot_bytes(case, sizing, type_name):
    y = delivered_planes(case, sizing)[0]
    return (SC.GUARD + 16 + 3 * y.size * SM.ELEMENT_BYTES[type_name] + SC.GUARD + 15) & ~15


def run_table(L, fn, case, sizing, layout, type_name, mul, add, src_ptr, dst_ptr, slot):
    """one call of a float entry point with a job per (destination offset, standard), job k's picture at dst_ptr + k * slot + GUARD +
    off -> [(first byte of job k's picture, its expected bytes)]"""
    jobs = (L.PackJob * len(JOBS))()
    std = (C.c_uint8 * len(JOBS))(*[s for _, s in JOBS])
    at = []
    for k, (off, s) in enumerate(JOBS):
        at.append(k * slot + SC.GUARD + off)
        case.fill_job(jobs[k], src_ptr, dst_ptr + at[k], L.FMT_I420, sizing[1] if sizing[0] == "scale" else 0)
    ow, oh = sizing[1] if sizing[0] == "size" else (0, 0)
    sm = _sample(L, type=L.SAMPLE[type_name], mul=[float(x) for x in mul], add=[float(x) for x in add])
    assert fn(jobs, len(JOBS), ow, oh, M.LAYOUTS[layout], std, C.byref(sm)) == 0
    tab = SM.table(type_name, mul, add)
    return [(at[k], SM.apply_picture(expect_rgb(case, sizing, layout, s), layout, tab)) for k, (_, s) in enumerate(JOBS)]


def check_table(got, placed, what):
    mask = np.ones(got.size, dtype=bool)
    for at, exp in placed:
        assert np.array_equal(got[at:at + exp.size], exp), (what, np.flatnonzero(got[at:at + exp.size] != exp)[:8])
        mask[at:at + exp.size] = False
    assert np.all(got[mask] == 0xa5), what


def aligned(n, fill=0xa5):
    """n bytes of `fill` that begin at a multiple of 16"""
    buf = np.full(n + 16, fill, dtype=np.uint8)
    base = (-buf.ctypes.data) % 16
    return buf[base:base + n]


@pytest.mark.parametrize("type_name", TYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sample_pack_on_the_host(layout, type_name):
    """every window under every sizing with every factor set: destinations 0, 4, 8 and 12 bytes from a 16-byte boundary, the four
    standards side by side in one table; the bytes are the model's and the 0xA5 around every destination is intact.  Delivered widths
    with ow mod 8 in 0, 2, 4 and 6, rows that begin at every multiple of 4 modulo 16"""
    L, lib = _lib()
    tails, starts = set(), set()
    es = SM.ELEMENT_BYTES[type_name]
    for name, case, sizings in windows():
        for sizing in sizings:
            slot = slot_bytes(case, sizing, type_name)
            oh, ow = delivered_planes(case, sizing)[0].shape
            tails.add(ow % 8)
            starts |= {(off + r * (3 if layout == "rgb24" else 1) * ow * es) % 16 for off, _ in JOBS for r in range(oh)}
            for fname, mul, add in factor_sets(type_name):
                buf = aligned(slot * len(JOBS))
                placed = run_table(L, lib.lh264_debug_sample_cpu, case, sizing, layout, type_name, mul, add, case.buf.ctypes.data, buf.ctypes.data, slot)
                check_table(buf, placed, (name, sizing, layout, type_name, fname))
    assert tails == {0, 2, 4, 6} and starts == {0, 4, 8, 12}


def test_the_debug_entry_points_check_their_arguments():
    """what the RGB entry points refuse, a sample struct the call refuses or that names uint8 or is NULL, and a destination that is no
    multiple of 4 are LH264_E_ARG from both entry points and nothing is written; lh264_debug_sample_dev without a device is
    LH264_E_NODEVICE"""
    L, lib = _lib()
    case = SC.Case(16, 16, 0, 0)
    buf = aligned(8192)
    j = L.PackJob()
    case.fill_job(j, case.buf.ctypes.data, buf.ctypes.data + 64, L.FMT_I420, 0)
    std = (C.c_uint8 * 1)(0)
    one = (1.0, 1.0, 1.0)
    good = _sample(L, type=1, mul=one)
    for fn in (lib.lh264_debug_sample_cpu, lib.lh264_debug_sample_dev):
        for layout in (0, 3, -1):
            assert fn(C.byref(j), 1, 0, 0, layout, std, C.byref(good)) == L.E_ARG, layout
        for bad in ((16, 0), (15, 16), (4098, 16), (1, 1)):
            assert fn(C.byref(j), 1, bad[0], bad[1], 1, std, C.byref(good)) == L.E_ARG, bad
        assert fn(None, 1, 0, 0, 1, std, C.byref(good)) == L.E_ARG and fn(C.byref(j), 0, 0, 0, 1, std, C.byref(good)) == L.E_ARG and fn(C.byref(j), 1, 0, 0, 1, None, C.byref(good)) == L.E_ARG
        std[0] = 4
        assert fn(C.byref(j), 1, 0, 0, 1, std, C.byref(good)) == L.E_ARG
        std[0] = 0
        j.format = L.FMT_NV12
        assert fn(C.byref(j), 1, 0, 0, 1, std, C.byref(good)) == L.E_ARG
        j.format = L.FMT_I420
        assert fn(C.byref(j), 1, 0, 0, 1, std, None) == L.E_ARG
        for s in (_sample(L), _sample(L, type=4, mul=one), _sample(L, type=1, mul=one, struct_bytes=24), _sample(L, type=2, mul=(1.0, float("inf"), 1.0)), _sample(L, type=3, mul=one, add=(0.0, 0.0, float("nan")))):
            assert fn(C.byref(j), 1, 0, 0, 1, std, C.byref(s)) == L.E_ARG
        for off in (1, 2, 3, 5, 6, 7):
            j.dst = buf.ctypes.data + 64 + off
            assert fn(C.byref(j), 1, 0, 0, 2, std, C.byref(good)) == L.E_ARG, off
        j.dst = buf.ctypes.data + 64
    assert np.all(buf == 0xa5)
    import torch
    if not torch.cuda.is_available():
        assert lib.lh264_debug_sample_dev(C.byref(j), 1, 0, 0, 1, std, C.byref(good)) == L.E_NODEVICE
        assert np.all(buf == 0xa5)
    assert lib.lh264_debug_sample_cpu(C.byref(j), 1, 0, 0, 1, std, C.byref(good)) == 0 and not np.all(buf == 0xa5)


# ---- the command lines --------------------------------------------------------------------------------------------------------------------
def test_the_command_lines_refuse_bad_sample_options(tmp_path):
    """--sample takes f32 | f16 | bf16 and needs --rgb, --mul and --add take three finite numbers and need --sample: anything else ends
    both command lines with the usage code before a stream is read or a device looked for"""
    src = os.path.join(STREAMS, "BA_MW_D.264")
    _lib()
    bad = [["--sample", "f32"], ["--sample", "f16", "--mul", "1,1,1"], ["--rgb", "rgb24", "--sample", "f64"], ["--rgb", "rgb24", "--sample", "float32"], ["--rgb", "rgbp", "--sample", ""],
           ["--rgb", "rgb24", "--mul", "1,1,1"], ["--rgb", "rgb24", "--add", "0,0,0"], ["--rgb", "rgb24", "--sample", "f32", "--mul", "1,1"], ["--rgb", "rgb24", "--sample", "f32", "--mul", "1,1,1,1"],
           ["--rgb", "rgb24", "--sample", "bf16", "--add", "0,x,0"], ["--rgb", "rgb24", "--sample", "f16", "--mul", "1,inf,1"], ["--rgb", "rgb24", "--sample", "f16", "--add", "nan,0,0"],
           ["--rgb", "rgb24", "--sample", "f16", "--mul", "1,1e39,1"], ["--rgb", "rgb24", "--sample", "f32", "--mul", ""], ["--sample", "f32", "--nv12"]]
    for cmd in ([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"]):
        for args in bad:
            r = subprocess.run(cmd + ["--decode"] + args + [str(tmp_path), src], capture_output=True, timeout=120, cwd=ROOT)
            assert r.returncode == 2 and b"--sample: f32 | f16 | bf16" in r.stdout + r.stderr, (cmd, args, r.stdout, r.stderr)
            assert os.listdir(str(tmp_path)) == []
