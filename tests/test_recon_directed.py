"""The directed inputs of tests/recon_directed.py reach what they claim: shown with the oracle alone (CPU).  The device runs of the same
inputs are in tests/test_recon_directed_gpu.py."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import oracle_lib as O
import recon_directed as D
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = np.array([1, -5, 20, 20, -5, 1])


def oracle_stream(frames, flags=0):
    """every picture of a chain through the oracle (references: the finished pictures) -> list of HostPic"""
    pics, out = {}, []
    for f in frames:
        refs = [pics[r] for r in f.ref_ids]
        dst = O.HostPic(f.mb_w, f.mb_h)
        O.recon_frame(f.mbs, f.coeffs, f.slices, dst, refs, 0)
        pics[f.id] = dst
        if flags:
            dst = O.HostPic(f.mb_w, f.mb_h)
            O.recon_frame(f.mbs, f.coeffs, f.slices, dst, refs, flags)
        out.append(dst)
    return out


def partitions(f, k):
    """(ox, oy, w, h, mvx, mvy) of macroblock k's partitions"""
    m = f.mbs[k]
    typ, sub = int(m["mb_type"]), int(m["sub_type"][0])
    shape = [s for s, (t, st, _) in D.SHAPES.items() if t == typ and (typ != synth.P8x8 or st == sub)][0]
    return [(ox, oy, w, h, int(m["mv"][(oy >> 2) * 4 + (ox >> 2)][0]), int(m["mv"][(oy >> 2) * 4 + (ox >> 2)][1])) for (ox, oy, w, h) in D.SHAPES[shape][2]]


def clamped(f, k, ox, oy, mvx, mvy):
    lo, hx, hy = D.clamp_bounds(f.mb_w, f.mb_h)
    x, y = k % f.mb_w, k // f.mb_w
    return min(max(4 * (16 * x + ox) + mvx, lo), hx), min(max(4 * (16 * y + oy) + mvy, lo), hy)


# ---- pcm_picture ----------------------------------------------------------------------------------------------------------------------
def test_pcm_picture_is_its_planes():
    rng = np.random.default_rng(1)
    y, u, v = D.content_uniform(rng, 48, 80), D.content_uniform(rng, 24, 40), D.content_binary(rng, 24, 40)
    pic = oracle_stream([D.pcm_picture(5, 3, y, u, v)])[0]
    for p, want in enumerate((y, u, v)):
        assert np.array_equal(pic.plane(p), want)


# ---- mc_grid --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(D.SHAPES))
def test_mc_grid_covers_fractions_and_alignments(shape):
    """Every shape meets all 16 luma and all 64 chroma fractions and every byte alignment of the kernel's fetches.  The alignments are
    computed as the kernel computes them (inter_phase): the luma fetch of a 4x4 block starts at plane + syy * stride + sx - 2, the
    chroma fetch at plane + cys * stride + cxs.  Assumption: planes are 4-byte aligned - the strides of pic_geometry are multiples
    of 32 / 16, the plane offsets multiples of 4, and ReconSession places pictures at multiples of 256 in one device allocation.
    Of the 16 pairs (luma alignment, chroma alignment) only 8 exist: both are functions of the block's integer column s modulo 8,
    (s - 2) & 3 and (s >> 1) & 3; all 8 are met.  Each alignment is met with each fraction of its own plane."""
    _, f = D.mc_grid(shape, "uniform")
    sy, sc, off_y, off_u, off_v, _ = O.pic_geometry(f.mb_w, f.mb_h)
    assert sy % 4 == 0 and sc % 4 == 0 and off_y % 4 == 0 and off_u % 4 == 0 and off_v % 4 == 0
    lfr, cfr, pairs, l_al_fx, c_al_dx, signs = set(), set(), set(), set(), set(), set()
    for k in range(len(f.mbs)):
        for (ox, oy, w, h, mvx, mvy) in partitions(f, k):
            assert (mvx, mvy) == (k % 64 - 32, k // 64 - 8)
            fx, fy = clamped(f, k, ox, oy, mvx, mvy)
            assert (fx, fy) == (4 * (16 * (k % 64) + ox) + mvx, 4 * (16 * (k // 64) + oy) + mvy)       # no vector of the grid is clamped
            lfr.add((fx & 3, fy & 3)); cfr.add((fx & 7, fy & 7)); signs.add((mvx < 0, mvy < 0))
            for bx in range(0, w, 4):
                sx, cxs = (fx >> 2) + bx, (fx >> 3) + (bx >> 1)
                lsh, csh = (sx - 2) & 3, cxs & 3
                pairs.add((lsh, csh)); l_al_fx.add((lsh, fx & 3)); c_al_dx.add((csh, fx & 7))
    assert len(lfr) == 16 and len(cfr) == 64 and len(signs) == 4
    assert pairs == {((s - 2) & 3, (s >> 1) & 3) for s in range(8)} and len(pairs) == 8
    assert len(l_al_fx) == 16 and len(c_al_dx) == 32


def test_mc_grid_mixed_puts_different_fractions_into_one_macroblock():
    for shape in D.SHAPES:
        _, f = D.mc_grid(shape, "uniform", mixed=True)
        n_parts = len(D.SHAPES[shape][2])
        mixed_fy = some_zero = 0
        for k in range(len(f.mbs)):
            ps = partitions(f, k)
            assert [(p[4], p[5]) for p in ps] == [(k % 64 - 32 + 5 * i, k // 64 - 8 + 3 * i) for i in range(n_parts)]
            fys = {p[5] & 3 for p in ps}
            mixed_fy += len(fys) > 1
            some_zero += (0 in fys) and len(fys) > 1
        if n_parts > 1:
            assert mixed_fy > 500 and some_zero > 200          # strips with and without a vertical fraction in one wave (any_fy)


def test_tap_extreme_content_reaches_the_ends_of_the_filters():
    """over the windows the grid reads on the tap-extreme content, the 6-tap sums reach +10,710 and -2,550 vertically and horizontally,
    and the centre position both clips of (x + 512) >> 10"""
    ref, f = D.mc_grid("16x16", "tap_extreme")
    pic = oracle_stream([ref])[0].padded_plane(0).astype(np.int64)
    v_ext, h_ext, centre = set(), set(), set()
    for k in range(len(f.mbs)):
        (ox, oy, w, h, mvx, mvy), = partitions(f, k)
        fx, fy = clamped(f, k, ox, oy, mvx, mvy)
        x0, y0 = (fx >> 2) + D.PAD, (fy >> 2) + D.PAD
        win = pic[y0 - 2:y0 + 16 + 3, x0 - 2:x0 + 16 + 3]
        vs = sum(TAPS[i] * win[i:i + 16, :] for i in range(6))          # vertical sums of rows 0..15, columns -2..18
        hs = sum(TAPS[i] * win[:, i:i + 16] for i in range(6))
        if fy & 3:
            v_ext.update((int(vs[:, 2:18].max()), int(vs[:, 2:18].min())))
        if fx & 3:
            h_ext.update((int(hs[2:18].max()), int(hs[2:18].min())))
        if (fx & 3) == 2 and (fy & 3) == 2:
            j = sum(TAPS[i] * vs[:, i:i + 16] for i in range(6))
            centre.update((int(j.max() + 512) >> 10, int(j.min() + 512) >> 10))
    assert max(v_ext) == 10710 and min(v_ext) == -2550
    assert max(h_ext) == 10710 and min(h_ext) == -2550
    assert max(centre) > 255 and min(centre) < 0


# ---- mc_border ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb_w,mb_h", [(1, 1), (2, 2), (3, 2)])
def test_mc_border_reads_the_outermost_padding(mb_w, mb_h):
    """Every case lands where it says: on a bound of BaseMC's clamp, 1..3 quarter samples inside it, or 1 beyond (clamped back).  Inside
    the low bound the 6-tap window starts at sample -32, the outermost padded column / row.  At the high bound the outermost sample a
    window can reach is W + 30 (H + 30): the clamp stops at integer position W + 13 with fraction 0 (window W + 13 .. W + 28), and from
    position W + 12 with a fraction the window ends at W + 12 + 15 + 3; sample W + 31 is never read.  Both are asserted as such."""
    frames, cases = D.mc_border(mb_w, mb_h)
    lo, hx, hy = D.clamp_bounds(mb_w, mb_h)
    W, H = 16 * mb_w, 16 * mb_h
    assert len(cases) == 80
    seen = set()
    for (fi, k, name, shape) in cases:
        f = frames[fi]
        ps = partitions(f, k)
        assert len(ps) == (1 if shape == "16x16" else 16)
        d = int(name[-2:])
        for (ox, oy, w, h, mvx, mvy) in ps:
            ax, ay = 4 * (16 * (k % mb_w) + ox) + mvx, 4 * (16 * (k // mb_w) + oy) + mvy
            fx, fy = clamped(f, k, ox, oy, mvx, mvy)
            x_lo, x_hi = name.startswith(("x_lo", "tl", "bl")), name.startswith(("x_hi", "tr", "br"))
            y_lo, y_hi = name.startswith(("y_lo", "tl", "tr")), name.startswith(("y_hi", "bl", "br"))
            if x_lo: assert ax == lo - d and fx == max(ax, lo)
            if x_hi: assert ax == hx + d and fx == min(ax, hx)
            if y_lo: assert ay == lo - d and fy == max(ay, lo)
            if y_hi: assert ay == hy + d and fy == min(ay, hy)
            first_x, last_x = (fx >> 2) - (2 if fx & 3 else 0), (fx >> 2) + w - 1 + (3 if fx & 3 else 0)
            first_y, last_y = (fy >> 2) - (2 if fy & 3 else 0), (fy >> 2) + h - 1 + (3 if fy & 3 else 0)
            assert -32 <= first_x and last_x <= W + 30 and -32 <= first_y and last_y <= H + 30
            if d < 0:                                          # inside the bound: a fraction, and the window at the outermost sample
                if x_lo: assert first_x == -32
                if y_lo: assert first_y == -32
                if x_hi and w == 16: assert last_x == W + 30
                if y_hi and h == 16: assert last_y == H + 30
            seen.add((name, shape))
    assert len(seen) == 80


# ---- bs_thresholds --------------------------------------------------------------------------------------------------------------------
def test_bs_thresholds_decide_the_filter():
    """For every pair, the filter changes the samples beside the edge where the vectors differ by 4 and leaves them alone where they
    differ by 3: a wrong threshold, or a wrong block index in the 8x8-transform remaps, shows in those samples.  Two reference indices
    that name one picture: the edge IS filtered - MB_BS_MV compares the indices, not the pictures (deblocking.cpp:58-63)."""
    cases = D.bs_thresholds()
    names = {c.name for c in cases}
    assert len(names) == len(cases)
    for c in cases:
        fin = oracle_stream(c.frames)[-1].plane(0)
        pre = oracle_stream(c.frames, O.NO_DEBLOCK)[-1].plane(0)
        changed = bool((D.edge_samples(fin, c.edge) != D.edge_samples(pre, c.edge)).any())
        assert changed == c.filtered, c.name
        if c.name.endswith("/3"):
            assert not c.filtered and (c.name[:-1] + "4") in names
        if c.name.endswith("/4"):
            assert c.filtered
    one = [c for c in cases if "one picture" in c.name]
    assert len(one) == 4 and all(c.filtered for c in one)
    for c in one:
        f = c.frames[-1]
        assert f.slices["ref_slot"][0, 0] == f.slices["ref_slot"][0, 1] == 0 and set(f.mbs["ref_idx"].ravel()) == {0, 1}
    for key in ("internal 4x4", "internal 8x8", "internal 16x8", "internal 8x16", "mb edge dir0", "mb edge dir1", "t8 cur1 nb0", "t8 cur0 nb1",
                "t8 cur1 nb1", "t8 nz remap", "P16x16 internal", "SKIP internal", "two pictures"):
        assert any(key in n for n in names), key


# ---- row_masks ------------------------------------------------------------------------------------------------------------------------
def _recompute_mb(f, k, base, refs):
    """macroblock k alone over a copy of the unfiltered picture `base` -> its three blocks"""
    L = O.lib()
    pic = O.HostPic(f.mb_w, f.mb_h)
    pic.buf[:] = base.buf
    sl = np.concatenate([f.slices, f.slices[:1]])
    sl[-1]["first_mb"], sl[-1]["n_mbs"] = k, 1
    arr = (O.OrcPic * 16)()
    for i, r in enumerate(refs):
        arr[i] = r.struct()
    d = pic.struct()
    mbs, co = np.ascontiguousarray(f.mbs), np.ascontiguousarray(f.coeffs)
    L.orc_recon_slice(mbs.ctypes.data_as(C.c_void_p), co.ctypes.data_as(C.c_void_p), sl.ctypes.data_as(C.c_void_p), len(sl) - 1,
                      C.byref(d), arr, f.mb_w, f.mb_h)
    x, y = k % f.mb_w, k // f.mb_w
    return [pic.plane(p)[y * bs:(y + 1) * bs, x * bs:(x + 1) * bs].copy() for p, bs in ((0, 16), (1, 8), (2, 8))]


def _stale(base, f, x, y, what):
    """a copy of `base` in which the bottom row (what 'row') or right column ('col') of macroblock (x, y) holds other values"""
    pic = O.HostPic(f.mb_w, f.mb_h)
    pic.buf[:] = base.buf
    for p, bs in ((0, 16), (1, 8), (2, 8)):
        pl = pic.plane(p)
        if what == "row":
            pl[(y + 1) * bs - 1, x * bs:(x + 1) * bs] ^= 0x80
        else:
            pl[y * bs:(y + 1) * bs, (x + 1) * bs - 1] ^= 0x80
    return pic


@pytest.mark.parametrize("mb_w", D.MASK_WIDTHS)
def test_row_masks_place_intra_macroblocks_that_read_their_neighbours(mb_w):
    """every listed column carries an isolated intra macroblock in row 1 and in row 2 of some picture, and each of them reads what the
    rows' masks decide about: with other values in the bottom row of the macroblock above-left, above or above-right, or in the right
    column of the left neighbour, the oracle's prediction changes - a line the kernel did not publish would show."""
    frames = D.row_masks(mb_w)
    D.check_refs_defined(frames)
    pre = oracle_stream(frames, O.NO_DEBLOCK | O.NO_EXPAND)
    fin = oracle_stream(frames)
    seen = {1: set(), 2: set()}
    kinds = set()
    for fi, f in enumerate(frames[1:], 1):
        intra = (f.mbs["mb_type"] & 7) != 0
        for r in (1, 2):
            cols = sorted(np.nonzero(intra[r * mb_w:(r + 1) * mb_w])[0])
            assert cols == sorted(f.placed[r]) and all(b - a >= 5 for a, b in zip(cols, cols[1:]))
            seen[r].update(cols)
        assert not intra[:mb_w].any()
        assert all(abs(a - b) >= 2 for a in f.placed[1] for b in f.placed[2])
        refs = [fin[fi - 1]]
        for r in (1, 2):
            for c in f.placed[r]:
                k = r * mb_w + c
                m = f.mbs[k]
                want = _recompute_mb(f, k, pre[fi], refs)
                for p, bs in ((0, 16), (1, 8), (2, 8)):
                    assert np.array_equal(want[p], pre[fi].plane(p)[r * bs:(r + 1) * bs, c * bs:(c + 1) * bs])
                typ, plane_l, plane_c = int(m["mb_type"]), int(m["intra_mode"][0]) == 3, int(m["chroma_mode"]) == 3
                kinds.add((typ, plane_l, plane_c))
                reads = [(c, r - 1, "row")]
                if c > 0:
                    reads += [(c - 1, r, "col"), (c - 1, r - 1, "row")]
                if c + 1 < mb_w and typ in (synth.I4, synth.I8):
                    reads.append((c + 1, r - 1, "row"))
                for (nx, ny, what) in reads:
                    got = _recompute_mb(f, k, _stale(pre[fi], f, nx, ny, what), refs)
                    assert any(not np.array_equal(g, w_) for g, w_ in zip(got, want)), (fi, r, c, typ, nx, ny, what)
    want_cols = set(D.mask_columns(mb_w))
    assert seen[1] == want_cols and seen[2] == want_cols
    assert {62, mb_w - 1} <= want_cols and (mb_w < 66 or {63, 64, 65} <= want_cols) and (mb_w < 129 or {126, 127, 128} <= want_cols)
    if mb_w >= 65:
        assert kinds >= {(synth.I4, False, False), (synth.I8, False, False), (synth.I16, True, False), (synth.I16, False, True)}


@pytest.mark.parametrize("mb_w", [63, 130])
def test_row_masks_complement(mb_w):
    frames = D.row_masks(mb_w, complement=True)
    D.check_refs_defined(frames)
    seen = {1: set(), 2: set()}
    for f in frames[1:]:
        inter = (f.mbs["mb_type"] & 0x1F8) != 0
        for r in (1, 2):
            cols = sorted(np.nonzero(inter[r * mb_w:(r + 1) * mb_w])[0])
            assert cols == sorted(f.placed[r])
            seen[r].update(cols)
        assert not inter[:mb_w].any()
    assert seen[1] == seen[2] == set(D.mask_columns(mb_w))
    oracle_stream(frames)


# ---- wave counts ----------------------------------------------------------------------------------------------------------------------
class _WgLds(C.Structure):          # struct WgLds of lh264_kernels.hip
    _fields_ = [("progress", C.c_int * 16), ("stored", C.c_int * 16), ("tab", C.c_uint8 * (52 + 52 + 208))]


class _WaveLds(C.Structure):        # struct WaveLds of lh264_kernels.hip
    _fields_ = [("T", C.c_uint8 * (20 * 32)), ("C", C.c_uint8 * (2 * 10 * 16)), ("R", C.c_int16 * 384), ("rec", C.c_uint32 * 64), ("trec", C.c_uint32 * 32),
                ("slc", C.c_uint32 * 58), ("leftY", C.c_uint8 * 16), ("leftC", C.c_uint8 * 16), ("lfY", C.c_uint32 * 20), ("lfC", C.c_uint32 * 20),
                ("mvi", C.c_int32 * 64), ("bs", C.c_uint8 * 32), ("E", C.c_uint8 * 32), ("S", C.c_int32 * 64), ("refp", C.c_uint64 * 48),
                ("known_prefix", C.c_int32)]


def formula_geometry(mb_w, mb_h, waves_env=None):
    """pick_waves of lh264_capi.hip restated: (waves, LDS bytes)"""
    inflight = min((mb_w + 1) // 2, mb_h)
    nw = 1
    while nw < inflight and nw < 8:
        nw <<= 1
    if waves_env is not None and 1 <= waves_env <= 8:
        nw = waves_env
    wg, wave, slot = (C.sizeof(_WgLds) + 15) & ~15, C.sizeof(_WaveLds), 128 * mb_w + 96
    while True:
        lds = wg + wave * nw + (nw + 1) * slot
        if lds <= 160 * 1024 or nw == 1:
            return nw, lds
        nw >>= 1


def test_recon_geometry_getter_matches_the_source_formula(monkeypatch):
    from losslessh264_amd import _lib
    monkeypatch.delenv("LH264_WAVES", raising=False)
    want = {45: 8, 120: 4, 240: 2}
    for w in (45, 120, 240):
        rc, nw, lds = _lib.recon_geometry(w, 9)
        assert (rc, nw, lds) == (0,) + formula_geometry(w, 9) and nw == want[w]
    assert _lib.recon_geometry(45, 2)[1:] == formula_geometry(45, 2) and _lib.recon_geometry(45, 2)[1] == 2
    assert _lib.recon_geometry(1, 1)[1:] == formula_geometry(1, 1) and _lib.recon_geometry(1, 1)[1] == 1
    # the widths of wave_edges: both sides of every fallback, as the source's struct sizes give them
    assert D.wave_thresholds() == {8: 116, 4: 232, 2: 406, 1: 623}
    for w, nw in D.wave_edge_widths():
        assert formula_geometry(w, 9) == _lib.recon_geometry(w, 9)[1:] and formula_geometry(w, 9)[0] == nw
    rc, nw, lds = _lib.recon_geometry(624, 2)                  # the refusal is decided before a device is looked at
    assert rc == _lib.E_UNSUPPORTED and nw == 1 and lds > 160 * 1024 and b"too wide" in _lib.lib().lh264_last_error()
    assert _lib.recon_geometry(0, 4)[0] == _lib.E_ARG
    for env in (1, 2, 3, 5, 6, 7, 8, 9, 0):                    # LH264_WAVES as the launch reads it
        monkeypatch.setenv("LH264_WAVES", str(env))
        assert _lib.recon_geometry(20, 18)[1:] == formula_geometry(20, 18, env)
        assert _lib.recon_geometry(129, 3)[1:] == formula_geometry(129, 3, env)


# ---- ranges ---------------------------------------------------------------------------------------------------------------------------
def test_ranges_hold_the_extremes():
    r = D.ranges()
    for frames in r.values():
        D.check_refs_defined(frames)
        oracle_stream(frames)
    f, = r["dc_weight"]
    assert set(f.slices["luma_dc_weight"]) == set(D.DC_WEIGHTS) and 0 in D.DC_WEIGHTS
    assert (f.mbs["mb_type"] == synth.I16).all()
    seen = {(int(f.slices["luma_dc_weight"][m["slice_id"]]), int(m["qp_y"])) for m in f.mbs}
    assert seen == {(w, q) for w in D.DC_WEIGHTS for q in D.DC_QPS}
    L = O.lib()
    for k, m in enumerate(f.mbs):                              # f * qmul stays inside int32, and reaches its last factor of 2
        wt = int(f.slices["luma_dc_weight"][m["slice_id"]])
        qmul = L.orc_luma_dc_qmul(int(m["qp_y"]), wt if wt else 16)
        peak = 16 * int(np.abs(f.coeffs[k][:256:16].astype(np.int64)).max())
        assert peak * qmul + 2 < 1 << 31
        if (k // f.mb_w) % 2 == 0:
            amp = D.dc_amp_bound(int(m["qp_y"]), wt)
            assert peak == 16 * amp and (amp == 32767 or 16 * (amp + 1) * qmul + 2 >= 1 << 31)
    assert L.orc_luma_dc_qmul(51, 255) == (255 * (14 << 8)) >> 4 and L.orc_luma_dc_qmul(7, 0 or 16) == 11 << 1
    for f in r["low_qp"]:
        assert f.mbs["qp_y"].max() <= 9
    types = set(np.concatenate([f.mbs["mb_type"] for f in r["low_qp"]]))
    assert types >= {synth.I4, synth.I16, synth.I8, synth.IPCM, synth.P16, synth.P16x8, synth.P8x16, synth.P8x8, synth.P8x8R0, synth.SKIP}
    for name, dens in (("t8_density0.5", 0.4), ("t8_density1.0", 0.95)):
        t8 = [f.coeffs[k][b * 64:b * 64 + 64] for f in r[name] for k in range(len(f.mbs)) for b in range(4)
              if f.mbs[k]["flags"] & 1 and (f.mbs[k]["cbp"] >> b) & 1]                 # the coded 8x8 blocks
        assert len(t8) >= 20 and np.abs(np.concatenate(t8).astype(np.int32)).max() >= 32700
        assert np.count_nonzero(np.concatenate(t8)) >= dens * 64 * len(t8)
    for name in ("refs16", "refs16_weighted"):
        frames = r[name]
        assert len(frames) == 19 and len(frames[16].ref_ids) == 16
        f = frames[16]
        assert sorted(f.slices["ref_slot"][0]) == list(range(16)) and list(f.slices["ref_slot"][0]) != list(range(16))
        assert set(f.mbs["ref_idx"].ravel()) == set(range(16))
        f = frames[17]
        assert f.slices["ref_slot"][0][3] == f.slices["ref_slot"][0][5] and set(f.mbs["ref_idx"].ravel()) == {3, 5}
        f = frames[18]
        lost = {k for k in range(16) if f.slices["ref_slot"][0][k] < 0}
        assert lost == {2, 7, 15} and f.slices["ref_slot"][0][0] >= 0 and lost < set(f.mbs["ref_idx"].ravel())
    wp = r["refs16_weighted"]
    denoms, lw, lo_, cw, co = set(), set(), set(), set(), set()
    for f in wp[1:]:
        sl = f.slices[0]
        assert sl["weighted_pred"] == 1
        denoms.add((int(sl["luma_log2_denom"]), int(sl["chroma_log2_denom"])))
        used = sorted(set(f.mbs["ref_idx"].ravel()))
        for tab in ("luma_weight", "luma_offset"):
            assert len(set(sl[tab])) == 16                    # distinct per ref_idx
        lw.update(sl["luma_weight"][used]); lo_.update(sl["luma_offset"][used])
        cw.update(sl["chroma_weight"][used].ravel()); co.update(sl["chroma_offset"][used].ravel())
    assert denoms == set(D.WP_DENOMS) and (7, 7) in denoms
    for s in (lw, lo_, cw, co):
        assert s >= set(D.WP_EXTREMES)


# ---- in_flight ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb_w,mb_h", [(2, 19), (3, 33)])
def test_in_flight_needs_cross_the_row_boundaries(mb_w, mb_h):
    """the last reference row a macroblock needs (inter_phase's `need`, restated) lies on the last sample row of a macroblock row for
    some macroblocks and on the first of the next for others - under a vertical fraction, without one, and where the chroma term
    decides; the odd pictures sit on the clamp with and without fractions"""
    frames = D.in_flight(mb_w, mb_h)
    D.check_refs_defined(frames)
    assert len(frames) == 6 and all(f.ref_ids == [f.id - 1] for f in frames[1:])
    _, _, hy = D.clamp_bounds(mb_w, mb_h)
    hit = set()
    for fi, f in enumerate(frames[1:], 1):
        for k in range(len(f.mbs)):
            ps = partitions(f, k)
            for (ox, oy, w, h, mvx, mvy) in ps:
                fy = clamped(f, k, ox, oy, mvx, mvy)[1]
                if fi & 1:
                    assert hy - 3 <= fy <= hy
                    hit.add(("clamp", fy & 3))
                    continue
                syy, cys = (fy >> 2) + h - 4, (fy >> 3) + ((h - 4) >> 1)         # the partition's last row of 4x4 blocks
                luma, chroma = syy + 3 + (3 if fy & 3 else 0), 2 * (cys + 1 + (1 if fy & 7 else 0)) + 1
                hit.add(("frac" if fy & 3 else "chroma" if chroma > luma else "nofrac", max(luma, chroma) % 16))
    assert {("clamp", i) for i in range(4)} <= hit
    assert {("frac", 15), ("frac", 0)} <= hit                  # syy + 6 = 16k + 15 and 16k + 16
    # without a luma fraction the luma term decides only from an even row (syy + 3 = 16k + 15); from an odd row the chroma term is
    # larger (the chroma fraction is 4): Y + 16 = 16k + 15, then 16k + 17
    assert {("nofrac", 15), ("chroma", 15), ("chroma", 1)} <= hit


# ---- the rule of include/lh264.h beside ref_slot --------------------------------------------------------------------------------------
def _damaged(data, rng):
    out = [data]
    for _ in range(3):
        out.append(data[:int(rng.integers(0, len(data) + 1))])
    for _ in range(4):
        c = bytearray(data)
        for _i in range(int(rng.integers(1, 9))):
            c[int(rng.integers(0, len(c)))] = int(rng.integers(0, 256))
        out.append(bytes(c))
    return out


def _undefined(f):
    inter = (f.mbs["mb_type"] & 0x1F8) != 0
    return bool(inter.any()) and (len(f.ref_ids) == 0 or bool((f.slices["ref_slot"][f.mbs["slice_id"][inter], 0] < 0).any()))


def test_front_end_emits_inter_macroblocks_without_a_reference_only_before_the_first_idr():
    """The rule beside ref_slot in include/lh264.h.  An inter macroblock whose slice has ref_slot[0] < 0, or whose picture has no
    reference, defines nothing: the oracle leaves the samples, the kernel reads job reference 0, the reference itself reads a null
    picture.  Over every fixture stream, whole, truncated and with corrupted bytes (the damage of tests/native/parser_stress.cpp, on the
    streams of up to 64 KB), and the concealment fixtures with the option off and on, the front end emits such a picture in exactly
    one situation: in front of a stream's first IDR picture, when the IDR was lost (BA_MW_D_IDR_LOST.264, and nothing else among the
    fixtures).  decode_batch gives those pictures a reference of 128s (tests/test_decode_batch_gpu.py); ReconSession, which has no
    such picture, refuses them before it looks for a device.  With concealment on, a lost macroblock's slice names its source in
    ref_slot[0]: a slot past the picture's references where the source is the picture of 128s."""
    import losslessh264_amd as lh
    rng = np.random.default_rng(77)
    n_frames = n_inter = 0
    offenders = set()
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "streams", "*"))) + sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "conceal", "*.264")))
    assert len(paths) >= 44
    for path in paths:
        data = open(path, "rb").read()
        for d in (_damaged(data, rng) if len(data) <= 65536 else [data]):
            seen_idr = False
            for f in lh.parse_stream(d)[0]:
                seen_idr = seen_idr or f.idr
                n_frames += 1
                n_inter += int(np.count_nonzero(f.mbs["mb_type"] & 0x1F8))
                if _undefined(f):
                    assert not seen_idr, (path, f.id)
                    offenders.add(os.path.basename(path))
                    with pytest.raises(ValueError, match="without reference 0"):
                        lh.ReconSession([[f]])
                else:
                    D.check_refs_defined([f])
        if "conceal" in path:
            for method in ("slice_copy", "mv_copy"):
                for f in lh.parse_file(data, conceal=method)[0]:
                    inter = (f.mbs["mb_type"] & 0x1F8) != 0
                    slot0 = f.slices["ref_slot"][f.mbs["slice_id"], 0]
                    assert not (inter & (slot0 < 0)).any() and not (inter & (slot0 > len(f.ref_ids))).any(), (path, method, f.id)
    assert offenders == {"BA_MW_D_IDR_LOST.264"}
    assert n_frames > 1000 and n_inter > 10000, (n_frames, n_inter)
