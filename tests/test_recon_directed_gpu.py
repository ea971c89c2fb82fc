"""The directed inputs of tests/recon_directed.py through recon_chain_kernel (ReconSession), every padded plane of every picture
against the oracle, bit for bit: motion compensation at the ends of its arithmetic and at the clamp, the 64-macroblock row masks,
every wave count and both sides of every LDS fallback, the refusal of a picture too wide, ranges the random generator never draws,
the boundary-strength thresholds, and references still in flight.  tests/test_recon_directed.py shows (CPU) that the inputs reach
what they claim."""
import numpy as np
import pytest

import oracle_lib as O
import recon_directed as D
import synth

pytestmark = pytest.mark.gpu

_oracle_cache = {}


def _oracle(key, frames):
    """the chain through the oracle, once per input (the pictures are compared, never written)"""
    if key not in _oracle_cache:
        pics, out = {}, []
        for f in frames:
            dst = O.HostPic(f.mb_w, f.mb_h)
            O.recon_frame(f.mbs, f.coeffs, f.slices, dst, [pics[r] for r in f.ref_ids], 0)
            pics[f.id] = dst
            out.append(dst)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def _describe(f, k):
    m = f.mbs[k]
    s = "mb %d (%d,%d) type %#x flags %d qp %d" % (k, k % f.mb_w, k // f.mb_w, m["mb_type"], m["flags"], m["qp_y"])
    if int(m["mb_type"]) & 0x1F8:
        s += " sub %s ref_idx %s mv %s" % (list(m["sub_type"]), list(m["ref_idx"]), sorted(set(map(tuple, m["mv"].tolist()))))
    else:
        s += " modes %s chroma %d" % (list(m["intra_mode"]), m["chroma_mode"])
    return s


def _check(sess, chain, frames, want, label):
    """first differing sample with its macroblock, type and parameters"""
    for i, f in enumerate(frames):
        got = sess.picture(chain, i, padded=True)
        for p in range(3):
            ref = want[i].padded_plane(p)
            if not np.array_equal(got[p], ref):
                ys, xs = np.nonzero(got[p] != ref)
                bs, pad = (8, 16) if p else (16, 32)
                x, y = int(xs[0]) - pad, int(ys[0]) - pad
                kx, ky = min(max(x // bs, 0), f.mb_w - 1), min(max(y // bs, 0), f.mb_h - 1)
                raise AssertionError("%s: chain %d picture %d plane %d: %d samples differ, first at (%d,%d) got %d want %d; %s"
                                     % (label, chain, i, p, len(ys), x, y, got[p][ys[0], xs[0]], ref[ys[0], xs[0]], _describe(f, ky * f.mb_w + kx)))


def _run(named, replicate=1):
    """named: [(label, frames)] -> one session, one chain each (x replicate), all compared"""
    import losslessh264_amd as lh
    for _, frames in named:
        D.check_refs_defined(frames)
    sess = lh.ReconSession([fr for _, fr in named], replicate=replicate)
    sess.run(); sess.synchronize()
    for c in range(sess.n_chains):
        label, frames = named[c % len(named)]
        _check(sess, c, frames, _oracle(label, frames), label)


@pytest.fixture(autouse=True)
def _no_wave_override(monkeypatch):
    monkeypatch.delenv("LH264_WAVES", raising=False)


# ---- motion compensation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content,mixed", [("tap_extreme", False), ("binary", False), ("uniform", False), ("tap_extreme", True), ("uniform", True)])
def test_mc_grid(content, mixed):
    """all seven partition shapes (a chain each): every fraction, sign and fetch alignment, on content that drives the 6-tap sums to
    +10,710 / -2,550 and both clips of the centre position; mixed: different fractions in the strips of one wave"""
    _run([("mc_grid %s %s%s" % (shape, content, " mixed" if mixed else ""), D.mc_grid(shape, content, mixed)) for shape in D.SHAPES])


@pytest.mark.parametrize("mb_w,mb_h", [(1, 1), (2, 2), (3, 2)])
def test_mc_border(mb_w, mb_h):
    """vectors on, just inside and just beyond each bound of the clamp, in x, in y and at the corners, 16x16 and 4x4"""
    _run([("mc_border %dx%d" % (mb_w, mb_h), D.mc_border(mb_w, mb_h)[0])])


# ---- the 64-macroblock row masks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb_w", D.MASK_WIDTHS)
def test_row_masks(mb_w):
    """isolated intra macroblocks (and, in the complement, isolated inter ones) at columns 0, 1, 61..66, 125..130 and the last two of
    rows 1 and 2: the special cases of pub_line / pub_left at the ends of a 64-bit mask word and its reload every 64 macroblocks"""
    _run([("row_masks %d" % mb_w, D.row_masks(mb_w)), ("row_masks %d complement" % mb_w, D.row_masks(mb_w, complement=True))])


# ---- wave counts ----------------------------------------------------------------------------------------------------------------------
def _edge_cases():
    try:
        return D.wave_edge_widths()
    except Exception:                      # library not built: collection must not fail, the test will
        return [(0, 0)]


@pytest.mark.parametrize("width,waves", _edge_cases())
def test_wave_edges(width, waves):
    """both sides of every fallback of pick_waves, the last width one wave carries, and a 4K picture: 9 rows, so 8 waves are wanted.
    The wave count a launch ran with cannot be read back; the getter that shares pick_waves with the launch says what it chooses (and
    tests/test_recon_directed.py holds it against the source's formula), the picture shows that the launch was right."""
    from losslessh264_amd import _lib
    rc, nw, lds = _lib.recon_geometry(width, 9)
    assert rc == 0 and nw == waves and lds <= 160 * 1024
    assert _lib.recon_geometry(width + 1, 9)[1] <= nw
    _run([("wave_edges %d" % width, D.wave_edges(width))])


def _wave_count_inputs():
    return [[("synth seed 9", synth.make_stream(seed=9, mb_w=20, mb_h=18, n_frames=3, n_slices=4, idc=2, t8=True)),
             ("in_flight 2x19", D.in_flight(2, 19)), ("in_flight 3x33", D.in_flight(3, 33))],
            [("row_masks 65", D.row_masks(65))], [("row_masks 129", D.row_masks(129))]]


@pytest.mark.parametrize("waves", [1, 2, 3, 5, 8])
def test_wave_counts(waves, monkeypatch):
    """LH264_WAVES (read at every launch): 1, 2 and 8 waves and the counts that are no power of two (NW + 1 line slots with odd NW)"""
    from losslessh264_amd import _lib
    monkeypatch.setenv("LH264_WAVES", str(waves))
    assert _lib.recon_geometry(20, 18)[1] == waves and _lib.recon_geometry(65, 3)[1] == waves
    assert _lib.recon_geometry(129, 3)[1] == (waves if waves < 8 else 4)       # 8 waves do not fit 129 macroblocks
    for named in _wave_count_inputs():
        _run(named, replicate=2)


def test_too_wide_is_refused_and_launches_nothing():
    """the first width beyond one wave: LH264_E_UNSUPPORTED with its text, before anything is launched (the pictures keep their
    fill); the next call succeeds.  An argument check, not a fault."""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib
    width = D.wave_thresholds()[1] + 1
    frames = synth.make_stream(seed=61, mb_w=width, mb_h=2, n_frames=1, p_frames=False)
    sess = lh.ReconSession([frames])
    rc = sess.lib.lh264_recon_chains(sess.d_jobs.data_ptr(), sess.d_chain_first.data_ptr(), sess.n_chains, sess.max_w, sess.max_h, sess._stream())
    assert rc == _lib.E_UNSUPPORTED and b"too wide" in sess.lib.lh264_last_error()
    with pytest.raises(RuntimeError, match="too wide"):
        sess.run()
    sess.synchronize()
    assert bool((sess.d_pics == 128).all())
    small = synth.make_stream(seed=62, mb_w=5, mb_h=4, n_frames=2)
    _run([("after the refusal", small)])
    sess2 = lh.ReconSession([synth.make_stream(seed=61, mb_w=width - 1, mb_h=2, n_frames=1, p_frames=False)])
    sess2.run(); sess2.synchronize()
    f = sess2.streams[0]
    _check(sess2, 0, f, _oracle("last width", f), "last width of one wave, 2 rows")


# ---- ranges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dc_weight", "low_qp", "t8_density0.5", "t8_density1.0", "refs16", "refs16_weighted"])
def test_ranges(name):
    """scaling-list weights of the luma DC with amplitudes up to the int32 bound, QP 0..9, saturating 8x8 transforms, 16 references
    with a permuted list, two indices for one picture, ref_slot -1 behind a valid entry 0, weights / offsets / denominators at the ends
    of their syntax"""
    _run([("ranges " + name, D.ranges()[name])])


# ---- boundary strengths ---------------------------------------------------------------------------------------------------------------
def test_bs_thresholds():
    """every pair of tests/recon_directed.py:bs_thresholds, a chain each"""
    _run([("bs " + c.name, c.frames) for c in D.bs_thresholds()])


# ---- references in flight -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb_w,mb_h", [(2, 19), (3, 33)])
def test_in_flight(mb_w, mb_h):
    """Tall chains whose every macroblock reads the previous picture - the one the workgroup may still be writing - as far down as
    the clamp allows, or exactly where the last row it needs crosses a macroblock-row boundary.  An under-estimated wait shows only
    if the other wave happens to be late: this test can catch it by chance only (8 replicas, more than 1,000 macroblocks each).  It
    is here because nothing else aims at that line of inter_phase."""
    _run([("in_flight %dx%d" % (mb_w, mb_h), D.in_flight(mb_w, mb_h))], replicate=8)
