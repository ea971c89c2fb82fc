"""Inputs for the glue of the reconstruct kernel's macroblock loop (no GPU here): the moves between the tile, the carry, the row
buffers and the picture, whose predicates depend on the macroblock's place only (a left neighbour, a row above, the last column, the
last row) - so the smallest pictures in which one macroblock sees every combination of them - and the QP patterns that decide whether
the in-loop filter looks its thresholds up once or three times.  tests/test_recon_glue.py shows with the oracle alone that the inputs
reach what they claim, tests/test_recon_glue_gpu.py runs them through the kernel."""
import numpy as np

import recon_directed as D
import synth

# (mb_w, mb_h): 1x1 has no neighbour and is last in both directions; 2x1 / 1x2 add one neighbour; 1x9 gives every one of 8 waves a
# row and the ninth row to the first wave again; 12x1 is one row, longer than the bench picture's; 3x3 has a macroblock of every kind;
# 11x9 is the bench picture
SHAPES = [(1, 1), (2, 1), (1, 2), (1, 9), (12, 1), (3, 3), (11, 9)]
SLICED = [(3, 3), (11, 9)]
QP = 30
TARGET = 4          # the macroblock (1, 1) of a 3x2 picture: left neighbour 3, top neighbour 1


def chain(mb_w, mb_h, **kw):
    """intra, then two P pictures"""
    return synth.make_stream(seed=700 + 16 * mb_w + mb_h, mb_w=mb_w, mb_h=mb_h, n_frames=3, **kw)


def intra_chain(mb_w, mb_h):
    """three intra pictures: nothing reads a reference, so the padding need not be defined"""
    return synth.make_stream(seed=800 + 16 * mb_w + mb_h, mb_w=mb_w, mb_h=mb_h, n_frames=3, p_frames=False)


def _inter_picture(fid, mb_w, mb_h, rng, idc=0, qp=QP):
    f = D.new_frame(fid, mb_w, mb_h, [fid - 1], idc=idc, qp=qp)
    for k in range(mb_w * mb_h):
        D.random_inter(f.mbs[k], f.coeffs[k], rng, span=12, density=0.3)
    return f


def uncovered(k, mb_w=3, mb_h=3):
    """intra picture, a P picture whose macroblock k no slice covers (record and coefficients zero: what the front end leaves), and a
    P picture that reads it.  QP 45: the edges towards the zero record (QP 0) take the mean, 23, which still filters"""
    rng = np.random.default_rng(900 + k)
    n = mb_w * mb_h
    frames = synth.make_stream(seed=900 + k, mb_w=mb_w, mb_h=mb_h, n_frames=1)
    f = _inter_picture(1, mb_w, mb_h, rng, qp=45)
    runs = [(a, b) for a, b in ((0, k), (k + 1, n)) if b > a]
    f.slices = np.repeat(f.slices[:1], len(runs))
    for s, (a, b) in enumerate(runs):
        f.slices[s]["first_mb"], f.slices[s]["n_mbs"] = a, b - a
        f.mbs["slice_id"][a:b] = s
    f.mbs[k] = np.zeros((), dtype=f.mbs.dtype)
    f.coeffs[k] = 0
    f.covered[k] = 0
    frames.append(f)
    frames.append(_inter_picture(2, mb_w, mb_h, rng))
    return frames


def uncovered_places():
    return {"corner": 0, "edge": 1, "middle": 4}


def qp_pattern(name):
    """a PCM picture and a 3x2 P picture whose macroblocks all have QP 30 but for what `name` says about the neighbours of TARGET;
    intra_cb_cr: one intra picture whose Cb and Cr QPs differ in every macroblock"""
    rng = np.random.default_rng(1000 + QP_PATTERNS.index(name))
    if name == "intra_cb_cr":
        f = synth.make_stream(seed=1001, mb_w=3, mb_h=2, n_frames=1)[0]
        f.slices["alpha_c0_offset"], f.slices["beta_offset"] = 0, 0
        f.mbs["qp_y"] = QP
        f.mbs["qp_c"] = (QP - 4, QP + 5)
        return [f]
    frames = [D.pcm_content(rng, 3, 2, "smooth", 0)]
    f = _inter_picture(1, 3, 2, rng)
    left, top = f.mbs[TARGET - 1], f.mbs[TARGET - 3]
    if name in ("left", "both"):
        left["qp_y"], left["qp_c"] = QP - 10, QP - 10
    if name in ("top", "both"):
        top["qp_y"], top["qp_c"] = QP + 10, QP + 10
    if name == "chroma":
        left["qp_c"] = (QP, QP + 8)
    frames.append(f)
    return frames


QP_PATTERNS = ("one", "left", "top", "both", "chroma", "intra_cb_cr")
