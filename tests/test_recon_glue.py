"""The inputs of tests/recon_glue_cases.py reach what they claim: shown with the oracle alone (CPU).  The device runs of the same inputs
are in tests/test_recon_glue_gpu.py."""
import numpy as np
import pytest

import oracle_lib as O
import recon_glue_cases as G
import recon_directed as D


def _traced_last(frames):
    """the chain through the oracle -> (pictures, the filter trace of the last picture)"""
    pics, out, trace = {}, [], None
    for i, f in enumerate(frames):
        dst = O.HostPic(f.mb_w, f.mb_h)
        refs = [pics[r] for r in f.ref_ids]
        if i == len(frames) - 1:
            trace = O.recon_frame_traced(f.mbs, f.coeffs, f.slices, dst, refs, 0)
        else:
            O.recon_frame(f.mbs, f.coeffs, f.slices, dst, refs, 0)
        pics[f.id] = dst
        out.append(dst)
    return out, trace


def _sets(trace, mb, plane):
    """the distinct (alpha, beta) pairs the lines of macroblock mb's edges in one plane were filtered with, per (dir, edge)"""
    t = trace[(trace["mb"] == mb) & (trace["plane"] == plane)]
    return {(int(d), int(e)): {(int(a), int(b)) for a, b in zip(t["alpha"][(t["dir"] == d) & (t["edge"] == e)], t["beta"][(t["dir"] == d) & (t["edge"] == e)])}
            for d, e in {(int(d), int(e)) for d, e in zip(t["dir"], t["edge"])}}


def _distinct(sets):
    return set().union(*sets.values()) if sets else set()


@pytest.mark.parametrize("name,luma,chroma_v", [("one", 1, 1), ("left", 2, 2), ("top", 2, 2), ("both", 3, 3), ("chroma", 1, 2)])
def test_qp_patterns_give_one_two_or_three_threshold_sets(name, luma, chroma_v):
    """the target macroblock's left edge, top edge and inner edges are all filtered, with as many different (alpha, beta) as the case
    is named for: in luma, and in Cr where only a chroma QP differs"""
    frames = G.qp_pattern(name)
    D.check_refs_defined(frames)
    _, trace = _traced_last(frames)
    y, v = _sets(trace, G.TARGET, 0), _sets(trace, G.TARGET, 2)
    for s in (y, v):
        assert (0, 0) in s and (1, 0) in s and any(e > 0 for _, e in s), "left, top and inner edges must all be filtered: %s" % sorted(s)
        assert all(len(x) == 1 for x in s.values())
    assert len(_distinct(y)) == luma and len(_distinct(v)) == chroma_v
    inner = _distinct({k: x for k, x in y.items() if k[1] > 0})
    assert len(inner) == 1
    if name in ("left", "both"):
        assert y[(0, 0)] != inner
    if name in ("top", "both"):
        assert y[(1, 0)] != inner
    if name == "left":
        assert y[(1, 0)] == inner
    if name == "top":
        assert y[(0, 0)] == inner
    if name == "one":                       # and nowhere else in the picture either: the whole picture takes the single lookup
        assert len({(int(a), int(b)) for a, b in zip(trace["alpha"][trace["plane"] == 0], trace["beta"][trace["plane"] == 0])}) == 1


def test_intra_macroblocks_with_two_chroma_qps_are_filtered_in_both_planes():
    frames = G.qp_pattern("intra_cb_cr")
    f = frames[0]
    assert (f.mbs["mb_type"] & 0x207 != 0).all() and (f.mbs["qp_c"][:, 0] != f.mbs["qp_c"][:, 1]).all()
    _, trace = _traced_last(frames)
    u, v = _sets(trace, G.TARGET, 1), _sets(trace, G.TARGET, 2)
    # the inner horizontal chroma edge (dir 1, edge 2) of both planes is filtered, with thresholds of two different QPs
    assert (1, 2) in u and (1, 2) in v and _distinct(u) != _distinct(v)


@pytest.mark.parametrize("place", list(G.uncovered_places()))
def test_uncovered_macroblocks_are_uncovered(place):
    k = G.uncovered_places()[place]
    frames = G.uncovered(k)
    D.check_refs_defined(frames)
    f = frames[1]
    assert int(f.mbs[k]["mb_type"]) == 0 and not f.mbs[k].tobytes().strip(b"\0") and not f.coeffs[k].any()
    in_slice = np.zeros(len(f.mbs), dtype=bool)
    for s in f.slices:
        in_slice[s["first_mb"]:s["first_mb"] + s["n_mbs"]] = True
    assert not in_slice[k] and in_slice.sum() == len(f.mbs) - 1
    assert (f.mbs["mb_type"][in_slice] != 0).all()
    pics, trace = _traced_last(frames[:2])
    x, y = k % f.mb_w, k // f.mb_w
    # nothing reconstructs it: beyond the reach of its neighbours' filters (3 samples) it keeps the picture's fill
    assert (pics[1].plane(0)[16 * y + 3:16 * y + 13, 16 * x + 3:16 * x + 13] == 128).all()
    assert not (trace["mb"] == k).any()
    # and its right / lower neighbour filters the edge towards it
    for nb, d in ((k + 1, 0), (k + f.mb_w, 1)):
        if (d == 0 and x + 1 < f.mb_w) or (d == 1 and y + 1 < f.mb_h):
            assert ((trace["mb"] == nb) & (trace["dir"] == d) & (trace["edge"] == 0)).any(), (nb, d)


def test_shapes_hold_every_combination_of_the_four_flags():
    seen = set()
    for w, h in G.SHAPES:
        for y in range(h):
            for x in range(w):
                seen.add((x > 0, y > 0, x == w - 1, y == h - 1))
    assert len(seen) == 16
    assert any(h > 8 for _, h in G.SHAPES)          # a row whose wave has already served a row of the same picture
