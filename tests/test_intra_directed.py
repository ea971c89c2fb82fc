"""What the directed intra pictures of tests/intra_directed.py reach, shown without a GPU: every coverage cell is reached, every
record is valid, on every case without residual and filter the oracle's reconstruction IS the prediction of the independent model
(tests/intra_model.py) in all three planes, and every deliberately wrong variant of the model differs from the true one on the cells
it belongs to - so a kernel that computed the variant would fail tests/test_intra_directed_gpu.py."""
import numpy as np
import pytest

import intra_directed as ID
import intra_model as M
import recon_directed as D
from synth import I4, I8, I16, IPCM


def _all_cases():
    return [c for cases in ID.families().values() for c in cases]


def test_names_are_unique_and_pictures_small():
    seen = set()
    for c in _all_cases():
        assert c.name not in seen, c.name
        seen.add(c.name)
        assert c.mb_w <= 8 and c.mb_h <= 6 and len(c.frames()) == 1
        assert len(c.sites) > 0


def test_every_cell_is_reached(capsys):
    """no allowance for missing cells; a cell no name stands for is a mistake of the evaluator"""
    names = ID.all_cell_names()
    hit = {}
    for c in _all_cases():
        for n, k in ID.cells(c).items():
            hit[n] = hit.get(n, 0) + k
    assert set(hit) <= set(names), sorted(set(hit) - set(names))[:5]
    missing = [n for n in names if not hit.get(n)]
    per = {}
    for n in names:
        per[n.split("/")[0]] = per.get(n.split("/")[0], 0) + 1
    with capsys.disabled():
        print("\ncells per group: " + ", ".join("%s %d" % kv for kv in sorted(per.items())))
        print("macroblocks under a strong filter whose neighbours it changed: " + ", ".join("%s %d" % (n[5:], hit[n]) for n in names if n.startswith("filt/") and n in hit))
    assert not missing, "%d cells not reached, first: %s" % (len(missing), missing[:10])


def test_records_are_valid():
    """the modes respect availability (for I4x4, I16x16 and chroma the availability the builder states, which no more than what the
    picture offers; for I8x8 the record's own flags); every other macroblock is I_PCM, every neighbour of a macroblock under test
    too; counts and cbp are those of the coefficients"""
    for c in _all_cases():
        f = c.f
        D.check_refs_defined(c.frames())
        assert int(f.slices["n_mbs"].sum()) == c.mb_w * c.mb_h and len(set(c.sites)) == len(c.sites)
        under_test = {(x, y) for (x, y, _, _) in c.sites}
        for k, m in enumerate(f.mbs):
            if (k % c.mb_w, k // c.mb_w) not in under_test:
                assert int(m["mb_type"]) == IPCM and (m["nzc"] == 16).all(), (c.name, k)
        for (x, y, avail, place) in c.sites:
            k = y * c.mb_w + x
            m = f.mbs[k]
            typ, mode = int(m["mb_type"]), [int(v) for v in m["intra_mode"]]
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    assert (dx, dy) == (0, 0) or (x + dx, y + dy) not in under_test, (c.name, x, y)
            phys = ID.physical_avail(f, k)
            assert avail & ~phys == 0, (c.name, x, y, avail, phys)
            if c.family == "pos" or getattr(c, "source_family", "") == "pos":
                assert avail == phys
            if typ == I4:
                lists = ID.i4_valid(avail)
                assert all(mode[b] in lists[b] for b in range(16)), (c.name, x, y, mode)
            elif typ == I8:
                assert int(m["flags"]) & 1 and int(m["intra_avail"]) == avail
                lists = ID.i8_valid(int(m["intra_avail"]))
                assert all(mode[((i >> 1) << 3) + ((i & 1) << 1)] in lists[i] for i in range(4)), (c.name, x, y, mode)
            else:
                assert typ == I16 and mode[0] in ID.i16_valid(avail), (c.name, x, y, mode)
            assert int(m["chroma_mode"]) in ID.chroma_valid(avail), (c.name, x, y)
            want = m.copy()
            D.set_nzc(want, f.coeffs[k])
            assert (want["nzc"] == m["nzc"]).all()
            co = f.coeffs[k]
            if not c.residual:
                assert not co.any() and int(m["cbp"]) == 0
            else:
                assert all(co[64 * b8:64 * b8 + 64].any() for b8 in range(4)) and int(m["cbp"]) == 0x2F and co[257:].any()


def test_unavailable_neighbours_hold_real_samples():
    """position family: no sample of the picture is 128 (what DC_128 or a missing picture would give), and where the block above and
    to the right of a *_TOP block exists, its bottom row is not the replicated sample"""
    n_top = 0
    for c in ID.families()["pos"]:
        assert all((p != 128).all() for p in c.planes), c.name
        for (x, y, avail, place) in c.sites:
            m = c.record(x, y)
            if int(m["mb_type"]) == I4 and y > 0:
                for bx in range(4):
                    if int(m["intra_mode"][bx]) in ID.TOP_MODES and 16 * x + 4 * bx + 8 <= 16 * c.mb_w:
                        row = c.planes[0][16 * y - 1]
                        assert (row[16 * x + 4 * bx + 4:16 * x + 4 * bx + 8] != row[16 * x + 4 * bx + 3]).any(), (c.name, x, y, bx)
                        n_top += 1
    assert n_top > 0


def test_oracle_equals_model_without_residual():
    """every zero-residual deblock_idc 1 case, all three planes, whole pictures (so every macroblock under test, and every I_PCM one)"""
    n = 0
    for c in _all_cases():
        if not c.zero_residual_unfiltered:
            continue
        want, got = c.model(), c.oracle(0)
        for p in range(3):
            if not np.array_equal(got.plane(p), want[p]):
                ys, xs = np.nonzero(got.plane(p) != want[p])
                bs = 8 if p else 16
                k = int(ys[0]) // bs * c.mb_w + int(xs[0]) // bs
                raise AssertionError("%s plane %d: %d samples differ, first at (%d,%d) oracle %d model %d; mb %d type %#x modes %s chroma %d avail %d"
                                     % (c.name, p, len(ys), xs[0], ys[0], got.plane(p)[ys[0], xs[0]], want[p][ys[0], xs[0]], k, c.f.mbs[k]["mb_type"],
                                        list(c.f.mbs[k]["intra_mode"]), c.f.mbs[k]["chroma_mode"], c.f.mbs[k]["intra_avail"]))
        n += len(c.sites)
    assert n == sum(len(c.sites) for fam in ("i4", "i8", "i16c", "pos") for c in ID.families()[fam]) and n > 900


def test_oracle_equals_model_with_residual():
    """beyond what is demanded: the model's block-by-block reconstruction with the residual the oracle's transforms give"""
    for c in ID.families()["res"]:
        want, got = c.model(), c.oracle(0)
        for p in range(3):
            assert np.array_equal(got.plane(p), want[p]), (c.name, p)


@pytest.mark.parametrize("variant", sorted(M.VARIANTS))
def test_variant_is_told_apart(variant, capsys):
    """the wrong variant changes at least one sample of a macroblock under test in EACH part it belongs to (a family's luma or its
    chroma): a variant that spans block sizes or planes is told apart in every one of them"""
    assert sorted(ID.VARIANT_PARTS) == sorted(M.VARIANTS)
    report = []
    for fam, part in ID.VARIANT_PARTS[variant]:
        n_mb = n_samples = 0
        for c in ID.families()[fam]:
            true, wrong = c.model(), c.model(variant)
            for (x, y, _, _) in c.sites:
                d = sum(int(np.count_nonzero(true[p][bs * y:bs * y + bs, bs * x:bs * x + bs] != wrong[p][bs * y:bs * y + bs, bs * x:bs * x + bs]))
                        for p, bs in (((0, 16),) if part == "luma" else ((1, 8), (2, 8))))
                n_mb += d > 0
                n_samples += d
        report.append("%s %s: %d macroblocks, %d samples" % (fam, part, n_mb, n_samples))
        assert n_mb > 0, (variant, fam, part)
    with capsys.disabled():
        print("\nvariant %s (%s) differs in " % (variant, M.VARIANTS[variant]) + "; ".join(report))


def test_steep_ramps_reach_the_largest_sums():
    """|H| = |V| = 9180 = 255 * 36 in luma, 2550 in chroma"""
    best = {16: 0, 8: 0}
    for c in ID.families()["i16c"]:
        if c.name.startswith("i16c steep++") or c.name.startswith("i16c steep--"):
            for (x, y, _, _) in c.sites:
                for plane, n in ((c.planes[0], 16), (c.planes[1], 8)):
                    hh, vv = M.plane_terms(plane, n * x, n * y, n)[:2]
                    assert abs(hh) == abs(vv)
                    best[n] = max(best[n], abs(hh))
    assert best == {16: 9180, 8: 2550}
