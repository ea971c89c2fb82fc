"""What the directed pictures of tests/deblock_directed.py reach, shown with the oracle alone (no GPU): every picture goes through the
oracle with its filter trace on, the cells of families A-J are evaluated on the traced lines, and every cell must be reached - but
for the ones no input can reach, each named with the reason in deblock_directed (they follow from the tables and from which
strengths an edge can carry, not from a search).  test_random_streams_coverage counts, for comparison, the cells that the seeded
random streams of tests/test_recon_gpu.py and tests/test_recon_lanes_gpu.py reach."""
import numpy as np
import pytest

import deblock_directed as DD
import oracle_lib as O
import recon_directed as D
import synth

_state = {}


def _traced():
    """family -> [(scene, frames, pictures, pre-deblock pictures, trace)], once"""
    if not _state:
        for fam, scenes in DD.families().items():
            _state[fam] = []
            for s in scenes:
                fr = s.frames()
                pics, pre, rec = DD.run_oracle(fr)
                _state[fam].append((s, fr, pics, pre, rec))
    return _state


def _family_of(cell):
    return cell.split("/")[0]


def test_names_are_unique_and_pictures_small():
    seen = set()
    for fam, items in _traced().items():
        for s, fr, *_ in items:
            assert s.name not in seen, s.name
            seen.add(s.name)
            assert 1 <= len(fr) <= 3 and s.mb_w * s.mb_h <= 54
            D.check_refs_defined(fr)


def test_records_are_defined():
    """what the kernel and the oracle are defined on: inter macroblocks have their reference, IPCM macroblocks count 16 everywhere,
    every other count is the number of nonzero coefficients of its block, cbp covers every coefficient, and the P picture's
    prediction IS the reference: before the filter the picture holds exactly the samples the builder put there"""
    for fam, items in _traced().items():
        for s, fr, pics, pre, rec in items:
            f = fr[-1]
            for p, want in enumerate((s.Y, s.U, s.V)):
                assert np.array_equal(pre[-1].plane(p), want), (s.name, p)
            for k, m in enumerate(f.mbs):
                if int(m["mb_type"]) == synth.IPCM:
                    assert (m["nzc"] == 16).all() and (f.coeffs[k] >= 0).all() and (f.coeffs[k] <= 255).all()
                    continue
                assert int(m["mb_type"]) & 0x1F8, (s.name, k)
                c = f.coeffs[k]
                want = m.copy()
                D.set_nzc(want, c)
                assert (want["nzc"] == m["nzc"]).all(), (s.name, k)
                assert not c[256:].any()
                for b8 in range(4):
                    assert bool(c[64 * b8:64 * b8 + 64].any()) == bool((int(m["cbp"]) >> b8) & 1), (s.name, k, b8)
                if int(m["mb_type"]) == synth.SKIP:
                    assert not c.any() and not m["mv"].any()


def test_evaluator_reproduces_the_trace():
    """the decisions the cells are evaluated with, recomputed from the `before` samples of every record, give its `after` samples"""
    n = 0
    for fam, items in _traced().items():
        for s, fr, pics, pre, rec in items:
            m = DD.model_of(rec)
            bad = np.nonzero((m["out"] != rec["after"]).any(1))[0]
            assert len(bad) == 0, (s.name, rec[bad[0]], m["out"][bad[0]])
            want_tc = DD.tc_of(rec["idx_tc"].astype(int), rec["bs"], rec["plane"] == 0)
            assert np.array_equal(want_tc, rec["tc"]), s.name
            assert np.array_equal(DD.ALPHA[DD.tab(rec["idx_a"].astype(int))], rec["alpha"]) and np.array_equal(DD.BETA[DD.tab(rec["idx_b"].astype(int))], rec["beta"])
            n += len(rec)
    assert n > 50000


def test_trace_is_off_by_default_and_changes_nothing():
    s = DD.families()["I"][0]
    fr = s.frames()
    plain, _, _ = DD.run_oracle(fr, trace=False)
    traced, _, rec = DD.run_oracle(fr, trace=True)
    assert len(rec) > 0 and O.lib().orc_deblock_trace_count() == 0
    for a, b in zip(plain, traced):
        assert np.array_equal(a.buf, b.buf)
    # nothing was filtered before the first record: its `before` is the unfiltered picture's line
    _, pre, _ = DD.run_oracle(fr, trace=False)
    r = rec[0]
    line = [pre[-1].plane(int(r["plane"]))[DD._positions(r, j)[::-1]] for j in range(8)]
    assert list(r["before"]) == line


def test_trace_overflow_is_reported_and_stays_inside_the_buffer():
    s = DD.families()["I"][0]
    fr = s.frames()
    refs = [O.HostPic(fr[0].mb_w, fr[0].mb_h)]
    O.recon_frame(fr[0].mbs, fr[0].coeffs, fr[0].slices, refs[0], [], 0)
    f = fr[1]
    full = O.recon_frame_traced(f.mbs, f.coeffs, f.slices, O.HostPic(f.mb_w, f.mb_h), refs, 0)
    for cap in (1, 15, 16, 17, len(full) - 1):
        with pytest.raises(O.TraceOverflow):          # (recon_frame_traced also asserts that the guard record behind `cap` is untouched)
            O.recon_frame_traced(f.mbs, f.coeffs, f.slices, O.HostPic(f.mb_w, f.mb_h), refs, 0, cap=cap)
    again = O.recon_frame_traced(f.mbs, f.coeffs, f.slices, O.HostPic(f.mb_w, f.mb_h), refs, 0, cap=len(full))
    assert again.tobytes() == full.tobytes()


def _coverage(items):
    hit = {}
    for s, fr, pics, pre, rec in items:
        for n, c in DD.cells(s, fr[-1], rec, pre[-1]).items():
            hit[n] = hit.get(n, 0) + c
    return hit


def test_every_cell_is_reached(capsys):
    """the cap on cells left out is zero; DD.all_cell_names() names the unreachable ones, and none of those may be reached either (a
    claim that a cell cannot be reached, refuted by a picture, is a mistake in the claim)"""
    names, unreach = DD.all_cell_names()
    assert len(set(names)) == len(names) and set(unreach) <= set(names)
    hit = {}
    for fam, items in _traced().items():
        for n, c in _coverage(items).items():
            hit[n] = hit.get(n, 0) + c
    assert set(hit) <= set(names), sorted(set(hit) - set(names))[:5]
    missing = [n for n in names if n not in unreach and not hit.get(n)]
    refuted = [n for n in unreach if hit.get(n)]
    per = {}
    for n in names:
        fam = _family_of(n)
        per.setdefault(fam, [0, 0])
        per[fam][0 if n not in unreach else 1] += 1
    with capsys.disabled():
        print("\ncells reached / named unreachable per family: " + ", ".join("%s %d / %d" % (k, v[0], v[1]) for k, v in sorted(per.items())))
    assert not missing, "%d cells not reached, first: %s" % (len(missing), missing[:10])
    assert not refuted, refuted[:10]


def test_unreachable_tc_pins_follow_from_the_tables():
    """the bound behind the E/../tc/.. cells named unreachable, by exhaustion: over every line of differences that passes the three
    gates at alpha and beta, the largest |(4 (q0 - p0) + (p1 - q1) + 4) >> 3| is max_raw(alpha, beta) - at the index's own beta and at
    the largest one the slice offsets allow (indexB = indexA + 24), which is the one a cell must miss to be named unreachable"""
    for idx in DD.IDX:
        for spread in (0, DD.MAX_SPREAD):
            a, b = int(DD.ALPHA[idx]), int(DD.BETA[min(idx + spread, 51)])
            d = np.arange(-(a - 1), a)[:, None, None]
            e1 = np.arange(-(b - 1), b)[None, :, None]
            e2 = np.arange(-(b - 1), b)[None, None, :]
            raw = (4 * d + (e1 - d - e2) + 4) >> 3                # p1 - q1 = (p1 - p0) - (q0 - p0) - (q1 - q0)
            assert np.abs(raw).max() == DD.max_raw(a, b), (idx, spread)
    assert DD.BETA[51] == DD.BETA.max() and (np.diff(DD.BETA) >= 0).all()      # a larger indexB never gives a smaller beta
    for idx in DD.IDX:
        for bs in (1, 2, 3):
            for luma in (True, False):
                t_min = int(DD.TC0[idx][bs - 1]) + (0 if luma else 1)
                bound = DD.max_raw(int(DD.ALPHA[idx]), int(DD.BETA[min(idx + DD.MAX_SPREAD, 51)]))
                assert DD.tc_pin_reachable(idx, bs, luma) == (bound >= t_min + 1)


def _random_streams():
    """the seeded random streams of tests/test_recon_gpu.py and tests/test_recon_lanes_gpu.py, built by their own code"""
    import test_recon_gpu as G
    import test_recon_lanes_gpu as LG
    for case in G.CASES:
        yield synth.make_stream(**case)
    for seed in LG.SUB_PARTITION_SEEDS:
        yield LG.sub_partition_stream(seed)
    for seed in LG.SUB_PARTITION_WEIGHTED_SEEDS:
        yield LG.sub_partition_weighted_stream(seed)
    for seed in LG.WEIGHTED_SEEDS:
        yield LG.weighted_stream(seed)
    for seed, offsets in LG.CHROMA_QP_CASES:
        yield LG.chroma_qp_stream(seed, offsets)


def test_random_streams_coverage(capsys):
    """counted, not demanded: the single-line cells (families A-E and their share of the tables) that the seeded random streams of
    the existing GPU tests reach, traced the same way.  The number is the measure of the gap the directed pictures close."""
    names, unreach = DD.line_cell_names()
    hit = set()
    for frames in _random_streams():
        pics = {}
        for f in frames:
            dst = O.HostPic(f.mb_w, f.mb_h)
            rec = O.recon_frame_traced(f.mbs, f.coeffs, f.slices, dst, [pics[r] for r in f.ref_ids], 0)
            pics[f.id] = dst
            hit |= {n for n, v in DD.line_cells(rec).items() if v.any()}
    _, unreach = DD.all_cell_names()
    want = [n for n in names if n not in unreach]
    got = [n for n in want if n in hit]
    per = {}
    for n in want:
        per.setdefault(_family_of(n), [0, 0])
        per[_family_of(n)][1] += 1
        per[_family_of(n)][0] += n in hit
    with capsys.disabled():
        print("\nrandom streams reach %d of the %d reachable single-line cells of families A-E: %s"
              % (len(got), len(want), ", ".join("%s %d / %d" % (k, v[0], v[1]) for k, v in sorted(per.items()))))
