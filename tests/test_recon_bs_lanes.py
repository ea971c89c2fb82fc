"""The inputs of tests/recon_stages.py:bs_lane_cases decide what they claim: shown with the oracle alone (CPU) - each case names
edges of its macroblock, the lines to look at, and whether the loop filter changes the samples beside the edge there.  The device runs
of the same inputs are in tests/test_recon_bs_lanes_gpu.py."""
import numpy as np
import pytest

import oracle_lib as O
import recon_directed as D
import recon_stages as S


@pytest.fixture(scope="module")
def cases():
    return S.bs_lane_cases()


def _oracle(frames, flags=0):
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


def test_every_claim_holds_against_the_oracle(cases):
    assert len({c.name for c in cases}) == len(cases)
    n_true = n_false = 0
    for c in cases:
        D.check_refs_defined(c.frames)
        D.check_refs_defined(c.oracle_frames)
        fin = _oracle(c.oracle_frames)[-1].plane(0)
        pre = _oracle(c.oracle_frames, O.NO_DEBLOCK)[-1].plane(0)
        assert c.claims
        for edge, filtered in c.claims:
            changed = bool((S.edge_lines(fin, edge) != S.edge_lines(pre, edge)).any())
            assert changed == filtered, (c.name, edge)
            n_true, n_false = n_true + filtered, n_false + (not filtered)
    assert n_true >= 40 and n_false >= 40


def test_the_list_holds_what_it_names(cases):
    by = {c.name: c for c in cases}
    P = lambda c: c.frames[-1]
    for d in (0, 1):
        # the 8x8 transform: inner edge 2 by vectors and by a count in one 8x8 block; edges 1 and 3 with their controls
        for v in ("3,0", "4,0", "0,-3", "0,-4"):
            assert P(by["t8 edge2 dir%d vectors %s" % (d, v)]).mbs[S.C]["flags"] == 1
            assert P(by["P8x8REF0 dir%d vectors %s" % (d, v)]).mbs[S.C]["mb_type"] == S.P8x8R0
            for who in ("current", "neighbour"):
                f = P(by["SKIP %s dir%d vectors %s" % (who, d, v)])
                k = S.C if who == "current" else S._nb(d)
                assert f.mbs[k]["mb_type"] == S.SKIP and f.mbs[S.C if who == "neighbour" else S._nb(d)]["mb_type"] == S.P16
        for side in ("before", "behind"):
            f = P(by["t8 edge2 dir%d count %s" % (d, side)])
            assert f.mbs[S.C]["flags"] == 1 and np.count_nonzero(f.mbs[S.C]["nzc"]) == 1 and np.count_nonzero(f.coeffs[S.C]) == 1
        for what in ("vectors", "counts"):
            t, n = by["t8 edges 1 3 dir%d %s" % (d, what)], by["no t8 edges 1 3 dir%d %s" % (d, what)]
            ft, fn = P(t).mbs[S.C].copy(), P(n).mbs[S.C].copy()
            assert ft["flags"] == 1 and fn["flags"] == 0
            ft["flags"] = 0
            assert ft.tobytes() == fn.tobytes()                # the control differs in the flag alone ...
            assert all(not f for _, f in t.claims) and all(f for _, f in n.claims)      # ... and is filtered
        assert P(by["intra neighbour dir%d pcm" % d]).mbs[S._nb(d)]["mb_type"] == S.IPCM
        assert P(by["intra neighbour dir%d control" % d]).mbs[S._nb(d)]["mb_type"] == S.P16
        c = by["concealed neighbour dir%d" % d]
        k = S._nb(d)
        assert P(c).mbs[k]["mb_type"] == S.P16 | S.CONCEAL and c.oracle_frames[-1].mbs[k]["mb_type"] == S.P16
        assert P(c).mbs[k]["slice_id"] == 1 and P(c).slices[1]["n_mbs"] == 1 and P(c).slices[1]["deblock_idc"] == 1
        assert list(P(c).slices["deblock_idc"]) == [0, 1, 0] and list(c.oracle_frames[-1].slices["deblock_idc"]) == [2, 1, 2]
        assert by["concealed neighbour dir%d control" % d].claims[0][1] is True
        for side in ("current", "neighbour"):
            for s in range(4):
                f = P(by["count %s dir%d segment %d" % (side, d, s)])
                assert sum(np.count_nonzero(f.mbs[k]["nzc"]) for k in range(9)) == 1
        for v in (3, 4):
            f = P(by["corner dir%d %d" % (d, v)])
            assert by["corner dir%d %d" % (d, v)].claims[0][0][:2] == (0, 0) and np.count_nonzero(f.mbs[0]["nzc"]) == 7
    assert P(by["intra pcm"]).mbs[S.C]["mb_type"] == S.IPCM and P(by["intra 16x16"]).mbs[S.C]["mb_type"] == S.I16
    for name, sid_left, sid_top in (("idc2 top border", 1, 0), ("idc2 left and top border", 0, 0), ("idc2 no border", 0, 0)):
        f = P(by[name])
        assert (f.slices["deblock_idc"] == 2).all()
        assert (f.mbs[S.C - 1]["slice_id"], f.mbs[S.C - 3]["slice_id"]) == (sid_left, sid_top)
    assert P(by["idc2 top border"]).mbs[S.C]["slice_id"] == 1 and P(by["idc2 left and top border"]).mbs[S.C]["slice_id"] == 1
    assert [f for _, f in by["idc2 top border"].claims] == [True, False]
    assert [f for _, f in by["idc2 left and top border"].claims] == [False, False]
    assert [f for _, f in by["idc2 no border"].claims] == [True, True]
