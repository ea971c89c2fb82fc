"""The directed inputs of tests/ctx_directed.py reach what they claim: shown with the oracle alone (CPU).  These are conditions on the
inputs, not measurements of the kernels; the device runs of the same inputs are in tests/test_ctx_directed_gpu.py."""
import itertools

import numpy as np
import pytest

import ctx_directed as D
import oracle_lib as O


def mbs_of(name):
    """(frame, k, oracle's list) of every macroblock of a family"""
    b = D.batch(name)
    for (c, i, f), e in zip(b.jobs(), D.expect(b)):
        for k in range(f.mb_w * f.mb_h):
            yield f, k, e.syms[k]


def targets_of(name):
    """what -> (frame, k, oracle's list) of the macroblocks a family of single cases is about"""
    b = D.batch(name)
    at = {(c, i): j for j, (c, i, _) in enumerate(b.jobs())}
    exps = D.expect(b)
    out = {}
    for c, i, k, what in b.targets:
        assert what not in out, what
        out[what] = (b.chains[c][i], k, exps[at[(c, i)]].syms[k])
    return out


# ---- the tables and the rules restated here ---------------------------------------------------------------------------------------------
def test_scan_tables():
    assert D.ZZ16 == [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]                   # H.264 4x4 frame scan
    assert D.ZZ64[:10] == [0, 1, 5, 6, 14, 15, 27, 28, 2, 4] and D.INV64[:9] == [0, 1, 8, 16, 9, 2, 3, 10, 17]
    assert sorted(D.ZZ64) == list(range(64)) and sorted(D.INV16) == list(range(16))
    # the oracle walks the same tables: a level at index r of a block gives scan position INV[r] + 1 coefficient symbols
    for n, inv in ((16, D.INV16), (64, D.INV64)):
        for r in range(n):
            f = D.new_frame(1, 1)
            lv = np.zeros(384, np.int16); lv[64 + r] = 5
            D.put_mb(f, 0, D.P16, 2, 0, n == 64, lv)
            s = O.model_frame_symbols(f, D.nnz24(lv).reshape(1, 24), None)[0]
            assert len(s) == (4 if n == 16 else 1) + inv[r] + 1, (n, r)


@pytest.mark.parametrize("name", sorted(D.FAMILIES))
def test_inputs_obey_the_parsers_contract(name):
    b = D.batch(name)
    for c, i, f in b.jobs():
        assert D.contract_violations(f) == [], (name, c, i)
        assert f.mb_w * f.mb_h <= 600 and f.mb_w * f.mb_h <= b.max_mbs
        assert int(f.mbs["slice_id"].max()) < len(f.slices)
    for c, ch in enumerate(b.chains):
        for i, p in enumerate(b.past[c]):
            assert p is None or p < i
        if b.keep is not None:
            for i, kp in enumerate(b.keep[c]):
                assert kp is None or isinstance(kp, np.ndarray) or kp < i


@pytest.mark.parametrize("name", sorted(D.FAMILIES))
def test_tags_agree_with_the_coders_rule(name):
    """pad derived from the symbol's place in the list == the tag the coder takes out of the prior when pad is 0"""
    for f, k, s in mbs_of(name):
        assert np.all(s["pad"] != 0)
        for x in s:
            kind = int(x["kind"])
            if kind in (D.AC4, D.AC8):
                assert int(x["pad"]) == D.ac_tag_base(int(x["prior"]), kind), (name, k)
            elif kind in (D.NZ4, D.NZ8):
                assert int(x["pad"]) == D.nz_tag(int(x["prior"])), (name, k)
            else:
                assert int(x["pad"]) == (17 if kind == D.LDC else 18)


def test_both_luma_tags_occur():
    seen = set()
    for name in ("last_position", "walk", "neighbours", "neighbours_t8"):
        for f, k, s in mbs_of(name):
            for b, n, start, at, nz, n_ac in D.blocks_of(f, k, s):
                if b < 16:
                    seen |= {(n, int(p)) for p in s["pad"][at + 1:at + 1 + n_ac]}
    assert seen == {(16, 19), (16, 24), (64, 19), (64, 24)}


@pytest.mark.parametrize("name", sorted(D.FAMILIES))
def test_nnz_restatement_is_the_oracles(name):
    """keep None: the numpy rule is model_nnz_images (a macroblock of type 0 takes PAST there)"""
    b = D.batch(name)
    for c, ch in enumerate(b.chains):
        for a, w in zip(D.nnz_images(ch, b.past[c], None), O.model_nnz_images(ch, b.past[c])):
            assert np.array_equal(a, w)


# ---- family 1 ---------------------------------------------------------------------------------------------------------------------------
def test_every_table_entry_decides_a_count():
    t = targets_of("last_position")
    assert len(t) == 48 + 512 + 5 + 32 + 4 + 3
    for cls in ("p16", "i16", "chroma"):
        seen = set()
        for r in range(16):
            f, k, s = t[("last4", cls, r)]
            (b,) = [b for b in range(24) if f.levels[k][b * 16:b * 16 + 16].any()]
            if r == 0 and cls != "p16":                         # the DC went separately: the block is its count symbol, value 0
                assert D.last_positions(f, k, s)[b] == -1 and s["value"][[x[3] for x in D.blocks_of(f, k, s) if x[0] == b][0]] == 0
                continue
            seen.add(D.deciding_index(f, k, s, b, 16))
            assert D.last_positions(f, k, s)[b] == D.INV16[r]
        assert seen == set(range(16)) - ({0} if cls != "p16" else set()), cls
    for cls in ("i8", "p16t8"):
        for blk in range(4):
            seen = {D.deciding_index(*t[("last8", cls, blk, r)], blk * 4, 64) for r in range(64)}
            assert seen == set(range(64)), (cls, blk)


def test_counts_of_the_special_macroblocks():
    t = targets_of("last_position")
    n = lambda what: len(t[what][2])
    assert n(("dc_only", "i16", 32)) == 32 and n(("dc_only", "chroma", 16)) == 16 and n(("i16_empty", 16)) == 16
    for what in (("dc_only", "i16", 32), ("dc_only", "chroma", 16)):
        f, k, s = t[what]
        assert all(nz == 0 and n_ac == 0 for b, _, _, _, nz, n_ac in D.blocks_of(f, k, s))
    assert n(("cbpc", 1)) == 8 and n(("cbpc", 2)) == 8 + 8 + D.INV16[7] + D.INV16[15]
    assert n(("full", "p16")) == D.FULL_P == 408 and n(("full", "i16")) == D.FULL_I16 == 408 and n(("full", "t8")) == D.FULL_T8 == 396
    assert max(len(s) for _, _, s in t.values()) < D.MAX_SYMS
    for t8 in (False, True):
        for cbpl in range(16):
            f, k, s = t[("cbpl", cbpl, t8)]
            assert len(D.blocks_of(f, k, s)) == bin(cbpl).count("1") * (1 if t8 else 4)
    for typ in (D.P16, D.I4, D.I16):
        f, k, s = t[("runs", typ)]
        runs = [1 + n_ac for *_, n_ac in D.blocks_of(f, k, s)]
        assert len(set(runs[:16])) == 16 and len(set(runs[16:])) == 8, runs
    f, k, s = t[("runs", "t8")]
    runs = [1 + n_ac for *_, n_ac in D.blocks_of(f, k, s)]
    assert len(set(runs[:4])) == 4 and len(set(runs[4:])) == 8


# ---- family 2 ---------------------------------------------------------------------------------------------------------------------------
def test_every_wmax_occurs():
    t = targets_of("wmax")
    assert len(t) == 2 * len(D.WMAX4) + 2 * len(D.WMAX8) + 2
    for what, (f, k, s) in t.items():
        if what[0] in ("wmax4", "wmax8"):
            assert D.wmax_of(f, k, s) == what[1], what
    assert {w[1] for w in t if w[0] == "wmax4"} == set(D.WMAX4) and {w[1] for w in t if w[0] == "wmax8"} == set(D.WMAX8)
    for l8, lc in ((63, 1), (0, 15)):
        f, k, s = t[("mixed", l8, lc)]
        lp = D.last_positions(f, k, s)
        assert all(lp[b] == l8 for b in (0, 4, 8, 12)) and all(lp[b] == lc for b in range(16, 24))


# ---- family 3 ---------------------------------------------------------------------------------------------------------------------------
def test_walk_reaches_every_context():
    left, prev, prev2, emitted = set(), set(), set(), set()
    lo = hi = False
    for f, k, s in mbs_of("walk"):
        a, b, c = D.inner_coords(s)
        left |= set(a.tolist()); prev |= set(b.tolist()); prev2 |= set(c.tolist())
        lo, hi = lo or (s["value"] == -32768).any(), hi or (s["value"] == 32767).any()
        for _, n, _, _, _, n_ac in D.blocks_of(f, k, s):
            emitted.add((n, n_ac))
    # a coefficient symbol exists only up to the block's last nonzero level, so at least one is left: min (4, left_nz) is 1..4, never 0
    assert left == {1, 2, 3, 4} and prev == set(range(5)) and prev2 == set(range(5))
    assert lo and hi and (64, 64) in emitted and (16, 16) in emitted and (16, 15) in emitted


# ---- family 4 ---------------------------------------------------------------------------------------------------------------------------
def test_neighbour_priors_are_all_reached():
    triples, taken = set(), set()
    for name in ("neighbours", "slices"):
        for f, k, s in mbs_of(name):
            for b, n, colour, past, left, above in D.nz_contexts(f, k, s):
                assert n == 16
                if name == "neighbours":
                    triples.add((colour, past, left, above))
                i = b - 16 if b >= 16 else b
                if k % f.mb_w and ((b & 3) == 0 if b < 16 else (i & 1) == 0):
                    taken.add((b, "left", left))
                if k >= f.mb_w and (b < 4 if b < 16 else (i & 2) == 0 and (i & 3) < 2):
                    taken.add((b, "above", above))
    assert triples == set(itertools.product(range(3), repeat=4))
    col = [0, 4, 8, 12, 16, 18, 20, 22]
    row = [0, 1, 2, 3, 16, 17, 20, 21]
    assert taken == {(b, "left", v) for b in col for v in range(3)} | {(b, "above", v) for b in row for v in range(3)}


def test_neighbour_priors_of_the_8x8_blocks_are_all_reached():
    seen, across = set(), set()
    for f, k, s in mbs_of("neighbours_t8"):
        for b, n, colour, past, left, above in D.nz_contexts(f, k, s):
            if n == 64:
                blk = b // 4
                seen |= {(blk, "past", past), (blk, "left", left), (blk, "above", above)}
                if k % f.mb_w and blk % 2 == 0:
                    across.add((blk, "left", left))
                if k >= f.mb_w and blk < 2:
                    across.add((blk, "above", above))
    assert seen == set(itertools.product(range(4), ("past", "left", "above"), range(3)))
    assert across == {(s, "left", v) for s in (0, 2) for v in range(3)} | {(s, "above", v) for s in (0, 1) for v in range(3)}


def test_chains_and_slices_are_what_they_claim():
    b = D.batch("neighbours")
    skipped = b.chains[4]
    assert [int(f.mbs["mb_type"][4]) for f in skipped] != [D.SKIP] * 3 and [int(f.mbs["mb_type"][4]) for f in skipped[1:]] == [D.SKIP] * 2
    e = D.expect(b)
    j0 = [j for j, (c, i, _) in enumerate(b.jobs()) if c == 4][0]
    assert e[j0].img[4].any() and np.array_equal(e[j0].img[4], e[j0 + 1].img[4]) and np.array_equal(e[j0].img[4], e[j0 + 2].img[4])
    assert all(int(skipped[2].mbs["mb_type"][k]) not in (D.SKIP, 0) for k in (5, 7))          # the right and lower neighbours are coded
    assert [f.frame_num for f in b.chains[5]] == [0, 1, 1] and b.past[5] == [None, 0, 0]
    assert {(f.mb_w, f.mb_h) for ch in b.chains for f in ch} >= {(1, 7), (7, 1), (1, 1), (6, 6)}
    s = D.batch("slices")
    f = s.chains[0][0]
    assert (f.mb_w, f.mb_h) == (20, 15) and np.array_equal(f.mbs["slice_id"], np.arange(300)) and set(f.slices["slice_type"].tolist()) == {0, 2}
    for g, e in zip(s.chains[0], D.expect(s)):                   # st is the macroblock's own slice's
        for k in range(300):
            if len(e.syms[k]):
                nz = [x for x in e.syms[k] if x["kind"] == D.NZ4][0]
                assert int(nz["prior"]) // (81 * 16) == int(g.slices["slice_type"][k])


# ---- family 5 ---------------------------------------------------------------------------------------------------------------------------
def test_keep_cases_take_every_source():
    b, n = D.batch("keep"), D.batch("keep_null")
    e, en = D.expect(b), D.expect(n)
    src = set()
    differs = False
    for j, (c, i, f) in enumerate(b.jobs()):
        kp, p = b.keep[c][i], b.past[c][i]
        for k in np.flatnonzero(f.mbs["mb_type"] == 0):
            src.add(("caller" if isinstance(kp, np.ndarray) else "none" if kp is None else "job", p is not None))
            want = kp[k] if isinstance(kp, np.ndarray) else np.zeros(24, np.uint8) if kp is None else e[j - i + kp].img[k]
            assert np.array_equal(e[j].img[k], want)
            assert any(int(f.mbs["mb_type"][q]) == D.SKIP for q in range(f.mb_w * f.mb_h)) or i == 0
        differs = differs or not np.array_equal(e[j].img, en[j].img)
        assert any(len(s) for s in e[j].syms)
    assert src >= {("caller", True), ("job", True), ("none", True), ("none", False)}
    assert differs                                              # KEEP is not PAST in these pictures: the two calls must answer differently


# ---- families 6 and 7 -------------------------------------------------------------------------------------------------------------------
def test_sizes_and_job_counts():
    assert sorted(f.mb_w * f.mb_h for ch in D.batch("sizes_small").chains for f in ch) == [1, 3, 20] and D.batch("sizes_small").max_mbs == 20
    assert sorted(f.mb_w * f.mb_h for ch in D.batch("sizes_large").chains for f in ch) == [257, 512, 513]
    for e in D.expect(D.batch("sizes_large")):
        assert e.total > 65535 // 8 and len(set(e.n.tolist())) > 8          # offsets that differ, beyond the first 256 macroblocks too
        assert e.n[256:].any()
    for nj in (1, 256, 257, 513):
        b = D.batch("jobs_%d" % nj)
        assert len(b.jobs()) == nj
        if nj > 1:
            assert {len(ch) for ch in b.chains} >= {1, 2, 7}
            assert len({e.total for e in D.expect(b)}) > 16


def test_small_pool_caps_are_where_they_claim():
    b = D.batch("small_pool")
    e = D.expect(b)
    total, one_less, inside, boundary, none = D.small_pool_caps(b)
    ends = np.concatenate([e[0].off + e[0].n, e[0].total + e[1].off + e[1].n])
    assert total == ends[-1] and one_less == total - 1 and none == 0
    assert e[0].total < inside < total and inside not in ends and boundary in ends and e[0].total < boundary < total
    assert len({total, one_less, inside, boundary, none}) == 5
    assert (e[1].n == 0).any()                                  # a skipped macroblock among them


def test_no_family_is_left_out():
    import test_ctx_directed_gpu as G
    assert set(G.RUN) == set(D.FAMILIES)
    for name in D.FAMILIES:
        assert sum(e.total for e in D.expect(D.batch(name))) > 0, name


# ---- the cases tell a wrong kernel from a right one (shown on the restated derivations) -----------------------------------------------------
def test_count_pass_restated_is_the_oracle_and_no_table_entry_can_move():
    for name in ("last_position", "wmax", "walk", "neighbours_t8", "jobs_257"):
        for f, k, s in mbs_of(name):
            assert D.count_from_raster(f, k) == len(s), (name, k)
    t = targets_of("last_position")
    for i, j in itertools.combinations(range(64), 2):
        inv = list(D.INV64); inv[i], inv[j] = inv[j], inv[i]
        for cls in ("i8", "p16t8"):
            for blk in range(4):
                assert any(D.count_from_raster(t[("last8", cls, blk, r)][0], t[("last8", cls, blk, r)][1], inv64=inv) != len(t[("last8", cls, blk, r)][2]) for r in (i, j)), (i, j, cls, blk)
    for i, j in itertools.combinations(range(16), 2):
        inv = list(D.INV16); inv[i], inv[j] = inv[j], inv[i]
        for cls in ("p16", "i16", "chroma"):
            assert any(D.count_from_raster(t[("last4", cls, r)][0], t[("last4", cls, r)][1], inv16=inv) != len(t[("last4", cls, r)][2]) for r in (i, j)), (i, j, cls)


def test_neighbour_indices_restated_are_the_oracle_and_a_wrong_one_shows():
    wrong = 0
    for name in ("neighbours", "neighbours_t8", "slices", "keep"):
        b = D.batch(name)
        for (c, i, f), e in zip(b.jobs(), D.expect(b)):
            for k in range(f.mb_w * f.mb_h):
                for blk, n, colour, past, left, above in D.nz_contexts(f, k, e.syms[k]):
                    assert D.nz_neighbours(f, k, blk, n, e.img, e.past_img) == (past, left, above), (name, c, i, k, blk)
                    wrong += D.nz_neighbours(f, k, blk, n, e.img, e.past_img, left_of_luma=2) != (past, left, above)
    assert wrong >= 20            # Lf[b + 2] for Lf[b + 3]: the priors of many symbols change, not of one


def test_the_tag_and_the_room_edge_are_in_the_expectation():
    """a kernel that writes the later coefficients' tag on a block's first one, or that refuses a run ending exactly at syms_cap, answers
    differently from the expectation: the first luma coefficient symbols carry 19, and with syms_cap = the total the last run ends on it"""
    b = D.batch("small_pool")
    e = D.expect(b)
    first = [int(s["pad"][at + 1]) for (c, i, f), x in zip(b.jobs(), e) for k, s in enumerate(x.syms) for blk, n, st, at, nz, n_ac in D.blocks_of(f, k, s)
             if blk < 16 and n_ac and int(f.mbs["mb_type"][k]) != D.I16]
    assert len(first) > 20 and set(first) == {19}
    total, _, _, boundary, _ = D.small_pool_caps(b)
    assert e[1].n[-1] > 0 and e[0].total + int(e[1].off[-1] + e[1].n[-1]) == total
    k = int(np.flatnonzero(e[0].total + e[1].off + e[1].n == boundary)[-1])
    assert e[1].n[k] > 0
