"""The synthetic coder fixtures (tests/coder_synth.py) on the CPU: each scenario has the property it exists for, read from the
oracle's decision trace and output, so that a fixture cannot drift off its target unnoticed.  tests/test_coder_synth_gpu.py codes
the same fixtures on the device."""
import os

import numpy as np
import pytest

import coder_synth as S


def _run(tr, tag):
    """longest run of consecutive 1-bits among the decisions of `tag` that follow one another in the trace"""
    t, _, b = tr
    m = ((t == tag) & (b == 1)).astype(np.int8)
    best = cur = 0
    for x in m:
        cur = cur + 1 if x else 0
        best = max(best, cur)
    return best


def test_flatten_puts_the_coefficient_symbols_at_the_marker():
    pic = S.Picture.from_lists([([S.raw(1, 1, 9), S.splice(), S.raw(2, 3, 9)], [S.csym(S.AC4, 7, 1), S.csym(S.AC4, 8, 2)]),
                                ([S.raw(3, 5, 9)], [S.csym(S.AC4, 9, 3)]),            # no marker: never coded
                                ([S.splice()], []), ([], [])])
    f = S.flatten([pic])
    assert list(f["kind"]) == [S.RAW, S.AC4, S.AC4, S.RAW, S.RAW]
    assert list(f["value"]) == [1, 1, 2, 3, 5]


def test_domain_of_the_random_generator():
    rng = np.random.default_rng(1)
    pic = S.random_picture(rng, 300)
    h = pic.host
    assert ((h["kind"] >= S.TREE) & (h["kind"] <= S.MVD) | (h["kind"] == S.SPLICE)).all()
    tb = h["prior"] >> 27
    tree = h["kind"] == S.TREE
    assert set(np.unique(tb[tree])) <= {t[0] for t in S.TREES}
    assert set(np.unique(tb[h["kind"] == S.POW2])) <= {S.TB_MODE8, S.TB_QPL}
    assert (h["prior"][h["kind"] == S.RAW] <= 16).all()
    tags = h["pad"][h["kind"] != S.SPLICE]
    assert ((tags <= 33) | (tags == 69)).all()
    c = pic.ctx
    pads = c["pad"]
    implied = np.array([S.implied_tag(int(k), int(p)) for k, p in zip(c["kind"], c["prior"])])
    assert ((pads == 0) | (pads == implied)).all()
    for n in np.diff(pic.host_off.astype(np.int64)):
        assert n <= S.MAX_SYN
    assert (np.bincount(np.searchsorted(pic.host_off, np.nonzero(h["kind"] == S.SPLICE)[0], side="right") - 1) <= 1).all()


def test_a_every_kind_and_table_and_the_longest_exponent():
    st = S.scenario_a()[0]
    f = S.flatten(st)
    pairs = {(int(k), int(p) >> 27) for k, p in zip(f["kind"], f["prior"]) if k >= S.TREE and k != S.RAW}
    assert {(S.TREE, t[0]) for t in S.TREES} <= pairs
    assert {(S.POW2, S.TB_MODE8), (S.POW2, S.TB_QPL), (S.BIT, S.TB_STOP), (S.BIT, S.TB_T8), (S.MVD, S.TB_MVD)} <= pairs
    assert set(np.unique(f["kind"])) == {S.LDC, S.CDC, S.NZ4, S.AC4, S.NZ8, S.AC8, S.TREE, S.POW2, S.BIT, S.RAW, S.MVD}
    assert {0, 1, 16} <= set(f["prior"][f["kind"] == S.RAW].tolist())
    for k in (S.LDC, S.AC4, S.AC8):
        assert {-32768, 32767, 0}.issubset(set(f["value"][f["kind"] == k].tolist()))
    r = S.oracle(st, trace=True)
    # 32767 as a coefficient: 32766 - 14 beyond the unary part -> exponent of 14 ones (EXP tags 21 / 26 / 31); as a DC: 15 ones (tag 17)
    assert max(_run(r.trace, t) for t in (21, 26, 31)) >= 14
    assert _run(r.trace, 17) >= 15
    assert max(_run(r.trace, t) for t in (15, 16)) >= 9            # the motion vector difference's unary part up to N = 9


def test_b_an_exp_tag_exists_without_a_decision():
    st = S.scenario_b()
    r = S.oracle(st[0], trace=True)
    assert 21 in r.tags and not (r.trace[0] == 21).any()        # the AC symbol of value 0: EXP stream touched, no decision on it
    assert S.oracle(st[1]).tags == {} and S.oracle(st[2]).tags == {}


def test_d_probabilities_0_and_255_are_reached():
    r = S.oracle(S.scenario_d()[0], trace=True)
    t, p, b = r.trace
    for tag in (2, 69, 30):
        m = t == tag
        assert ((p[m] == 0) & (b[m] == 0)).any(), tag            # a 0 at probability 0: list entry q = 256
        if tag != 69:                                              # (one DynProb: only one of the two extremes)
            assert ((p[m] == 255) & (b[m] == 1)).any(), tag
        assert (m.sum()) > 2 * 512                               # several halvings


def test_e_many_dynprobs():
    st = S.scenario_e()[0]
    f = S.flatten(st)
    distinct = len(np.unique(f["prior"][f["kind"] == S.AC4]))
    assert distinct > 600 * 128 and distinct > 4600                # above every flush threshold of the LDS caches, at every P
    assert len(f) > 2 * distinct                                   # revisited


def test_g_list_lengths_from_the_trace():
    """tag 69's list plus the 32 stop decisions lands on 256, 512 (chunks), 65,536, 131,072 (coarse chunks) and 262,144 (long_list),
    each exactly and one either side"""
    got = []
    for s in S.scenario_g_small():
        r = S.oracle(s, trace=True)
        n = int((r.trace[0] == 69).sum())
        assert len(r.trace[0]) == n
        got.append(n + 32)
    assert sorted(got) == sorted(m + d for m in (256, 512, 65536, 131072, 262144) for d in (-1, 0, 1))


def test_g_large_streams_hold_over_4m_entries():
    st = S.scenario_gh_large()
    for s in st:
        assert len(S.flatten(s)) > 0
        n = sum(int(((p.host["kind"] == S.RAW) * p.host["prior"].astype(np.int64)).sum() + (p.host["kind"] == S.BIT).sum()) for p in s)
        assert n > 4_000_000


def test_i_a_carry_through_300_0xff_bytes():
    r = S.oracle(S.scenario_i()[0], trace=True)
    t, p, b = r.trace
    for tag, carry in ((30, True), (25, False)):
        m = t == tag
        assert (p[m] == 128).all()
        got, run = S.bool_code(b[m], p[m])
        assert got == r.tags[tag]                                  # the Python replay is the oracle's coder
        if carry:
            assert run >= 300, run
        else:
            assert run == 0 and b"\xff" * 300 in got


@pytest.mark.skipif(not os.path.exists(S.REF_CODER), reason="oracle/_ref (the reference, built by oracle/Makefile) is not present")
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "i", "random"])
def test_oracle_equals_the_reference_coder(name):
    """orc_coder_symbols (the oracle every device test compares with) against the reference's own emitInt / emitUEGkInt / Branch<n> /
    emitBitsZeroToPow2Inclusive / emitBits / vpx_writer on the synthetic fixtures: int16 extremes, probability 0 and 255 with the
    q = 256 entry, halving, carries through 0xff runs - identical bytes in every tag"""
    if name == "c":
        streams = S.scenario_c(np.random.default_rng(3))
    elif name == "random":
        streams = [[S.random_picture(np.random.default_rng(s), 200)] for s in range(4)]
    else:
        streams = getattr(S, "scenario_" + name)()
    for st in streams:
        assert S.oracle(st).tags == S.ref_code(st)
