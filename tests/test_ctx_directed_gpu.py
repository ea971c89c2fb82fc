"""The directed inputs of tests/ctx_directed.py through the context-index kernels (the public calls of include/lh264.h, staged by
ctx_directed.Stage), against the oracle and the rules restated beside it: for every macroblock kind, value, prior and pad of every
symbol, n_syms, sym_off, sym_base and the total, and the nnz image; the pool and the fixed slots are compared whole, so nothing is
written where nothing belongs.  tests/test_ctx_directed.py shows (CPU) that the inputs reach what they claim."""
import pytest

import ctx_directed as D

pytestmark = pytest.mark.gpu

RUN = sorted(D.FAMILIES)
FIXED_TOO = ["last_position", "wmax", "walk", "neighbours", "neighbours_t8", "slices", "sizes_small", "sizes_large", "jobs_257"]


def _through_keep(name):
    return name == "keep_null"


@pytest.mark.parametrize("name", RUN)
def test_compact_layout(name):
    """the count call alone (counts, offsets, bases, total; the pool untouched), then the index call"""
    st = D.Stage(D.batch(name))
    D.compare(st, st.count(through_keep=_through_keep(name)))
    D.compare(st, st.index(through_keep=_through_keep(name)))


@pytest.mark.parametrize("name", FIXED_TOO)
def test_fixed_layout(name):
    """sym_off_dev == NULL: symbols at k * 432, n_syms from the symbol pass - the same lists as the compact layout gives"""
    b = D.batch(name)
    st = D.Stage(b.with_layout([(c, i) for c, i, _ in b.jobs()]))
    r = st.index()
    assert len(r.fixed) == len(b.jobs())
    D.compare(st, r)


@pytest.mark.parametrize("name", ["neighbours", "keep", "jobs_513"])
def test_mixed_layouts(name):
    """fixed and compact jobs in one call: the fixed ones count as empty in the bases and the total"""
    b = D.batch(name)
    st = D.Stage(b.with_layout([(c, i) for j, (c, i, _) in enumerate(b.jobs()) if j % 3 == 1]))
    assert 0 < len(st.d_fixed) < len(b.jobs()) and st.total < sum(e.total for e in st.exp)
    D.compare(st, st.count())
    D.compare(st, st.index())


@pytest.mark.parametrize("which", range(5))
def test_pool_too_small(which):
    """syms_cap below the need: the runs that fit are whole, the others read n_syms 0 and nothing at or beyond the cap changes (the
    buffer itself holds the full total); the count call still tells the need"""
    b = D.batch("small_pool")
    cap = D.small_pool_caps(b)[which]
    st = D.Stage(b)
    r = st.index(cap=cap)
    D.compare(st, r)
    assert (r.pool[cap:] == D.UNWRITTEN).all()
    assert st.count().total == st.total
