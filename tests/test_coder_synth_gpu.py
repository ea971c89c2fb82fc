"""The device coder (lh264_code_chains) against the oracle (orc_coder_symbols) on synthetic streams that steer it into the paths
the fixture streams of tests/test_coder_gpu.py may not reach: edge values of every binariser, degenerate and segment-edge pictures,
DynProbs at probability 0 / 255, LDS cache flushes and a spill table near full, hash_cap and out_cap at their limits, tag lists at
the range stage's chunk sizes, carries through long 0xff runs, one busy partition, and the batch shapes the form choice depends on.
Every tag's length and bytes must equal the oracle's and the status must be 0, unless the scenario is about the status.  The
fixtures and their CPU self-checks: tests/coder_synth.py, tests/test_coder_synth.py."""
import functools

import numpy as np
import pytest

import coder_synth as S

pytestmark = pytest.mark.gpu

# both forms of the first stages; the wave form at the production partition counts (log2p 3 and 4), and at 1 and 128 where cheap
FORMS = [("sw", None), ("wave", 3), ("wave", 4)]
FORMS_ALL = FORMS + [("wave", 0), ("wave", 7)]
FORM_IDS = lambda f: f[0] + ("" if f[1] is None else str(f[1]))


@pytest.fixture
def form(request, monkeypatch):
    path, log2p = request.param
    monkeypatch.setenv("LH264_CODER_PATH", path)
    if log2p is None:
        monkeypatch.delenv("LH264_CODER_LOG2P", raising=False)
    else:
        monkeypatch.setenv("LH264_CODER_LOG2P", str(log2p))
    return request.param


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return [S.oracle(s) for s in _streams(name)]


@functools.lru_cache(maxsize=None)
def _streams(name):
    if name == "c":
        return S.scenario_c(np.random.default_rng(3))
    if name == "f":
        return [[S.random_picture(np.random.default_rng(11), 40)]]
    if name == "j":
        return [[S.random_picture(np.random.default_rng(12), 50)]]
    if name == "k":
        rng = np.random.default_rng(13)
        return [[S.bit_list(30000, 2, (rng.random(30000) < 0.3).astype(np.int16))], [S.raw_list(40000, 69, rng)]]
    return getattr(S, "scenario_" + name)()


def _lengths(o):
    return np.array([len(o.tags.get(t, b"")) for t in S.TAG_OF_SLOT])


def _check(res, ors, what=""):
    assert len(res) == len(ors)
    for i, (r, o) in enumerate(zip(res, ors)):
        assert r.status == 0, "%s stream %d: status %d" % (what, i, r.status)
        assert (r.lens == _lengths(o)).all(), "%s stream %d: lengths %s, oracle %s" % (what, i, r.lens.tolist(), _lengths(o).tolist())
        for t in o.tags:
            assert r.tags[t] == o.tags[t], "%s stream %d tag %d differs" % (what, i, t)


@pytest.mark.parametrize("form", FORMS_ALL, ids=FORM_IDS, indirect=True)
def test_a_every_kind_and_edge_value(form):
    _check(S.device(_streams("a")), _oracle("a"))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS, indirect=True)
def test_b_degenerate_streams(form):
    st = _streams("b")
    _check(S.device(st), _oracle("b"))
    _check(S.device(st, split=True), _oracle("b"), "binarise + finish")


@pytest.mark.parametrize("layout", ["compact", "fixed"])
@pytest.mark.parametrize("form", FORMS_ALL, ids=FORM_IDS, indirect=True)
def test_c_segment_edges_and_symbol_maxima(form, layout):
    _check(S.device(_streams("c"), layout=layout), _oracle("c"))


@pytest.mark.parametrize("form", FORMS_ALL, ids=FORM_IDS, indirect=True)
def test_d_probabilities_0_and_255(form):
    _check(S.device(_streams("d")), _oracle("d"))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS, indirect=True)
def test_e_cache_flushes_and_a_spill_table_near_full(form):
    """the same stream at spill tables of 2^12 .. 2^20 cells in one call: each either exact or status bit 1, never wrong bytes with
    status 0; the largest fits, the smallest does not, and one in between is the smallest that fits (probe chains that wrap)"""
    st, o = _streams("e"), _oracle("e")[0]
    caps = [1 << k for k in range(20, 11, -1)]
    res = S.device(st * len(caps), hash_cap=caps)
    fits = []
    for cap, r in zip(caps, res):
        assert r.status in (0, 1), (cap, r.status)
        if r.status == 0:
            _check([r], [o], "hash_cap %d" % cap)
            fits.append(cap)
    assert caps[0] in fits and caps[-1] not in fits, fits
    assert fits == caps[:len(fits)], fits                  # a table that fits is not followed by a larger one that does not
    smallest = fits[-1]
    r = S.device(st, hash_cap=smallest // 2)[0]            # one step below: reported, never wrong with status 0
    assert r.status == 1


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS, indirect=True)
def test_f_hash_cap_limits_do_not_harm_the_other_streams(form):
    x, o = _streams("f")[0], _oracle("f")[0]
    caps = [1 << 14, 1 << 20, 1 << 21, 0, 3, 1 << 14]
    res = S.device([x] * len(caps), hash_cap=caps)
    _check([res[0], res[1], res[5]], [o, o, o])
    for r in res[2:5]:
        assert r.status & 1, r.status


@pytest.mark.parametrize("form", FORMS_ALL, ids=FORM_IDS, indirect=True)
def test_g_list_lengths_at_the_chunk_sizes(form):
    """tag lists of n + 32 = 256 k, 65,536 k and 262,144 (+-1): the bool coder's chunks (256) and coarse chunks (65,536), and lists
    walked whole by one lane (up to long_list = 262,144) and beyond"""
    _check(S.device(_streams("g_small")), _oracle("g_small"))
    paths = S.range_paths()
    assert paths[0] > 0 and paths[1] > 0, paths                  # first chunks, chunks walked on from the one before


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS, indirect=True)
def test_gh_two_large_streams_and_every_range_path(form):
    """two streams of 4.4 M list entries: the call's average is above 4 M, so lists longer than 65,536 get start-state candidates;
    skewed (probability 255: states only rotate, the whole map), mixed and incompressible lists"""
    _check(S.device(_streams("gh_large"), out_cap=1 << 20, hash_cap=1 << 12), _oracle("gh_large"))
    _, q = S.last_totals()
    assert q / 2 > 4_000_000
    paths = S.range_paths()
    print("range paths (first, walked, one, several, mapped):", paths)
    assert paths[0] > 0 and paths[2] > 0 and paths[3] > 0 and paths[4] > 0, paths


@pytest.mark.parametrize("form", FORMS_ALL, ids=FORM_IDS, indirect=True)
def test_i_carries_through_long_0xff_runs(form):
    _check(S.device(_streams("i")), _oracle("i"))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS, indirect=True)
def test_j_out_cap_boundary(form):
    x, o = _streams("j"), _oracle("j")[0]
    big = max(len(b) for b in o.tags.values())
    for cap in (big, big - 1):
        r = S.device(x, out_cap=cap)[0]
        if cap == big:
            _check([r], [o], "out_cap = largest tag")
        else:
            assert r.status & 4, r.status
            assert (r.lens == _lengths(o)).all()           # the lengths say how much room was needed
        # nothing written behind a tag's bytes (the stop padding byte included) nor behind the last slot
        for slot, ln in enumerate(r.lens):
            assert (r.slots[slot, min(int(ln), cap):] == S.SENTINEL).all(), (cap, slot, int(ln))
        assert (r.slots[35:] == S.SENTINEL).all() and (S.device.tail == S.SENTINEL).all()
        for t, b in o.tags.items():                        # what fits is the oracle's
            assert r.slots[S.TAG_OF_SLOT.index(t), :min(len(b), cap)].tobytes() == b[:cap]


@pytest.mark.parametrize("window", [0, 3])
@pytest.mark.parametrize("form", FORMS_ALL, ids=FORM_IDS, indirect=True)
def test_k_one_busy_partition(form, window, monkeypatch):
    """every decision of a stream on one DynProb / only raw bits (one cell): one partition busy, the others empty"""
    monkeypatch.setenv("LH264_CODER_WINDOW", str(window))
    _check(S.device(_streams("k")), _oracle("k"))


def _expected_form(n, mbs_per_stream):
    """lh264_capi.hip code_binarise: -1 for the sw form, else the partition count"""
    if 384 <= n < 1024 and mbs_per_stream <= 12288:
        return -1
    log2p = 3 if (n >= 512 and mbs_per_stream <= 12288) else 4
    while log2p < 7 and (n << log2p) < 2048:
        log2p += 1
    return 1 << log2p


@functools.lru_cache(maxsize=None)
def _small_pool():
    rng = np.random.default_rng(21)
    st = [[S.random_picture(rng, int(rng.integers(1, 6)), host_max=12, ctx_max=20)] for _ in range(8)]
    return st, [S.oracle(s) for s in st]


@pytest.mark.parametrize("n", [1, 7, 9, 100, 256, 383, 384, 512, 1023, 1024])
def test_l_batch_shapes_choose_form_and_partitions(n, monkeypatch):
    for v in ("LH264_CODER_PATH", "LH264_CODER_LOG2P", "LH264_CODER_WINDOW"):
        monkeypatch.delenv(v, raising=False)
    st, ors = _small_pool()
    streams = [st[i % 8] for i in range(n)]
    _check(S.device(streams, hash_cap=1 << 10, out_cap=1 << 12), [ors[i % 8] for i in range(n)])
    got = S.coder_parts(0)
    print("batch of %d streams: %s" % (n, "sw" if got < 0 else "wave, P = %d" % got))
    assert got == _expected_form(n, sum(s[0].n_mbs for s in streams) // n)


@pytest.mark.parametrize("mbs", [12288, 12289])
def test_l_384_streams_at_the_macroblock_limit(mbs, monkeypatch):
    for v in ("LH264_CODER_PATH", "LH264_CODER_LOG2P", "LH264_CODER_WINDOW"):
        monkeypatch.delenv(v, raising=False)
    st, ors = _small_pool()
    streams = []
    for i in range(384):
        p = st[i % 8][0]
        pad = mbs - p.n_mbs                                   # empty macroblocks behind the symbols: cheap
        streams.append([S.Picture(p.host, np.concatenate([p.host_off, np.full(pad, p.host_off[-1], np.uint32)]), p.ctx,
                                  np.concatenate([p.ctx_n, np.zeros(pad, np.uint16)]))])
    _check(S.device(streams, hash_cap=1 << 10, out_cap=1 << 12), [ors[i % 8] for i in range(384)])
    got = S.coder_parts(0)
    print("384 streams of %d macroblocks: %s" % (mbs, "sw" if got < 0 else "wave, P = %d" % got))
    assert got == _expected_form(384, mbs)


def test_l_one_large_stream_among_many_tiny_ones(monkeypatch):
    for v in ("LH264_CODER_PATH", "LH264_CODER_LOG2P", "LH264_CODER_WINDOW"):
        monkeypatch.delenv(v, raising=False)
    st, ors = _small_pool()
    big = [S.random_picture(np.random.default_rng(22), 3000, host_max=40, ctx_max=200)]
    streams = [st[i % 8] for i in range(300)]
    streams.insert(137, big)
    o = [ors[i % 8] for i in range(300)]
    o.insert(137, S.oracle(big))
    cap = max(len(b) for x in o for b in x.tags.values())            # room for the largest tag of the call, no more
    _check(S.device(streams, hash_cap=[1 << 20 if s is big else 1 << 10 for s in streams], out_cap=cap), o)
    print("one large stream among 300: out_cap %d" % cap)
