"""A stream coded in segments of whole pictures, one lh264_code_chains_resume call after another with the coders' state carried in a
per-stream block of device memory, must give the bytes the unsegmented call (lh264_code_chains) gives, wherever the cuts fall: the
reference's files for the golden streams, the oracle's (tests/coder_synth.py) for the synthetic ones.  Fixtures and bookkeeping:
tests/segment_synth.py."""
import functools
import glob
import os

import numpy as np
import pytest

import coder_synth as S
import golden_io
import segment_synth as G

pytestmark = pytest.mark.gpu

MODES = ["whole", "every", 2, 3]


def _cuts(mode):
    if mode == "whole":
        return lambda n: []
    if mode == "every":
        return lambda n: list(range(1, n))
    return lambda n: G.even_cuts(n, mode)


def _lengths(tags):
    return np.array([len(tags.get(t, b"")) for t in S.TAG_OF_SLOT])


def _check(res, want, what):
    """res: DeviceResults; want: {tag: bytes} per stream"""
    assert len(res) == len(want)
    for i, (r, w) in enumerate(zip(res, want)):
        assert r.status == 0, "%s stream %d: status %d" % (what, i, r.status)
        assert (r.lens == _lengths(w)).all(), "%s stream %d: lengths %s, expected %s" % (what, i, r.lens.tolist(), _lengths(w).tolist())
        for t in w:
            assert r.tags[t] == w[t], "%s stream %d tag %d differs" % (what, i, t)


@functools.lru_cache(maxsize=None)
def _synth():
    """synthetic streams with places to cut: escape codes and edge values (a), degenerate streams (b), DynProbs at 0 / 255 and across
    their halving (d), a carry through a long 0xff run (i), random pictures, and tag lists long enough that a segment's list spans
    several coarse chunks of the range walk (65,536 decisions) and is walked from candidate start states (above 262,144).  Pictures of
    more than two macroblocks are cut into three, so that every stream can be cut inside what was one picture"""
    rng = np.random.default_rng(21)
    streams = S.scenario_a() + S.scenario_b() + S.scenario_d() + S.scenario_i()
    streams += [[S.random_picture(np.random.default_rng(30 + k), 30 + 7 * k) for k in range(6)]]
    streams += [[S.bit_list(30000, 2, (rng.random(30000) < 0.3).astype(np.int16)), S.raw_list(40000, 69, rng)]]
    streams += [[S.raw_list(900000, 69, rng), S.bit_list(200000, 8, (rng.random(200000) < 0.1).astype(np.int16), index=40)]]
    cut = [[q for p in s for q in (G.split_picture(p, G.even_cuts(p.n_mbs, 3)) if p.n_mbs > 2 else [p])] for s in streams]
    return streams, cut


@functools.lru_cache(maxsize=None)
def _synth_oracle():
    return [S.oracle(s).tags for s in _synth()[0]]


def test_synthetic_streams_unsegmented_call_equals_the_oracle():
    """the baseline of the tests below: lh264_code_chains on the uncut streams"""
    _check(S.device(_synth()[0], out_cap=1 << 18), _synth_oracle(), "lh264_code_chains")


@pytest.mark.parametrize("log2p", [0, 3, 4])
@pytest.mark.parametrize("mode", MODES, ids=str)
def test_synthetic_streams_cut(mode, log2p, monkeypatch):
    monkeypatch.setenv("LH264_CODER_LOG2P", str(log2p))
    staged = G.stage(_synth()[1])
    run = G.SegRun(staged, out_cap=1 << 18)
    res = run.run_cuts(lambda c: _cuts(mode)(staged.n_pics(c)))
    _check(res, _synth_oracle(), "cut %s, log2p %d" % (mode, log2p))
    if mode == "every":
        assert run.calls == max(staged.n_pics(c) for c in range(staged.n_streams))
    # the decisions of every tag, summed over the segments: the same however the stream was cut
    tr = S.oracle(_synth()[0][8], trace=True).trace
    want = [int((tr[0] == t).sum()) for t in S.TAG_OF_SLOT]
    assert run.decisions(8)[:35] == want


FIXTURES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(golden_io.GOLDEN_DIR, "pip_*.npz")))


@pytest.mark.parametrize("log2p", [0, 3, 4])
def test_golden_streams_cut(log2p, monkeypatch):
    """the streams of tests/test_coder_gpu.py: parsed, context-indexed on the device, then coded whole, as FIRST | LAST, cut after every
    picture, into two and into three - the reference's bytes every time"""
    import losslessh264_amd as lh
    monkeypatch.setenv("LH264_CODER_LOG2P", str(log2p))
    streams, refs = [], []
    for name in FIXTURES:
        z = np.load(os.path.join(golden_io.GOLDEN_DIR, "pip_" + name + ".npz"))
        frames, err = lh.parse_stream(open(os.path.join(golden_io.GOLDEN_DIR, "streams", name), "rb").read())
        assert err == ""
        streams.append(frames[:len(z["hdr"])])
        refs.append({int(k[4:]): z[k].tobytes() for k in z.files if k.startswith("tag_")})
    ctx = lh.CtxSession(streams)
    ctx.run()
    coder = lh.CoderSession(ctx, out_cap=1 << 17)
    coder.run()
    ctx.synchronize()
    for c, name in enumerate(FIXTURES):
        assert coder.tags(c) == refs[c], name
    staged = G.stage_session(coder)
    for mode in MODES:
        run = G.SegRun(staged, hash_cap=coder.hash_cap, out_cap=1 << 17)
        _check(run.run_cuts(lambda c: _cuts(mode)(staged.n_pics(c))), refs, "cut %s" % mode)


def test_streams_in_different_phases_share_a_call():
    """stream A's second segment beside stream B's first beside a FIRST | LAST stream C, then A's last beside B's last"""
    streams, cut = _synth()
    pick = [8, 9, 6, 7]                                       # random pictures, the lists of 30 / 40 k, scenario d, scenario i
    staged = G.stage([cut[k] for k in pick])
    want = [_synth_oracle()[k] for k in pick]
    n = [staged.n_pics(c) for c in range(4)]
    a1, a2 = G.even_cuts(n[0], 3)
    b1, = G.even_cuts(n[1], 2)
    run = G.SegRun(staged, out_cap=1 << 18)
    run.call([(0, 0, a1, G.FIRST)])
    run.call([(0, a1, a2, 0), (1, 0, b1, G.FIRST), (2, 0, n[2], G.FIRST | G.LAST)])
    run.call([(1, b1, n[1], G.LAST), (3, 0, n[3], G.FIRST | G.LAST), (0, a2, n[0], G.LAST)])
    _check(run.results(), want, "mixed phases")


def test_partitions_change_between_the_segments_of_a_stream(monkeypatch):
    """the carry's table is laid out independently of the partitions: a stream's segments coded with 1, 16, 8, 128 and 2 partitions in
    turn (as happens in the batch call, where log2p follows the number of streams of each group) give the stream's bytes"""
    streams, cut = _synth()
    pick = [8, 6, 9, 10]
    staged = G.stage([cut[k] for k in pick])
    run = G.SegRun(staged, out_cap=1 << 18)
    cuts = [[0] + G.even_cuts(staged.n_pics(c), 5) + [staged.n_pics(c)] for c in range(len(pick))]
    for k, log2p in enumerate([0, 4, 3, 7, 1]):
        monkeypatch.setenv("LH264_CODER_LOG2P", str(log2p))
        parts = [(c, x[k], x[k + 1], (G.FIRST if k == 0 else 0) | (G.LAST if k == len(x) - 2 else 0)) for c, x in enumerate(cuts) if k < len(x) - 1]
        assert parts
        run.call(parts)
    assert all(len(x) == 6 for x in cuts[:1])
    _check(run.results(), [_synth_oracle()[k] for k in pick], "log2p 0, 4, 3, 7, 1 in turn")


def test_a_carry_runs_back_into_the_bytes_of_the_segment_before():
    """(a) the first segment ends while tag 30's last bytes are a run of 0xff, and the first addend of the second segment carries into
    them: the bytes already written turn into zeroes, and the byte in front of the run counts one up"""
    streams, at = G.carry_into_ff_run()
    want = [S.oracle(streams[0]).tags]
    assert want == [S.oracle(S.scenario_i()[0]).tags]                    # the same symbols as the uncut fixture
    _check(S.device(streams), want, "lh264_code_chains")
    run = G.SegRun(G.stage(streams))
    run.call([(0, 0, 1, G.FIRST)])
    hdr, rec = run.carry_words(0)
    slot = S.TAG_OF_SLOT.index(30)
    bits, ndec = int(rec[slot, 0]) | int(rec[slot, 1]) << 32, int(rec[slot, 2]) | int(rec[slot, 3]) << 32
    assert ndec == at and hdr[0] == 0 and hdr[1] == 1
    written = run.slot_bytes(0, slot, bits >> 3)
    tail = len(written) - len(written.rstrip(b"\xff"))
    assert tail > 300, "the first segment does not end in a run of 0xff bytes (%d)" % tail
    final = int(run.lens()[0, slot])
    assert final == len(written) - tail - 1, "bytes reported final: %d of %d written, %d of them 0xff" % (final, len(written), tail)
    run.call([(0, 1, 2, 0)])
    after = run.slot_bytes(0, slot, bits >> 3)
    assert after[-tail:] == b"\0" * tail and after[-tail - 1] == written[-tail - 1] + 1 and after[:final] == written[:final]
    run.call([(0, 2, 3, G.LAST)])
    _check(run.results(), want, "cut in front of the carry")


def test_tags_that_come_late_or_pause_and_a_one_macroblock_segment():
    """(b) tag 8 first comes into existence in the third segment, (c) tag 69 has no decision at all in the two middle segments,
    (d) the second segment is a single picture of one macroblock with one decision"""
    streams = G.late_and_absent_tags(np.random.default_rng(5))
    want = [S.oracle(streams[0]).tags]
    assert sorted(want[0]) == [2, 8, 69]
    _check(S.device(streams), want, "lh264_code_chains")
    run = G.SegRun(G.stage(streams))
    run.call([(0, 0, 1, G.FIRST)])
    _, rec = run.carry_words(0)
    exists = [t for s, t in enumerate(S.TAG_OF_SLOT) if rec[s, 5]]
    assert exists == [2, 69]
    run.call([(0, 1, 2, 0)])
    d69 = run.decisions(0)[34]
    run.call([(0, 2, 3, 0)])
    _, rec = run.carry_words(0)
    assert [t for s, t in enumerate(S.TAG_OF_SLOT) if rec[s, 5]] == [2, 8, 69] and run.decisions(0)[34] == d69 == 3 * 3 * 16
    run.call([(0, 3, 4, G.LAST)])
    _check(run.results(), want, "late and pausing tags")
    _check(G.SegRun(G.stage(streams)).run_cuts(lambda c: [1, 2, 3]), want, "again")


def test_a_failed_segment_fails_the_stream():
    """status bits are per segment and sticky: a table that is too small (status 1, coder_synth.scenario_e) in the first segment is
    still reported after the last"""
    st = S.scenario_e(n_cells=40000, passes=1)
    cut = [G.split_picture(st[0][0], G.even_cuts(st[0][0].n_mbs, 2))]
    run = G.SegRun(G.stage(cut), hash_cap=1 << 10)
    res = run.run_cuts(lambda c: [1])
    assert res[0].status & 1 and run.carry_words(0)[0][0] & 1


# ---- the whole path: lh264_compress_batch_opts ------------------------------------------------------------------------------------
def _sha(b):
    import hashlib
    return hashlib.sha1(bytes(b)).hexdigest()


def _batch(datas, segment_mbs=None):
    import losslessh264_amd as lh
    b = lh.compress_batch_handles(datas, 16, segment_mbs=segment_mbs)
    res = [b.result(i) + (b.segments(i), b.pictures(i)) for i in range(b.n)]
    b.free()
    return res


def _same(name, got, want, what):
    assert got[2] is None, "%s %s: %s" % (what, name, got[2])
    assert got[0] == want[0], "%s %s: the default stream differs" % (what, name)
    assert sorted(got[1]) == sorted(want[1]), "%s %s: tags %s, unsegmented %s" % (what, name, sorted(got[1]), sorted(want[1]))
    for t in want[1]:
        assert got[1][t] == want[1][t], "%s %s: tag %d differs" % (what, name, t)


def test_compress_batch_in_segments_gives_the_unsegmented_files():
    """every stream of the reference's sweep that compresses (all but the one tests/test_sweep.py names as REFUSED) in one batch: a
    segment per picture (segment_mbs = 1), and segments of four pictures - the batch once for every picture size among the streams, so
    that each stream meets segment_mbs = 4 x its own picture size -: default stream, set of tags and every tag's bytes as without
    segments, hence the reference's SHA-1s where tests/test_sweep.py holds the stream to them"""
    import losslessh264_amd as lh
    import test_sweep as W
    names = [n for n in W.STREAMS if n not in W.REFUSED]
    datas = [W._data(n) for n in names]
    whole = _batch(datas)
    size = {}
    for name, (main, tags, err, segs, pics) in zip(names, whole):
        assert err is None and segs == (1 if pics else 0), (name, err, segs, pics)
        if name not in W.TAGS_DIFFER:
            ref = W.SWEEP[name]["files"]
            assert _sha(main) == ref["main"][1] and all(_sha(b) == ref[str(t)][1] for t, b in tags.items() if t != W.TAG_PCM), name
        frames, _ = lh.parse_stream(W._data(name))
        size[name] = frames[0].mb_w * frames[0].mb_h if frames else 0
    for S_mbs in [1] + sorted({4 * v for v in size.values() if v}):
        cut = _batch(datas, segment_mbs=S_mbs)
        for name, got, want in zip(names, cut, whole):
            _same(name, got, want, "segment_mbs %d" % S_mbs)
            pics = got[4]
            assert pics == want[4]
            if S_mbs == 1:
                assert got[3] == pics and (got[3] > 1) == (pics > 1), (name, got[3], pics)
            elif size[name] * 4 == S_mbs:
                assert got[3] >= (pics + 3) // 4, (name, got[3], pics)
    # a refused stream stays refused, whole or cut
    for S_mbs in (None, 1):
        bad = _batch([W._data(n) for n in sorted(W.REFUSED)], segment_mbs=S_mbs)
        assert all(r[2] is not None and not r[1] for r in bad)


def test_compress_batch_large_pictures_a_segment_each():
    """the synthetic 720p / 1080p streams of tests/restore_cases.py, a picture per segment"""
    import restore_cases as R
    datas = [R.data(n) for n in R.SYNTH]
    whole, cut = _batch(datas), _batch(datas, segment_mbs=1)
    for name, got, want in zip(R.SYNTH, cut, whole):
        _same(name, got, want, "segment_mbs 1")
        assert got[3] == got[4] > 1 and want[3] == 1, (name, got[3], got[4], want[3])


def test_decisions_do_not_depend_on_the_cut():
    import losslessh264_amd as lh
    data = open(os.path.join(golden_io.GOLDEN_DIR, "streams", "BA_MW_D.264"), "rb").read()
    counts = []
    for S_mbs in (None, 1, 99 * 7):
        b = lh.compress_batch_handles([data, data + data], 4, segment_mbs=S_mbs)
        assert b.status(0) == 0 and b.status(1) == 0
        counts.append([[b.decisions(i, t) for t in S.TAG_OF_SLOT] for i in range(2)])
        b.free()
    assert counts[0] == counts[1] == counts[2] and sum(counts[0][0]) > 100000
    assert all(2 * x >= y >= x for x, y in zip(counts[0][0], counts[0][1]))      # two copies: the decisions of both


# ---- a stream that does not fit one coder call -------------------------------------------------------------------------------------
def _ba_mw_d():
    return open(os.path.join(golden_io.GOLDEN_DIR, "streams", "BA_MW_D.264"), "rb").read()


def _handles(data, segment_mbs=None):
    import losslessh264_amd as lh
    b = lh.compress_batch_handles([data], 16, segment_mbs=segment_mbs)
    main, tags, err = b.result(0)
    out = dict(main=main, tags=tags, err=err, segments=b.segments(0), pictures=b.pictures(0),
               decisions={t: b.decisions(0, t) for t in S.TAG_OF_SLOT})
    b.free()
    return out


def test_a_stream_beyond_one_coder_call():
    """BA_MW_D.264 concatenated K times is a valid stream (every copy starts with its parameter sets and an IDR picture) whose adaptive
    state runs on across the copies.  K is computed: the largest per-tag decision count n1 of one copy, K = ceil (1.1 x 2^27 / n1) - that
    tag's list is then longer than the 2^27 entries one lh264_code_chains call can address.  With the default options the stream
    compresses in more than one segment, restores to the input, and every tag's bytes equal those of a second run cut every 100
    pictures.  (The uncut run is not made: its memory is in proportion to the stream.)"""
    import losslessh264_amd as lh
    one = _ba_mw_d()
    r1 = _handles(one)
    assert r1["err"] is None and r1["segments"] == 1
    tag1, n1 = max(r1["decisions"].items(), key=lambda kv: kv[1])
    K = -(-int(1.1 * (1 << 27)) // n1)
    print("one copy: %d pictures, largest list tag %d with %d decisions, all tags %d; K = %d copies, %d bytes" %
          (r1["pictures"], tag1, n1, sum(r1["decisions"].values()), K, K * len(one)))
    assert 100 <= K <= 20000
    data = one * K
    a = _handles(data)
    print("default options: %d segments, %d bytes of tags, tag %d: %d decisions" % (a["segments"], sum(len(b) for b in a["tags"].values()), tag1, a["decisions"][tag1]))
    assert a["err"] is None, a["err"]
    assert a["segments"] > 1 and a["pictures"] == K * r1["pictures"]
    assert a["decisions"][tag1] > 1 << 27 and a["decisions"][tag1] == K * n1
    assert lh.restore(a["main"], a["tags"]) == data
    b = _handles(data, segment_mbs=100 * 99)
    print("segment_mbs 9,900: %d segments" % b["segments"])
    assert b["err"] is None and b["segments"] >= K and b["decisions"] == a["decisions"]
    assert b["main"] == a["main"] and sorted(b["tags"]) == sorted(a["tags"])
    for t in a["tags"]:
        assert b["tags"][t] == a["tags"][t], "tag %d differs between the two cuts" % t


def test_a_segment_over_the_coders_counter_is_sent_again(monkeypatch):
    """The coder codes fewer than 2^27 decisions into ALL tag lists of a stream in one call; one copy of BA_MW_D.264 has 683 k.  With
    the estimate that normally cuts segments by their decisions switched off (LH264_COMPRESS_DECISIONS), the count pass is asked:
      * 256 copies and a segment size above the stream: a WHOLE stream of 175 M decisions - status 8 from lh264_code_chains, the stream
        becomes a long one and is sent again in halves;
      * 400 copies and segments of 300: a long stream whose FIRST segment (205 M) is over the limit - status 8 from
        lh264_code_chains_resume with the carry untouched, sent again with 150 copies a segment.
    Status OK, more than one segment, and the bytes of a run cut every 100 pictures; then the same with the estimate at work (the
    default): no segment is refused, the bytes are the same."""
    one = _ba_mw_d()
    per_copy = sum(_handles(one)["decisions"].values())
    assert 600000 < per_copy < 800000
    for K, seg_mbs in ((256, 10 ** 7), (400, 300 * 9900)):
        data = one * K
        assert min(K, seg_mbs // 9900) * per_copy > 1 << 27 and (min(K, seg_mbs // 9900) // 2) * per_copy < 1 << 27
        ref = _handles(data, segment_mbs=9900)
        assert ref["err"] is None and ref["segments"] == K
        monkeypatch.setenv("LH264_COMPRESS_DECISIONS", str(1 << 40))
        a = _handles(data, segment_mbs=seg_mbs)
        monkeypatch.delenv("LH264_COMPRESS_DECISIONS")
        b = _handles(data, segment_mbs=seg_mbs)
        print("K = %d, segment_mbs %d: %d segments after the count pass's answer, %d with the estimate" % (K, seg_mbs, a["segments"], b["segments"]))
        for r in (a, b):
            assert r["err"] is None, r["err"]
            assert r["segments"] > 1 and r["pictures"] == 100 * K and r["decisions"] == ref["decisions"]
            assert r["main"] == ref["main"] and sorted(r["tags"]) == sorted(ref["tags"])
            for t in ref["tags"]:
                assert r["tags"][t] == ref["tags"][t], "K = %d: tag %d differs" % (K, t)
        assert a["segments"] == (2 if K == 256 else 3)           # halves; 150 + 150 + 100 copies
        assert b["segments"] >= K * per_copy // (1 << 26)        # cut by the estimate: at most 2^26 estimated decisions a segment


def test_eight_copies_equal_the_reference_console_application(tmp_path):
    """K = 8: the files the reference's own console application writes (407,158 bytes in all), where that binary has been built"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "h264dec")
    data = _ba_mw_d() * 8
    cuts = [_handles(data), _handles(data, segment_mbs=99), _handles(data, segment_mbs=99 * 150)]
    assert [c["segments"] for c in cuts] == [1, 800, 6] and all(c["err"] is None for c in cuts)
    for c in cuts[1:]:
        assert c["main"] == cuts[0]["main"] and c["tags"] == cuts[0]["tags"]
    assert len(cuts[0]["main"]) + sum(len(b) for b in cuts[0]["tags"].values()) == 407158
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/h264dec is not built here (the reference's sources are not on this machine): the comparison with its files is left out")
    src, dst = str(tmp_path / "in.264"), str(tmp_path / "out.pip")
    open(src, "wb").write(data)
    subprocess.run([exe, src, dst], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert open(dst, "rb").read() == cuts[0]["main"]
    ref = {int(f.rsplit(".", 1)[1]): open(str(tmp_path / f), "rb").read() for f in os.listdir(str(tmp_path)) if f.startswith("out.pip.")}
    assert ref == cuts[0]["tags"]


# ---- memory follows the segment, not the stream --------------------------------------------------------------------------------------
_CHILD = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, %r)
import losslessh264_amd as lh
from losslessh264_amd import _lib as L
K = int(sys.argv[1])
one = open(%r, "rb").read()
b = lh.compress_batch_handles([one * K], 16, segment_mbs=9900)
main, tags, err = b.result(0)
dev, pin = C.c_size_t(0), C.c_size_t(0)
L.check(L.lib().lh264_compress_arena_bytes(C.byref(dev), C.byref(pin)))
print(json.dumps(dict(err=err, segments=b.segments(0), device=dev.value, pinned=pin.value, tagged=sum(len(x) for x in tags.values()), input=len(one) * K)))
"""


def test_memory_is_bounded_by_the_segment_not_the_stream():
    """64 and then 256 copies of BA_MW_D.264 in segments of 100 pictures, each in a fresh process (the buffers only grow inside one): what
    the library holds on the device and page-locked after the longer stream exceeds what it holds after the shorter one by no more
    than may grow with the stream - the two results' tagged bytes, and the prior table (hash_cap x 64 bytes, sized from the file's
    length and capped at 2^20 cells: the same for both)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD % (root, os.path.join(golden_io.GOLDEN_DIR, "streams", "BA_MW_D.264"))
    got = {}
    for K in (64, 256):
        out = subprocess.run([sys.executable, "-c", code, str(K)], check=True, capture_output=True, timeout=600).stdout.decode()
        got[K] = json.loads(out.strip().splitlines()[-1])
        print("K = %d: %s" % (K, got[K]))
        assert got[K]["err"] is None and got[K]["segments"] >= K
    caps = []
    for K in (64, 256):
        hc = 1 << 13
        while hc * 2 < got[K]["input"] and hc < (1 << 20):
            hc <<= 1
        caps.append(hc)
    assert caps[0] == caps[1] == 1 << 20
    allowed = got[64]["tagged"] + got[256]["tagged"] + caps[1] * 64
    for what in ("device", "pinned"):
        assert got[256][what] - got[64][what] <= allowed, (what, got[64][what], got[256][what], allowed)


def test_command_lines_take_segment_mbs(tmp_path):
    """`lh264dec --segment-mbs N` and `python -m losslessh264_amd --segment-mbs N` write the files the reference's console application
    wrote for the stream (tests/golden/cli_*.npz), coded in segments of two pictures"""
    import subprocess
    import sys
    import restore_cases as R
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "SVA_BA2_D.264"
    main, tags = R.cli_fixture(name)
    src = os.path.join(golden_io.GOLDEN_DIR, "streams", name)
    for k, cmd in enumerate(([os.path.join(root, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"])):
        d = tmp_path / str(k)
        d.mkdir()
        dst = str(d / "out.pip")
        out = subprocess.run(cmd + ["--segment-mbs", "198", src, dst], check=True, capture_output=True, timeout=300, cwd=root).stdout.decode()
        assert open(dst, "rb").read() == main
        got = {int(f.rsplit(".", 1)[1]): open(str(d / f), "rb").read() for f in os.listdir(str(d)) if f.startswith("out.pip.")}
        assert got == tags, (cmd, sorted(got), sorted(tags))
        if k == 1:
            assert " segments" in out and int(out.split(",")[-1].split()[0]) > 1, out
