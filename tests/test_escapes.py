"""The escape stream, tag 71 of the container (include/lh264.h LH264_TAG_ESC): the part of an mb_skip_run above 511 and of 16 active
references that the prior tables' trees drop.  On the CPU: the front end's accessor, the exact bytes of the format, and both restorers
(the host restore, and the kernel's code stepped on the host with either writer) on the files the compress direction computes with the
tag beside them - for the three streams of tests/golden/escape/ and the four refused streams of tests/golden/edge/."""
import glob
import os

import pytest

import edge_cases as E
import escape_cases as X
import losslessh264_amd as lh

R = __import__("sys").modules["losslessh264_amd.restore"]


def test_committed_streams_regenerate():
    made = X.made()
    assert sorted(made) == X.FIXTURES
    for name, (b, count) in made.items():
        assert b == X.data(name), name
        assert X.REF[name]["sha1"] == E.sha(b) and X.REF[name]["bytes"] == len(b) < 2048, name
        assert X.REF[name]["pictures"] == count["pictures"]


def test_no_escapes_inside_the_range():
    for p in sorted(glob.glob(os.path.join(E.golden_io.GOLDEN_DIR, "streams", "*"))):
        assert lh.escapes(open(p, "rb").read()) == b"", p
    for name in E.NAMES:
        if name not in E.REFUSED:
            assert lh.escapes(E.data(name)) == b"", name
    for name in X.NAMES:
        assert lh.escapes(X.data(name)) != b"" and lh.out_of_range(X.data(name)) != "", name


def test_exact_bytes_of_the_tag():
    """skip512: the IDR picture's 1200 macroblocks read one SKIPRUN symbol each, the run of 512 is the next one: gap 1200 = 0xb0 0x09,
    512 >> 9 = 1, one symbol.  nref_2_3_15_16: 16 pictures of 4 macroblocks with at most 15 references, then 2 x 4 with 16: 16 >> 4 = 1"""
    assert lh.escapes(E.data("skip512")) == bytes([9, 0xb0, 0x09, 1, 1])
    assert lh.escapes(E.data("nref_2_3_15_16")) == bytes([12, 64, 1, 8])
    assert lh.escapes(E.data("skip_all")) == bytes([9, 0xb0, 0x09, 2, 1])


def test_entries_of_the_fixtures():
    """what the generator's docstrings promise: high parts 1, 2 and 3, gaps above 0, NUMREF entries that repeat, close and reopen, one
    entry for a run of pictures, and entries of the two tables interleaved"""
    S, N = X.TB_SKIPRUN, X.TB_NUMREF
    assert X.entries(lh.escapes(X.data("runs_hi"))) == [(S, 1664, 1, 2), (S, 1, 2, 1), (S, 2, 3, 1), (S, 1, 3, 1), (S, 0, 1, 2)]
    # 4 + 15 x 4 symbols in front; 16, 16 | 15 | 16, 16 (first slice of the last picture) | 3
    assert X.entries(lh.escapes(X.data("nref16_mixed"))) == [(N, 64, 1, 8), (N, 4, 1, 6)]
    both = X.entries(lh.escapes(X.data("both")))
    assert both == [(S, 1200, 2, 15), (S, 0, 1, 2), (S, 1, 2, 1), (N, 1200, 1, 3), (S, 2, 2, 2), (N, 1, 1, 1)]
    for name in X.NAMES:
        assert lh.escapes(X.data(name)) == b"".join(X.leb(*e) for e in X.entries(lh.escapes(X.data(name))))


@pytest.mark.parametrize("name", X.NAMES)
def test_both_restorers_return_the_input(name):
    """cpu_compress's files - the reference's own where it decoded the stream - plus tag 71: the host restore, and the kernel's code
    stepped on the host through the CAVLC instance and through the one with the CABAC writer"""
    main, tags = X.with_escapes(name)
    d = X.data(name)
    assert lh.restore(main, tags) == d
    for cabac_device in (False, True):
        outs, paths, st = R.restore_batch_cpu_check([(main, tags)], 1, None, statuses=True, cabac_device=cabac_device)
        assert paths == [R.PATH_DEVICE], (paths, st)
        assert st[0][0] == 0 and outs[0] == d
    # and without the tag the stream does not come back
    try:
        back = lh.restore(main, {t: b for t, b in tags.items() if t != X.TAG_ESC})
    except RuntimeError:
        back = None
    assert back != d


@pytest.mark.parametrize("name", [n for n in X.FIXTURES if X.REF[n]["reference_decodes"]])
def test_files_equal_the_references(name):
    main, tags = X.cpu_compress(name)
    ref = X.REF[name]["files"]
    assert X.TAG_ESC not in tags
    assert E.sha(main) == ref["main"][1] and len(main) == ref["main"][0]
    assert {str(t) for t, b in tags.items() if b} == {k for k in ref if k != "main"}
    for t, b in tags.items():
        if b:
            assert [len(b), E.sha(b)] == ref[str(t)], (name, t)


def _malformed(name):
    """[(label, tag 71)] from the stream's own entries"""
    good = X.entries(lh.escapes(X.data(name)))
    raw = b"".join(X.leb(*e) for e in good)
    t, g, h, r = good[-1]
    head = b"".join(X.leb(*e) for e in good[:-1])
    cases = [("cut inside a varint", head + X.leb(t) + X.leb(g + 300)[:1]),
             ("cut inside an entry", raw[:-1]),
             ("too wide", head + X.leb(t) + b"\xff" * 9 + b"\x7f" + X.leb(h, r)),
             ("high 0", head + X.leb(t, g, 0, r)),
             ("repeat 0", head + X.leb(t, g, h, 0)),
             ("unknown table", head + X.leb(10, g, h, r)),
             ("surplus entry", raw + X.leb(t, 0, 1, 1)),
             ("gap + 1", head + X.leb(t, g + 1, h, r))]
    if t == X.TB_NUMREF:
        cases.append(("num_ref above 16", head + X.leb(t, g, 2, r)))
    return cases


@pytest.mark.parametrize("name", ["skip512", "nref_2_3_15_16", "runs_hi", "nref16_mixed", "both"])
def test_malformed_tags_are_errors(name):
    """an error from both restorers, never other bytes with status 0"""
    main, tags = X.with_escapes(name)
    d = X.data(name)
    assert lh.restore(main, tags) == d
    for label, bad in _malformed(name):
        t2 = dict(tags)
        t2[X.TAG_ESC] = bad
        with pytest.raises(RuntimeError):
            lh.restore(main, t2)
        for cabac_device in (False, True):
            outs, paths, st = R.restore_batch_cpu_check([(main, t2)], 1, None, statuses=True, cabac_device=cabac_device)
            assert st[0][0] != 0 and outs[0] is None, (name, label, st)
            assert paths == [R.PATH_FALLBACK], (name, label, paths)      # the kernel's code noticed; the host restore gave the error


@pytest.mark.parametrize("num_ref", [17, 32])
def test_more_than_16_references_are_not_carried(num_ref):
    """the front end parses up to 32 active references; no restorer accepts more than 16 (the recorded entry would be refused as
    corrupt), so the front end hands out no escape stream for such a stream and compress refuses it with the flag too
    (tests/test_escapes_gpu.py)"""
    name, d = X.beyond(num_ref)
    frames, err = E._parsed[name][:2]
    assert err == "" and len(frames) == 17
    assert lh.out_of_range(d).startswith("num_ref_idx_l0_active %d " % num_ref)
    assert lh.escapes(d) == b""
    assert lh.parse_file(d, pcm=True, escapes=True)[4] == b""
    # what the refusal protects from: the entry the symbols stand for is one both restorers refuse
    main, tags = X.cpu_compress(name)
    tags = dict(tags)
    tags[X.TAG_ESC] = X.leb(X.TB_NUMREF, 64, num_ref >> 4, 4)
    with pytest.raises(RuntimeError, match="more than 16 active references"):
        lh.restore(main, tags)
    outs, paths, st = R.restore_batch_cpu_check([(main, tags)], 1, None, statuses=True)
    assert st[0][0] != 0 and outs[0] is None and paths == [R.PATH_FALLBACK]


def test_parse_file_hands_out_the_escape_stream():
    for name in ("runs_hi", "skip511"):
        d = X.data(name)
        assert lh.parse_file(d, escapes=True)[3] == lh.escapes(d)
        assert lh.parse_file(d, pcm=True, escapes=True)[3:] == (b"", lh.escapes(d))


def test_the_container_carries_the_tag():
    for name in ("runs_hi", "nref16_mixed"):
        main, tags = X.with_escapes(name)
        blob = lh.pack(main, tags)
        assert lh.restore_file(blob) == X.data(name)
        assert blob != lh.pack(main, {t: b for t, b in tags.items() if t != X.TAG_ESC})
