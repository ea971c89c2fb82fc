"""The range-edge streams (tests/golden/edge/, see tests/test_edges.py) through the kernels: compress, restore on the device, decode.

The property every restore path must meet on every edge stream: either compress refuses it, or the restore equals the input."""
import hashlib

import numpy as np
import pytest

import edge_cases as E
import restore_cases as RC
import losslessh264_amd as lh

R = __import__("sys").modules["losslessh264_amd.restore"]
pytestmark = pytest.mark.gpu

NOT_REFUSED = [n for n in E.NAMES if n not in E.REFUSED]
_cache = {}


def _compressed():
    """ONE compress_batch of all edge streams with the default coder path, shared by the restore tests"""
    if "c" not in _cache:
        _cache["c"] = lh.compress_batch([E.data(n) for n in E.NAMES], 16)
    return dict(zip(E.NAMES, _cache["c"]))


@pytest.mark.parametrize("path", ["sw", "wave"])
def test_compress_refuses_or_restores(path, monkeypatch):
    """one batch of all edge streams under both forms of the coder's first stages: the refused set, the files against the reference's
    recorded SHA-1s wherever it decoded the stream, and the restore of everything that was not refused"""
    monkeypatch.setenv("LH264_CODER_PATH", path)
    res = lh.compress_batch([E.data(n) for n in E.NAMES], 16)
    assert {n for n, r in zip(E.NAMES, res) if r[2] is not None} == E.REFUSED
    for name, (main, tags, err) in zip(E.NAMES, res):
        if name in E.REFUSED:
            assert err.startswith(lh.out_of_range(E.data(name))) and "outside the container's range" in err, (name, err)
            continue
        cm, ct = E.cpu_compress(name)
        assert main == cm and {t: x for t, x in tags.items() if x} == ct, name                # the oracle's coder over the same symbols
        if E.REF[name]["reference_decodes"]:
            assert E.same_as_reference_files(name, main, tags), name
        assert lh.restore(main, tags) == E.data(name), name


def test_restore_on_the_device_mixed_with_corpus_streams():
    """one launch: every edge stream that compress hands out and reference-written CAVLC file sets of the corpus; bytes equal to the
    input and to lh264_pip_restore_batch, by the kernel"""
    edge = [(n, _compressed()[n]) for n in NOT_REFUSED]
    assert all(r[2] is None for _, r in edge)
    have_pcm = {"CVPCMNL1_SVA_C.264", "QCIF_2P_I_allIPCM.264"}  # their reference-written sets lack the samples
    corpus = [n for n in RC.CLI if n not in have_pcm and not RC.is_cabac(n)][:6]
    assert len(corpus) == 6
    items = [(r[0], r[1]) for _, r in edge] + [RC.cli_fixture(n) for n in corpus]
    want = [E.data(n) for n, _ in edge] + [RC.data(n) for n in corpus]
    paths = RC.check_same(items, lh.restore_batch_device)
    outs, paths2 = lh.restore_batch_device(items, 16)
    assert paths == paths2
    for i, (o, w) in enumerate(zip(outs, want)):
        assert o == w, "item %d" % i
    assert all(p == R.PATH_DEVICE for p in paths), paths


def test_decode_batch_equals_the_reference_decoder():
    """one decode_batch of all edge streams: the reference decoder's SHA-1 where it decoded the stream, the oracle's pictures for all"""
    b = lh.decode_batch([E.data(n) for n in E.NAMES])
    try:
        for i, name in enumerate(E.NAMES):
            assert (b.status(i), b.error(i)) == (0, ""), name
            got = b.data(i)
            assert len(b.pictures(i)) == E.REF[name]["pictures"], name
            assert got == E.oracle_i420(E.parsed(name)[0]), name
            if E.REF[name]["reference_decodes"]:
                assert hashlib.sha1(got).hexdigest() == E.REF[name]["yuv_sha1"], name
    finally:
        b.free()


def test_zero_run_4160_cut_between_pictures_2_and_3():
    """segments of two pictures: the model's history (the zero run of 4159) crosses the cut in the carried state"""
    d = E.data("zero_run_4160")
    b = lh.compress_batch_handles([d], 16, segment_mbs=2 * 4160)
    try:
        assert b.segments(0) == 2
        main, tags, err = b.result(0)
    finally:
        b.free()
    assert err is None
    whole = _compressed()["zero_run_4160"]
    assert main == whole[0] and {t: x for t, x in tags.items() if x} == {t: x for t, x in whole[1].items() if x}
    assert lh.restore(main, tags) == d
    outs, paths = lh.restore_batch_device([(main, tags)], 1)
    assert outs == [d] and paths == [R.PATH_DEVICE]


def test_a_refused_long_stream_is_refused_in_segments_too():
    """skip513 coded in segments of one picture: the mark is found when its second picture is collected"""
    res = lh.compress_batch([E.data("skip513"), E.data("skip511")], 16, segment_mbs=1200)
    assert res[0][2] is not None and "mb_skip_run 513" in res[0][2]
    assert res[1][2] is None and lh.restore(res[1][0], res[1][1]) == E.data("skip511")


def test_dp_update_on_the_device_for_every_pair_of_counts():
    """the kernel's probability update (a division by a float reciprocal, corrected by one step either way) against the integer
    formula, for every (c0, c1) with c0 + c1 <= 513 and both decisions"""
    c0, c1 = np.meshgrid(np.arange(514, dtype=np.int64), np.arange(514, dtype=np.int64), indexing="ij")
    keep = (c0 + c1) <= 513
    c0, c1 = c0[keep], c1[keep]
    assert len(c0) == 514 * 515 // 2
    words, bits, want = [], [], []
    for bit in (0, 1):
        a, b = c0 + (1 - bit), c1 + bit
        prob = (256 * (a + 1)) // (a + b + 2)
        half = (a + b) > 512
        a2, b2 = np.where(half, (a + 1) >> 1, a), np.where(half, (b + 1) >> 1, b)
        assert int(prob.max()) <= 255 and int(prob.min()) >= 0 and int(max(a2.max(), b2.max())) < 1024
        words.append(c0 | (c1 << 10) | (np.int64(77) << 20))     # the incoming prob field is not read
        bits.append(np.full(len(c0), bit))
        want.append(a2 | (b2 << 10) | (prob << 20))
    words, bits, want = np.concatenate(words), np.concatenate(bits), np.concatenate(want)
    assert len(words) == 264710
    got = R.dp_update_device(words.astype(np.uint32), bits.astype(np.uint8))
    bad = np.flatnonzero(got.astype(np.int64) != want)
    assert len(bad) == 0, "%d of %d differ, the first: c0 %d c1 %d bit %d -> %#x, want %#x" % (
        len(bad), len(want), words[bad[0]] & 1023, (words[bad[0]] >> 10) & 1023, bits[bad[0]], got[bad[0]], want[bad[0]])
