"""The CABAC syntax-edge streams (tests/golden/cabac_edge/, see tests/test_cabac_edges.py) through the kernels: compress under both
coder paths, restore on the device with the CABAC writer of restore_cabac_kernel, decode.

The property every restore path must meet on every stream: either compress refuses it, or the restore equals the input."""
import hashlib
import sys

import pytest

import cabac_edge_cases as CE
import edge_cases as E
import restore_cabac_fixtures as FX
import restore_cases as RC
import losslessh264_amd as lh

R = sys.modules["losslessh264_amd.restore"]
pytestmark = pytest.mark.gpu

_cache = {}


def _compressed():
    """ONE compress_batch of all CABAC edge streams with the default coder path, shared by the restore tests"""
    if "c" not in _cache:
        _cache["c"] = lh.compress_batch([CE.data(n) for n in CE.NAMES], 16)
    return dict(zip(CE.NAMES, _cache["c"]))


def _nonempty(tags):
    return {t: x for t, x in tags.items() if x}


@pytest.mark.parametrize("path", ["sw", "wave"])
def test_compress_refuses_or_restores(path, monkeypatch):
    """one batch under each form of the coder's first stages: the refused set, the files against the oracle's coder over the same
    symbols and against the reference's recorded SHA-1s, and the host restore of everything that was not refused"""
    monkeypatch.setenv("LH264_CODER_PATH", path)
    res = lh.compress_batch([CE.data(n) for n in CE.NAMES], 16)
    assert {n for n, r in zip(CE.NAMES, res) if r[2] is not None} == CE.REFUSED
    for name, (main, tags, err) in zip(CE.NAMES, res):
        if name in CE.REFUSED:
            assert err.startswith(lh.out_of_range(CE.data(name))) and "outside the container's range" in err, (name, err)
            continue
        cm, ct = CE.cpu_compress(name)
        assert main == cm and _nonempty(tags) == ct, name
        if CE.REF[name]["reference_decodes"]:
            assert CE.same_as_reference_files(name, main, tags), name
        assert lh.restore(main, tags) == CE.data(name), name


def test_restore_on_the_device_with_the_cabac_writer():
    """one launch: every CABAC edge stream, every CAVLC edge stream that compress hands out and three CABAC file sets of the corpus
    (small ones: the kernel restores a stream as one chain, and the whole CIF streams, which tests/test_restore_cabac_gpu.py sends
    through it, would take this test from seconds to most of a minute); as lh264_pip_restore_batch, bytes equal to the input, all by the kernel.  Without the flag the CABAC ones are the host's,
    with the same bytes"""
    cab = [(n, _compressed()[n]) for n in CE.NOT_REFUSED]
    assert all(r[2] is None for _, r in cab)
    cav = [n for n in E.NAMES if n not in E.REFUSED]
    cav_res = lh.compress_batch([E.data(n) for n in cav], 16)
    assert all(r[2] is None for r in cav_res)
    corpus = [RC.cli_fixture("test_qcif_cabac.264"), FX.load(FX.OWN_IPCM)[:2], FX.load(FX.CONCAT)[:2]]
    corpus_want = [RC.data("test_qcif_cabac.264"), RC.data("QCIF_2P_I_allIPCM.264"), RC.data("BA_MW_D.264") + RC.data("test_qcif_cabac.264")]
    items = [(r[0], r[1]) for _, r in cab] + [(r[0], r[1]) for r in cav_res] + corpus
    want = [CE.data(n) for n, _ in cab] + [E.data(n) for n in cav] + corpus_want
    names = CE.NOT_REFUSED + cav + ["test_qcif_cabac.264", FX.OWN_IPCM, FX.CONCAT]

    def dev(its, threads=0, out_cap=None, statuses=False):
        return R.restore_batch_device(its, threads, out_cap, statuses, cabac_device=True)
    paths = RC.check_same(items, dev)                             # status, length and bytes are the host batch's ...
    assert paths == [R.PATH_DEVICE] * len(items), dict(zip(names, paths))
    for n, (st, ln, o), w in zip(names, RC.host_results(items), want):
        assert st == 0 and o == w, n                              # ... which are the inputs
    outs, paths = R.restore_batch_device(items, 16)
    for n, o, w in zip(names, outs, want):
        assert o == w, n
    is_cabac = [True] * len(cab) + [False] * len(cav) + [True] * len(corpus)
    assert paths == [R.PATH_HOST if c else R.PATH_DEVICE for c in is_cabac], dict(zip(names, paths))


def test_sixteen_references_with_escapes():
    """cabac_refidx16 with escapes=True: tag 71 is there; the host restore, the device call with the CABAC writer in the kernel and the
    device call without it (which hands a CABAC stream to the host's writer) all return the input"""
    d = CE.data("cabac_refidx16")
    (main, tags, err), = lh.compress_batch([d], 16, escapes=True)
    assert err is None and tags.get(CE.TAG_ESC)
    assert tags[CE.TAG_ESC] == lh.escapes(d)
    assert lh.restore(main, tags) == d
    outs, paths = lh.restore_batch_device([(main, tags)], 1, cabac_device=True)
    assert outs == [d] and paths == [R.PATH_DEVICE]
    outs, paths = lh.restore_batch_device([(main, tags)], 1)
    assert outs == [d] and paths == [R.PATH_HOST]


def test_decode_batch_equals_the_reference_decoder():
    """one decode_batch of all streams: the oracle's pictures for all, the reference decoder's SHA-1 where it decoded the stream"""
    b = lh.decode_batch([CE.data(n) for n in CE.NAMES])
    try:
        for i, name in enumerate(CE.NAMES):
            assert (b.status(i), b.error(i)) == (0, ""), name
            got = b.data(i)
            assert len(b.pictures(i)) == CE.REF[name]["pictures"], name
            assert got == E.oracle_i420(CE.parsed(name)[0]), name
            if CE.REF[name]["reference_decodes"]:
                assert hashlib.sha1(got).hexdigest() == CE.REF[name]["yuv_sha1"], name
    finally:
        b.free()


def test_mixed_cut_between_its_pictures():
    """cabac_mixed in segments of one picture: the carried state crosses every change of entropy coder; the files are those of the
    whole stream"""
    d = CE.data("cabac_mixed")
    b = lh.compress_batch_handles([d], 16, segment_mbs=16)
    try:
        assert b.segments(0) == 6
        main, tags, err = b.result(0)
    finally:
        b.free()
    assert err is None
    whole = _compressed()["cabac_mixed"]
    assert main == whole[0] and _nonempty(tags) == _nonempty(whole[1])
    assert lh.restore(main, tags) == d
