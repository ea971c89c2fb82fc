"""The streams of tests/golden/uncoded_t8/ (macroblocks that code nothing under the 8x8 transform, see tests/test_uncoded_t8.py)
through the kernels: slice_parse_kernel and slice_parse_cabac_kernel against their CPU forms, lh264_decode_batch on every parse route
against the oracle's pictures and the reference's recorded SHA-1s, compress under both coder paths, restore on the device with either
writer, and the stream cut in segments of one picture.  Bytes against bytes; the streams are a few hundred bytes each."""
import hashlib
import sys

import pytest

import losslessh264_amd as lh
import uncoded_t8_cases as U
from losslessh264_amd import slice_parse as SP
from test_slice_parse_gpu import same_dump

R = sys.modules["losslessh264_amd.restore"]
pytestmark = pytest.mark.gpu

DATAS = [U.data(n) for n in U.NAMES]


def _nonempty(tags):
    return {t: x for t, x in tags.items() if x}


# ---- the device parsers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.NAMES)
def test_parse_kernels_equal_their_cpu_forms(name):
    """records, coefficient planes, slice tables, results, guards.  A CAVLC stream goes through slice_parse_kernel and, with the CABAC
    switch on, through the instance that holds both; a CABAC stream through slice_parse_cabac_kernel"""
    data = U.data(name)
    for cabac in ((True,) if name in U.CABAC else (False, True)):
        cpu, g0, e0 = SP.slice_parse(data, threads=4, cabac=cabac)
        assert g0 and sum(p.n_deferred for p in cpu) == sum(len(f.slices) for f in U.parsed(name).frames)
        assert all((p.results[:, 1] == 0).all() for p in cpu)
        dev, g1, e1 = SP.slice_parse(data, on_device=True, cabac=cabac)
        assert g1, "guard bytes were overwritten on the device"
        assert e0 == e1
        same_dump(cpu, dev)


# ---- decode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(parse="device"), dict(parse="device+cabac"), dict(round_pictures=1), dict(parse="device+cabac", round_pictures=1)],
                         ids=["host", "device", "device+cabac", "host-round1", "device+cabac-round1"])
def test_decode_batch_equals_the_oracle_and_the_reference(kw):
    """one decode_batch of all streams: the oracle's I420 for all, the reference's SHA-1 per picture for all but the one stream it
    decodes otherwise.  round_pictures=1: one picture a round, so that a QP carried to the end of a picture is seen not to reach the
    next one"""
    b = lh.decode_batch(DATAS, **kw)
    try:
        for i, name in enumerate(U.NAMES):
            assert (b.status(i), b.error(i)) == (0, ""), name
            got = b.data(i)
            assert len(b.pictures(i)) == len(U.REF[name]["picture_sha1"]), name
            assert got == b"".join(U.pictures(name)), name
            same = [hashlib.sha1(got[at:at + U.PIC_BYTES]).hexdigest() == want for at, want in zip(range(0, len(got), U.PIC_BYTES), U.REF[name]["picture_sha1"])]
            assert same == ([False, True, False, False] if name in U.NOT_AS_THE_REFERENCE else [True] * len(same)), name
            route = "host" if "parse" not in kw or (name in U.CABAC and kw["parse"] == "device") else "device"
            assert b.parse_path(i) == route, name
            if route == "device":
                assert b.device_slices(i) == sum(len(f.slices) for f in U.parsed(name).frames), name
                assert (b.device_cabac_slices(i) > 0) == (name in U.CABAC), name
    finally:
        b.free()


# ---- compress and restore ---------------------------------------------------------------------------------------------------------------
_cache = {}


def _compressed():
    if "c" not in _cache:
        _cache["c"] = lh.compress_batch(DATAS, 16)
    return _cache["c"]


@pytest.mark.parametrize("path", ["sw", "wave"])
def test_compress_under_both_coder_paths(path, monkeypatch):
    """no refusal; the files are the CPU compress of the same symbols; lh.restore returns the input"""
    monkeypatch.setenv("LH264_CODER_PATH", path)
    res = lh.compress_batch(DATAS, 16)
    for name, (main, tags, err) in zip(U.NAMES, res):
        assert err is None, (name, err)
        cm, ct = U.cpu_compress(name)
        assert main == cm and _nonempty(tags) == ct, name
        assert lh.restore(main, tags) == U.data(name), name


def test_restore_on_the_device_with_either_writer():
    """one launch for all streams: with the CABAC writer in the kernel every stream is the kernel's; without it the CABAC streams are
    the host's.  The input comes back either way"""
    res = _compressed()
    assert all(r[2] is None for r in res)
    items = [(r[0], r[1]) for r in res]
    outs, paths = R.restore_batch_device(items, 16, cabac_device=True)
    assert outs == DATAS and paths == [R.PATH_DEVICE] * len(items), dict(zip(U.NAMES, paths))
    outs, paths = R.restore_batch_device(items, 16)
    assert outs == DATAS and paths == [R.PATH_HOST if n in U.CABAC else R.PATH_DEVICE for n in U.NAMES], dict(zip(U.NAMES, paths))


def test_segments_of_one_picture_give_the_files_of_the_whole_stream():
    """the streams in which the carried QP was moved away from SliceQPY, cut after every picture (12 macroblocks)"""
    names = ["i8_cbp0_cavlc_p", "i8_cbp0_cabac"]
    whole = dict(zip(U.NAMES, _compressed()))
    b = lh.compress_batch_handles([U.data(n) for n in names], 16, segment_mbs=12)
    try:
        for i, n in enumerate(names):
            assert b.segments(i) == len(U.REF[n]["picture_sha1"]), n
            main, tags, err = b.result(i)
            assert err is None, (n, err)
            assert main == whole[n][0] and _nonempty(tags) == _nonempty(whole[n][1]), n
            assert lh.restore(main, tags) == U.data(n), n
    finally:
        b.free()
