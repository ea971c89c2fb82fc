"""The CABAC writer of the device restore on the device (lh264_pip_restore_batch_device_opts with LH264_RESTORE_CABAC_DEVICE,
csrc/lh264_restore.hip restore_cabac_kernel): every item as lh264_pip_restore_batch gives it, CABAC streams restored by the kernel."""
import sys

import pytest

import losslessh264_amd as lh
import restore_cabac_fixtures as FX
import restore_cases as RC

pytestmark = pytest.mark.gpu
R = sys.modules["losslessh264_amd.restore"]


def DEV(items, threads=0, out_cap=None, statuses=False):
    return R.restore_batch_device(items, threads, out_cap, statuses, cabac_device=True)


_compressed = {}


def _compress(names, datas=None):
    todo = [n for n in names if n not in _compressed]
    if todo:
        for n, r in zip(todo, lh.compress_batch([datas[n] if datas else RC.data(n) for n in todo], 16)):
            _compressed[n] = r
    return [_compressed[n] for n in names]


def test_device_restores_our_own_cabac_output():
    names = [n for n in RC.SWEEP + [n for n in RC.SYNTH if n not in RC.SWEEP] if RC.is_cabac(n)]
    assert len(names) >= 3, names
    res = _compress(names)
    for n, (_, _, err) in zip(names, res):
        assert err is None, (n, err)
    outs, paths = DEV([(m, t) for m, t, _ in res], 16)
    for n, o, p in zip(names, outs, paths):
        assert o == RC.data(n), n
        assert p == R.PATH_DEVICE, (n, p)


def test_device_matches_the_host_batch_on_the_cabac_reference_files():
    """the case of tests/test_restore_cabac.py on the device: every CABAC cli fixture, and the reference-written two-picture cut that
    stands for test_cif_I_CABAC_slice.264 (the cli set cannot hold its files: they are larger than a committed file may be; the whole
    stream goes through the kernel in test_device_restores_our_own_cabac_output).  What the host refuses, the kernel stops at."""
    names = [n for n in RC.CLI if RC.is_cabac(n)]
    assert {"test_qcif_cabac.264", "test_cif_P_CABAC_slice.264"} <= set(names)
    main, tags, want = FX.load(FX.I_CUT)
    items = [RC.cli_fixture(n) for n in names] + [(main, tags)]
    paths = RC.check_same(items, DEV)
    restorable = [st == 0 for st, _, _ in RC.host_results(items)]
    assert restorable.count(True) >= 4 and restorable[-1]
    assert paths == [R.PATH_DEVICE if ok else R.PATH_FALLBACK for ok in restorable], dict(zip(names + [FX.I_CUT], paths))
    outs, _ = DEV(items[-1:], 1)
    assert outs == [want]


def test_device_both_writers_in_one_stream():
    """a CAVLC stream and a CABAC stream of one picture size behind each other: the PPS changes the entropy coder between slices"""
    both = RC.data("BA_MW_D.264") + RC.data("test_qcif_cabac.264")
    (main, tags, err), = _compress(["BA_MW_D+test_qcif_cabac"], {"BA_MW_D+test_qcif_cabac": both})
    assert err is None, err
    outs, paths = DEV([(main, tags)], 16)
    assert outs == [both] and paths == [R.PATH_DEVICE]
    # without the flag the stream is the host's: one CABAC slice is enough
    outs, paths = R.restore_batch_device([(main, tags)], 16)
    assert outs == [both] and paths == [R.PATH_HOST]


def test_device_small_cabac_batch_and_the_default_routing():
    """more chains than one wave per SIMD... of one launch; longest-first ordering and per-stream work memory; then the same batch
    without the flag: the default routing is the host's, as before"""
    (main, tags, err), = _compress(["test_qcif_cabac.264"])
    assert err is None
    want = RC.data("test_qcif_cabac.264")
    outs, paths = DEV([(main, tags)] * 64, 16)
    assert all(o == want for o in outs)
    assert set(paths) == {R.PATH_DEVICE}
    outs, paths = R.restore_batch_device([(main, tags)] * 64, 16)
    assert all(o == want for o in outs)
    assert set(paths) == {R.PATH_HOST}
