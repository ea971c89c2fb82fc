"""The restore direction on the device (lh264_pip_restore_batch_device, csrc/lh264_restore.hip): every item as
lh264_pip_restore_batch gives it, CAVLC streams restored by the kernel."""
import sys

import pytest

import losslessh264_amd as lh
import restore_cases as RC

pytestmark = pytest.mark.gpu
R = sys.modules["losslessh264_amd.restore"]
DEV = R.restore_batch_device

_compressed = {}


def _compress(names):
    todo = [n for n in names if n not in _compressed]
    if todo:
        for n, r in zip(todo, lh.compress_batch([RC.data(n) for n in todo], 16)):
            _compressed[n] = r
    return [_compressed[n] for n in names]


def test_device_restores_our_own_output():
    """the 44 sweep streams and the 4 synthetic 720p / 1080p ones, compressed on the device: the 47 that compress come back byte for
    byte, CAVLC ones (I_PCM, 8x8 transform, multi-slice, constrained intra, multi-reference among them) through the kernel"""
    names = RC.SWEEP + [n for n in RC.SYNTH if n not in RC.SWEEP]
    res = _compress(names)
    ok = [(n, main, tags) for n, (main, tags, err) in zip(names, res) if err is None]
    assert len(ok) == 47, sorted(set(names) - {n for n, _, _ in ok})
    outs, paths = DEV([(m, t) for _, m, t in ok], 16)
    for (n, _, _), o, p in zip(ok, outs, paths):
        assert o == RC.data(n), n
        assert p == (R.PATH_HOST if RC.is_cabac(n) else R.PATH_DEVICE), (n, p)
    dev = {n for (n, _, _), p in zip(ok, paths) if p == R.PATH_DEVICE}
    assert {"CVPCMNL1_SVA_C.264", "tibby8x8cavlc.264", "syn720p_allI_4slices.264", "SVA_CL1_E.264", "MR1_BT_A.h264"} <= dev


def test_device_matches_the_host_batch_on_the_reference_files():
    items = [RC.cli_fixture(n) for n in RC.CLI]
    paths = RC.check_same(items, DEV)
    for n, p in zip(RC.CLI, paths):
        assert p == (R.PATH_HOST if RC.is_cabac(n) else R.PATH_DEVICE), n
    RC.check_same(items[:6], DEV, out_cap=1000)


def test_device_bench_sized_batch():
    (main, tags, err), = _compress(["BA_MW_D.264"])
    assert err is None
    outs, paths = DEV([(main, tags)] * 512, 16)
    want = RC.data("BA_MW_D.264")
    assert all(o == want for o in outs)
    assert set(paths) == {R.PATH_DEVICE}


def test_device_mixed_sizes_in_one_call():
    """QCIF, CIF, 720p and 1080p streams in one launch (per-stream sizing); the 8-picture 1080p stream once"""
    names = ["BA_MW_D.264", "tibby8x8cavlc.264", "syn720p_allI_4slices.264", "syn1080p_IP.264", "syn1080p_IP_8f.264", "test_qcif_cabac.264"]
    res = _compress(names)
    reps = [3, 2, 2, 2, 1, 1]
    items, want = [], []
    for n, (main, tags, err), k in zip(names, res, reps):
        assert err is None, n
        items += [(main, tags)] * k
        want += [n] * k
    outs, paths = DEV(items, 16)
    for n, o, p in zip(want, outs, paths):
        assert o == RC.data(n), n
        assert p == (R.PATH_HOST if n == "test_qcif_cabac.264" else R.PATH_DEVICE), n


def test_device_damaged_input_is_reported_as_the_host_reports_it():
    main, tags = RC.cli_fixture("SVA_BA1_B.264")
    cases = [(m, t) for _, m, t in RC.damaged(main, tags)]
    (pm, pt, err), = _compress(["CVPCMNL1_SVA_C.264"])
    assert err is None and RC.TAG_PCM in pt
    cases.append((pm, {t: b for t, b in pt.items() if t != RC.TAG_PCM}))        # I_PCM without its samples
    paths = RC.check_same(cases, DEV, allowed_paths=(R.PATH_DEVICE, R.PATH_FALLBACK))
    assert paths[-1] == R.PATH_FALLBACK and R.PATH_DEVICE in paths


@pytest.mark.parametrize("var,value", [("LH264_RESTORE_SLOTS", "64"), ("LH264_RESTORE_POOL", "600"), ("LH264_RESTORE_OUT_CAP", "300")])
def test_device_capacity_overflow_falls_back(monkeypatch, var, value):
    monkeypatch.setenv(var, value)
    items = [RC.cli_fixture("SVA_BA2_D.264"), RC.cli_fixture("SVA_NL2_E.264"), RC.cli_fixture("test_qcif_cabac.264")]
    paths = RC.check_same(items, DEV)
    assert paths == [R.PATH_FALLBACK, R.PATH_FALLBACK, R.PATH_HOST]
