"""The device restore's C ABI without a device (lh264_pip_restore_batch_device), and the kernel's code stepped on the host
(lh264_debug_restore_cpu: the same plan, capacities and chain as the kernel) against the host restore."""
import ctypes as C
import sys

import pytest

import losslessh264_amd as lh
import restore_cases as RC

R = sys.modules["losslessh264_amd.restore"]
CPU = R.restore_batch_cpu_check


def test_no_device_is_an_error_and_leaves_the_items():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = lh.lib()
    assert L.lh264_device_count() <= 0
    main, tags = RC.cli_fixture("SVA_BA2_D.264")
    arr, keep = R._restore_items([(main, tags)], None)
    arr[0].status, arr[0].out_len = 77, 99
    paths = (C.c_int32 * 1)(55)
    assert L.lh264_pip_restore_batch_device(C.byref(arr), 1, 1, paths) == -1            # LH264_E_NODEVICE
    assert (arr[0].status, arr[0].out_len, paths[0]) == (77, 99, 55)
    with pytest.raises(RuntimeError):
        lh.restore_batch_device([(main, tags)])


def test_kernel_chain_on_the_host_restores_the_reference_files():
    """every cli fixture: status, size and bytes as lh264_pip_restore_batch; CAVLC streams on the kernel's path, CABAC on the host's"""
    items = [RC.cli_fixture(n) for n in RC.CLI]
    paths = RC.check_same(items, CPU)
    for n, p in zip(RC.CLI, paths):
        assert p == (R.PATH_HOST if RC.is_cabac(n) else R.PATH_DEVICE), n
    assert paths.count(R.PATH_DEVICE) >= 15


def test_kernel_chain_on_the_host_small_output_buffer():
    """LH264_E_ARG with out_len = the size needed, as the host batch reports it"""
    items = [RC.cli_fixture("SVA_BA2_D.264"), RC.cli_fixture("test_qcif_cabac.264")]
    RC.check_same(items, CPU, out_cap=1000)


def test_kernel_chain_on_the_host_damaged_input():
    main, tags = RC.cli_fixture("SVA_BA1_B.264")
    cases = RC.damaged(main, tags)
    paths = RC.check_same([(m, t) for _, m, t in cases], CPU, allowed_paths=(R.PATH_DEVICE, R.PATH_FALLBACK))
    assert R.PATH_FALLBACK in paths and R.PATH_DEVICE in paths


@pytest.mark.parametrize("var,value", [("LH264_RESTORE_SLOTS", "64"), ("LH264_RESTORE_POOL", "600"), ("LH264_RESTORE_OUT_CAP", "300")])
def test_kernel_chain_on_the_host_capacity_overflow_falls_back(monkeypatch, var, value):
    monkeypatch.setenv(var, value)
    items = [RC.cli_fixture("SVA_BA2_D.264"), RC.cli_fixture("SVA_NL2_E.264")]
    paths = RC.check_same(items, CPU)
    assert paths == [R.PATH_FALLBACK, R.PATH_FALLBACK]
