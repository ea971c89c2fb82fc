"""The CABAC writer of the device restore without a device: the kernel's code stepped on the host (lh264_debug_restore_cpu_opts with
LH264_RESTORE_CABAC_DEVICE: the plan, capacities, chain and kernel instance of lh264_pip_restore_batch_device_opts) against the host
restore, and the options form of the call."""
import ctypes as C
import sys

import losslessh264_amd as lh
import restore_cabac_fixtures as FX
import restore_cases as RC

R = sys.modules["losslessh264_amd.restore"]
L = sys.modules["losslessh264_amd._lib"]
E_ARG = -2


def CPU(items, threads=0, out_cap=None, statuses=False):
    return R.restore_batch_cpu_check(items, threads, out_cap, statuses, cabac_device=True)


CABAC = [n for n in RC.CLI if RC.is_cabac(n)]
def _has_p_slice(data):
    return any((f.slices["slice_type"] == 0).any() for f in lh.parse_stream(data)[0])      # 0 = P, 2 = I


def test_cabac_reference_files_on_the_kernel_chain():
    """every CABAC cli fixture and the I-only cut: status, size and bytes as lh264_pip_restore_batch, on the kernel's path"""
    assert {"test_qcif_cabac.264", "test_cif_P_CABAC_slice.264"} <= set(CABAC)
    assert any(_has_p_slice(RC.data(n)) for n in CABAC)
    main, tags, want = FX.load(FX.I_CUT)
    frames = lh.parse_stream(want)[0]
    assert len(frames) == 2 and all(int(f.slice_syn[0, 3]) & 1 for f in frames) and not _has_p_slice(want)
    items = [RC.cli_fixture(n) for n in CABAC] + [(main, tags)]
    paths = RC.check_same(items, CPU)
    # (QCIF_2P_I_allIPCM.264 as the reference wrote it has no I_PCM samples: the host refuses it, and so the kernel stops)
    restorable = [st == 0 for st, _, _ in RC.host_results(items)]
    assert restorable.count(True) >= 4 and restorable[-1]
    assert paths == [R.PATH_DEVICE if ok else R.PATH_FALLBACK for ok in restorable], dict(zip(CABAC + [FX.I_CUT], paths))
    outs, _ = CPU(items[-1:], 1)
    assert outs == [want]


def test_cavlc_stream_beside_cabac_streams_in_one_call():
    """the instance with both writers restores a CAVLC stream too (its longer writer state included)"""
    names = ["test_qcif_cabac.264", "SVA_BA2_D.264", "test_cif_P_CABAC_slice.264"]
    assert not RC.is_cabac("SVA_BA2_D.264")
    paths = RC.check_same([RC.cli_fixture(n) for n in names], CPU)
    assert paths == [R.PATH_DEVICE] * 3


def test_both_writers_in_one_stream():
    """BA_MW_D.264 (CAVLC) and test_qcif_cabac.264 behind each other as one stream, as the reference wrote it: the chain changes its
    writer between slices, over one writer state; without the flag one CABAC slice makes the stream the host's"""
    both = RC.data("BA_MW_D.264") + RC.data("test_qcif_cabac.264")
    main, tags, _ = FX.load(FX.CONCAT)
    outs, paths = CPU([(main, tags)], 1)
    assert outs == [both] and paths == [R.PATH_DEVICE]
    outs, paths = R.restore_batch_cpu_check([(main, tags)], 1)
    assert outs == [both] and paths == [R.PATH_HOST]


def test_cabac_ipcm_macroblocks():
    """I_PCM in a CABAC slice, on the files lh264_compress_batch wrote of QCIF_2P_I_allIPCM.264 (the reference's carry no samples): the
    terminating bin flushes the engine, the 384 samples follow as bytes, the engine starts afresh behind them with the contexts kept"""
    name = "QCIF_2P_I_allIPCM.264"
    assert RC.is_cabac(name)
    main, tags, _ = FX.load(FX.OWN_IPCM)
    assert len(tags[RC.TAG_PCM]) == 99 * 384                 # a whole QCIF picture of I_PCM macroblocks
    paths = RC.check_same([(main, tags)], CPU)
    assert paths == [R.PATH_DEVICE]
    outs, _ = CPU([(main, tags)], 1)
    assert outs == [RC.data(name)]
    short = dict(tags)
    short[RC.TAG_PCM] = tags[RC.TAG_PCM][:98 * 384 + 383]    # the last macroblock's samples are incomplete: the chain stops in front of them
    assert RC.check_same([(main, short)], CPU) == [R.PATH_FALLBACK]


def _call(fn, items, struct_bytes, flags):
    arr, keep = R._restore_items(items, None)
    paths = (C.c_int32 * len(items))(*([55] * len(items)))
    opts = L.RestoreOpts(struct_bytes, 16, flags)
    rc = fn(C.byref(arr), len(items), C.byref(opts), paths)
    return rc, list(paths), [keep[i][2].raw[:arr[i].out_len] if arr[i].status == 0 else None for i in range(len(items))]


def test_flag_off_and_bad_options():
    lib = lh.lib()
    names = CABAC + ["SVA_BA2_D.264"]
    items = [RC.cli_fixture(n) for n in names]
    size = C.sizeof(L.RestoreOpts)
    assert size == 12
    rc, paths, outs = _call(lib.lh264_debug_restore_cpu_opts, items, size, 0)
    assert rc == 0 and paths == [R.PATH_HOST] * len(CABAC) + [R.PATH_DEVICE]
    want = [b for _, _, b in RC.host_results(items)]
    assert outs == want
    # the call without options is the call with zeroed flags
    arr, keep = R._restore_items(items, None)
    p2 = (C.c_int32 * len(items))()
    assert lib.lh264_debug_restore_cpu(C.byref(arr), len(items), 16, p2) == 0
    assert list(p2) == paths and [keep[i][2].raw[:arr[i].out_len] if arr[i].status == 0 else None for i in range(len(items))] == want
    for fn in (lib.lh264_debug_restore_cpu_opts, lib.lh264_pip_restore_batch_device_opts):      # before the device is looked at
        assert _call(fn, items, size, 2)[:2] == (E_ARG, [55] * len(items))
        assert _call(fn, items, size, 0x80000001)[0] == E_ARG
        assert _call(fn, items, size + 4, L.RESTORE_CABAC_DEVICE)[0] == E_ARG
        assert _call(fn, items, 0, 0)[0] == E_ARG


def test_cabac_damaged_input_is_reported_as_the_host_reports_it():
    main, tags = RC.cli_fixture("test_qcif_cabac.264")
    cases = RC.damaged(main, tags)
    paths = RC.check_same([(m, t) for _, m, t in cases], CPU, allowed_paths=(R.PATH_DEVICE, R.PATH_FALLBACK))
    assert R.PATH_FALLBACK in paths


def test_cabac_output_overflow_falls_back(monkeypatch):
    monkeypatch.setenv("LH264_RESTORE_OUT_CAP", "300")
    paths = RC.check_same([RC.cli_fixture("test_qcif_cabac.264")], CPU)
    assert paths == [R.PATH_FALLBACK]
