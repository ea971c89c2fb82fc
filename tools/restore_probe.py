"""Restore throughput, host against device: lh264_pip_restore_batch on 16 host threads and lh264_pip_restore_batch_device on the
current device, over batches of copies of one stream (compressed on the device first).  Restored MB/s = output bytes / wall time of
the call; the device call is split into host pass 1 (+ staging), the device stage, the kernel alone (HIP events) and host pass 2.
One JSON line per batch.  --cabac-device passes LH264_RESTORE_CABAC_DEVICE: streams with CABAC slices go through the kernel too
(without it the host restores them beside the kernel, and the "device" figures of such a batch are the host's).

    python tools/restore_probe.py                      # the CAVLC batches of DESIGN.md 4.5
    python tools/restore_probe.py --cabac-device       # its CABAC batches
    python tools/restore_probe.py --stream BA_MW_D.264 --copies 512 --reps 3
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEFAULT = [("BA_MW_D.264", 512), ("BA_MW_D.264", 2048), ("syn720p_allI_4slices.264", 256), ("syn1080p_IP.264", 256)]
DEFAULT_CABAC = [("test_qcif_cabac.264", 512), ("test_qcif_cabac.264", 2048)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream")
    ap.add_argument("--copies", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cabac-device", action="store_true")
    a = ap.parse_args()
    import losslessh264_amd as lh
    R = sys.modules["losslessh264_amd.restore"]
    runs = [(a.stream, a.copies)] if a.stream else (DEFAULT_CABAC if a.cabac_device else DEFAULT)
    for name, copies in runs:
        data = open(os.path.join(ROOT, "tests", "golden", "streams", name), "rb").read()
        (main_s, tags, err), = lh.compress_batch([data], a.threads)
        assert err is None, err
        items = [(main_s, tags)] * copies
        mb = len(data) * copies / 1e6
        rec = {"stream": name, "copies": copies, "restored_mb": round(mb, 2), "cabac_device": a.cabac_device}
        host, dev, split = [], [], []
        outs, paths = R.restore_batch_device(items[:2], a.threads, cabac_device=a.cabac_device)            # warm-up: arena, code object
        for _ in range(a.reps):
            t0 = time.perf_counter()
            o = lh.restore_batch(items, a.threads)
            host.append(time.perf_counter() - t0)
            assert o[0] == data and o[-1] == data
            t0 = time.perf_counter()
            outs, paths = R.restore_batch_device(items, a.threads, cabac_device=a.cabac_device)
            dev.append(time.perf_counter() - t0)
            split.append(R.restore_timing())
            assert all(x == data for x in outs) and (set(paths) == {R.PATH_DEVICE} or (set(paths) == {R.PATH_HOST} and not a.cabac_device))
        b = min(range(a.reps), key=lambda i: dev[i])
        rec.update({"host_s": round(min(host), 4), "host_mb_s": round(mb / min(host), 1),
                    "device_s": round(dev[b], 4), "device_mb_s": round(mb / dev[b], 1),
                    "pass1_ms": round(split[b][0], 1), "device_stage_ms": round(split[b][1], 1), "kernel_ms": round(split[b][2], 1),
                    "pass2_ms": round(split[b][3], 1), "kernel_runs_ms": [round(x[2], 1) for x in split], "device_runs_s": [round(x, 4) for x in dev], "host_runs_s": [round(x, 4) for x in host]})
        print(json.dumps(rec), flush=True)
    R.restore_release()


if __name__ == "__main__":
    main()
