"""slice_parse_kernel / slice_parse_cabac_kernel beside the host: `copies` copies of a stream concatenated into one Annex-B stream go
through lh264_debug_slice_parse_opts - the deferred header walk, then every slice (CAVLC through csrc/lh264_slice.h, CABAC through
csrc/lh264_slice_cabac.h) on the host threads and through the kernels - and through lh264_parse_batch_discard as the host yardstick.
The call's seconds include the header walk, the arena, both copies and the guard check; the kernels' own time is what
`rocprofv3 --kernel-trace --stats -- python tools/slice_parse_probe.py ... --device-only` reports for them.  A CABAC stream is
recognised by its slices and reported with "kernel": "slice_parse_cabac_kernel".

  python tools/slice_parse_probe.py 16 [stream] [--device-only]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from losslessh264_amd import parse as PA  # noqa: E402
from losslessh264_amd import slice_parse as SP  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    copies = int(args[0]) if args else 16
    path = args[1] if len(args) > 1 else os.path.join(ROOT, "tests", "golden", "streams", "BA_MW_D.264")
    one = open(path, "rb").read()
    data = one * copies
    marks = SP.parse_file_plain(one, deferred=True, cabac=True).deferred_cabac
    n_cabac, n_all = sum(sum(m) for m in marks), sum(len(m) for m in marks)
    kernels = (["slice_parse_kernel"] if n_all > n_cabac else []) + (["slice_parse_cabac_kernel"] if n_cabac else [])
    row = dict(stream=os.path.basename(path), copies=copies, bytes=len(data), kernel="+".join(kernels), cabac_slices=n_cabac * copies)
    runs = [("device", True)] if "--device-only" in sys.argv else [("host_form", False), ("device", True)]
    for name, dev in runs:
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            pics, guards, err = SP.slice_parse(data, on_device=dev, threads=16, cabac=True)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        assert guards and not err
        row["slices"] = sum(p.n_deferred for p in pics)
        row["mbs"] = sum(int(p.slices["n_mbs"].sum()) for p in pics)
        row[name + "_call_s"] = round(best, 4)
    if "--device-only" not in sys.argv:
        dt, n = PA.parse_batch_time([one] * copies, threads=16, keep=False)
        row["parse_batch_discard_s"] = round(dt, 4)
        row["parse_batch_discard_MBps"] = round(len(data) / dt / 1e6, 1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
