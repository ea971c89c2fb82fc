"""Inputs for the device restore tests (tests/test_restore_device.py, tests/test_restore_device_gpu.py): the reference-written
file sets (tests/golden/cli_*.npz), the damaged variants of one of them, and the comparison with the host batch restore."""
import glob
import json
import os

import numpy as np

import golden_io
import losslessh264_amd as lh

STREAMS = os.path.join(golden_io.GOLDEN_DIR, "streams")
CLI = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(golden_io.GOLDEN_DIR, "cli_*.npz")))
SWEEP = sorted(json.load(open(os.path.join(golden_io.GOLDEN_DIR, "ref_sweep.json"))))
SYNTH = ["syn720p_allI_4slices.264", "syn720p_allI_4slices_8f.264", "syn1080p_IP.264", "syn1080p_IP_8f.264"]
TAG_PCM = 70


def data(name):
    return open(os.path.join(STREAMS, name), "rb").read()


def cli_fixture(name):
    z = np.load(os.path.join(golden_io.GOLDEN_DIR, "cli_" + name + ".npz"))
    return z["main"].tobytes(), {int(k[4:]): z[k].tobytes() for k in z.files if k.startswith("tag_")}


def is_cabac(name):
    """from the slice flags, as test_pip_container._is_cabac"""
    frames, _ = lh.parse_stream(data(name))
    return any(int(f.slice_syn[0, 3]) & 1 for f in frames)


def damaged(main, tags, seed=5):
    """truncated tag streams, flipped bytes, a missing tag: (label, main, tags)"""
    rng = np.random.default_rng(seed)
    out = []
    big = sorted(t for t in tags if t not in (69, TAG_PCM) and len(tags[t]) > 16)
    for t in big[:4]:
        for frac in (0.0, 0.5, 0.9):
            t2 = dict(tags)
            t2[t] = tags[t][:int(len(tags[t]) * frac)]
            out.append(("trunc %d %.1f" % (t, frac), main, t2))
        for _ in range(2):
            b = bytearray(tags[t])
            i = int(rng.integers(len(b)))
            b[i] ^= 1 << int(rng.integers(8))
            t2 = dict(tags)
            t2[t] = bytes(b)
            out.append(("flip %d@%d" % (t, i), main, t2))
    for t in big[:3] + [69]:
        t2 = dict(tags)
        del t2[t]
        out.append(("missing %d" % t, main, t2))
    return out


def host_results(items, out_cap=None):
    """(status, out_len, bytes or None) per item from lh264_pip_restore_batch"""
    import ctypes as C
    R = __import__("sys").modules["losslessh264_amd.restore"]
    arr, keep = R._restore_items(items, out_cap)
    assert lh.lib().lh264_pip_restore_batch(C.byref(arr), len(items), 16) == 0
    return [(arr[i].status, arr[i].out_len, keep[i][2].raw[:arr[i].out_len] if arr[i].status == 0 else None) for i in range(len(items))]


def check_same(items, fn, out_cap=None, allowed_paths=None):
    """fn (items, threads, out_cap, statuses=True) gives what the host batch gives, item by item; returns the paths"""
    want = host_results(items, out_cap)
    outs, paths, st = fn(items, 16, out_cap, statuses=True)
    for i, ((ws, wl, wb), o, (s, ln), p) in enumerate(zip(want, outs, st, paths)):
        assert (s, ln) == (ws, wl), "item %d: status/out_len %s, the host batch %s" % (i, (s, ln), (ws, wl))
        assert o == wb, "item %d: bytes differ" % i
        if allowed_paths is not None:
            assert p in allowed_paths, "item %d: path %d" % (i, p)
    return paths
