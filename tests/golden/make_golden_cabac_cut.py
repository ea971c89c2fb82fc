#!/usr/bin/env python3
"""Reference-written files for the CABAC writer of the device restore, small enough to commit: tests/golden/restore_cabac/*.npz.
Each holds what the unmodified reference CLI built by oracle/Makefile (oracle/_ref/h264dec) wrote in compress mode: `main` = out.pip,
`tag_<n>` = out.pip.<n>.  Data only.

cut_<stream>.npz: the stream's first PICTURES pictures (whole NAL units), kept as `input`.  The cli_<stream>.npz set
(make_golden_cli.py) has no I-only CABAC stream: the files of test_cif_I_CABAC_slice.264 are larger than a committed file may be.

concat_<a>+<b>.npz: two streams of one picture size behind each other, a CAVLC and a CABAC one, as ONE stream: the PPS changes the
entropy coder between slices.

own_<stream>.npz: `main` and `tag_<n>` as this project's lh264_compress_batch wrote them (needs a device).  The reference's files of
QCIF_2P_I_allIPCM.264 carry no I_PCM samples, so no restore takes them; ours do, and the I_PCM branch of the CABAC writer (the engine
flushed, 384 raw bytes, the engine restarted) is tested on them without a device.
"""
import glob
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CUTS = [("test_cif_I_CABAC_slice.264", 2)]
CONCATS = [("BA_MW_D.264", "test_qcif_cabac.264")]
OWN = ["QCIF_2P_I_allIPCM.264"]


def first_pictures(data, pictures):
    """the NAL units up to the slice that begins picture `pictures` (first_mb_in_slice = 0: the slice header's first bit is 1)"""
    starts, i = [], 0
    while True:
        i = data.find(b"\x00\x00\x01", i)
        if i < 0:
            break
        starts.append(i - 1 if i > 0 and data[i - 1] == 0 else i)
        i += 3
    seen = 0
    for s in starts:
        p = data.index(b"\x00\x00\x01", s) + 3
        if (data[p] & 31) in (1, 5) and data[p + 1] & 0x80:
            if seen == pictures:
                return data[:s]
            seen += 1
    return data


def reference_files(data):
    """what the reference CLI writes for `data`: {"main": ..., "tag_<n>": ...}"""
    cli = os.path.join(ROOT, "oracle", "_ref", "h264dec")
    tmp = tempfile.mkdtemp(prefix="lh264_cut_")
    src, pip = os.path.join(tmp, "in.264"), os.path.join(tmp, "out.pip")
    open(src, "wb").write(data)
    subprocess.check_call([cli, src, pip], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = {"main": np.frombuffer(open(pip, "rb").read(), dtype=np.uint8)}
    for q in glob.glob(pip + ".*"):
        out["tag_" + q.rsplit(".", 1)[1]] = np.frombuffer(open(q, "rb").read(), dtype=np.uint8)
    return out


def main():
    os.makedirs(os.path.join(HERE, "restore_cabac"), exist_ok=True)
    stream = lambda name: open(os.path.join(HERE, "streams", name), "rb").read()
    for name, pictures in CUTS:
        cut = first_pictures(stream(name), pictures)
        out = reference_files(cut)
        out["input"] = np.frombuffer(cut, dtype=np.uint8)
        path = os.path.join(HERE, "restore_cabac", "cut_" + name + ".npz")
        np.savez_compressed(path, **out)
        print("%s: %d pictures, input %d B, main %d B, %d tags -> %d KB" % (name, pictures, len(cut), len(out["main"]), len(out) - 2,
                                                                              os.path.getsize(path) // 1024))
    for a, b in CONCATS:
        out = reference_files(stream(a) + stream(b))
        path = os.path.join(HERE, "restore_cabac", "concat_%s+%s.npz" % (a, b))
        np.savez_compressed(path, **out)
        print("%s + %s: main %d B, %d tags -> %d KB" % (a, b, len(out["main"]), len(out) - 1, os.path.getsize(path) // 1024))
    import sys
    sys.path.insert(0, ROOT)
    import losslessh264_amd as lh
    for name in OWN:
        (main_s, tags, err), = lh.compress_batch([stream(name)], 1)
        assert err is None, err
        out = {"main": np.frombuffer(main_s, dtype=np.uint8)}
        out.update({"tag_%d" % t: np.frombuffer(b, dtype=np.uint8) for t, b in tags.items()})
        path = os.path.join(HERE, "restore_cabac", "own_" + name + ".npz")
        np.savez_compressed(path, **out)
        print("%s: main %d B, %d tags -> %d KB" % (name, len(main_s), len(tags), os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
