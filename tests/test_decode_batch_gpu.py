"""lh264_decode_batch on the device: the reference's SHA-1 table, the oracle on the streams outside it, NV12 and device output, the
independence of the bytes from every cut of the work, resolution changes inside a stream, local failures, bounded memory and the
two command lines.  Every device step runs once."""
import glob
import hashlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
OK, E_ARG, E_UNSUPPORTED = 0, -2, -4


def _read(name):
    return open(os.path.join(STREAMS, name), "rb").read()


def _table():
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "decoder_sha1.json")))
    return {k: v for k, v in t.items() if not k.startswith("_")}


def _table_streams():
    sha = _table()
    names = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(STREAMS, "*"))) if os.path.basename(p) in sha]
    return names, sha


_cache = {}


def _table_decode():
    """ONE decode_batch over the streams of the table with the default options -> (names, [bytes], [picture lists]); shared by the
    tests that compare other calls with it"""
    if "t" not in _cache:
        import losslessh264_amd as lh
        names, sha = _table_streams()
        b = lh.decode_batch([_read(n) for n in names])
        st = [(b.status(i), b.error(i)) for i in range(len(names))]
        _cache["t"] = (names, [b.data(i) for i in range(len(names))], [b.pictures(i) for i in range(len(names))], st)
        b.free()
    return _cache["t"]


def test_the_references_table():
    names, sha = _table_streams()
    assert len(names) == 36
    names2, datas, pics, st = _table_decode()
    n = 0
    for i, name in enumerate(names):
        assert st[i] == (OK, ""), (name, st[i])
        assert len(pics[i]) > 0 and sum(p[5] for p in pics[i]) == len(datas[i]), name
        off = 0
        for (w, h, fn, idr, o, nb) in pics[i]:
            assert o == off and nb == w * h * 3 // 2, name
            off += nb
        assert hashlib.sha1(datas[i]).hexdigest() == sha[name], name
        n += 1
    assert n == 36


def _oracle_i420(data):
    """the stream's pictures by the oracle, cropped: unfilled reference slots point at the picture itself"""
    import losslessh264_amd as lh
    frames, err, _ = lh.parse_file(data)
    assert err == ""
    pics, out = {}, []
    for f in frames:
        assert f.covered.all()
        dst = O.HostPic(f.mb_w, f.mb_h)
        refs = [pics[r] if r in pics and (pics[r].mb_w, pics[r].mb_h) == (f.mb_w, f.mb_h) else dst for r in f.ref_ids]
        refs += [dst] * (16 - len(refs))
        O.recon_frame(f.mbs, f.coeffs, f.slices, dst, refs, 0 if f.is_ref else O.NO_EXPAND)
        pics[f.id] = dst
        for p in range(3):
            s = 1 if p else 0
            out.append(np.ascontiguousarray(dst.plane(p)[f.crop_y >> s:(f.crop_y + f.crop_h) >> s, f.crop_x >> s:(f.crop_x + f.crop_w) >> s]).tobytes())
    return b"".join(out), len(frames)


OUTSIDE = ["BA_MW_D_IDR_LOST.264", "BA_MW_D_P_LOST.264", "black.264", "syn1080p_IP.264", "syn1080p_IP_8f.264", "syn720p_allI_4slices.264",
           "syn720p_allI_4slices_8f.264", "test_scalinglist_jm.264", "tibby.264", "tibby8x8cavlc.264", "tibbycabac.264"]


def _outside_decode():
    """ONE decode_batch over the 11 streams outside the table"""
    if "o" not in _cache:
        import losslessh264_amd as lh
        b = lh.decode_batch([_read(n) for n in OUTSIDE])
        _cache["o"] = [(b.status(i), b.error(i), b.pictures(i), b.data(i)) for i in range(len(OUTSIDE))]
        b.free()
    return _cache["o"]


def test_all_streams_outside_the_table_take_part():
    sha = _table()
    every = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(STREAMS, "*")))]
    assert sorted(OUTSIDE) == sorted(n for n in every if n not in sha and n != "Error_I_P.264")
    assert len(OUTSIDE) == 11 and len(_outside_decode()) == 11


@pytest.mark.parametrize("name", OUTSIDE)
def test_streams_outside_the_table_against_the_oracle(name):
    """every picture = the oracle's cropped planes.  BA_MW_D_IDR_LOST.264 begins with P pictures whose slices name no reference: the
    oracle predicts nothing there (its fresh picture keeps 128), the decode call puts its 128 picture into the slot the kernel reads"""
    status, error, pictures, got = _outside_decode()[OUTSIDE.index(name)]
    assert (status, error) == (OK, ""), name
    want, n_pics = _oracle_i420(_read(name))
    assert len(pictures) == n_pics, name
    assert len(got) == len(want), name
    if got != want:
        a, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        bad = np.flatnonzero(a != w)
        offs = np.array([p[4] for p in pictures])
        which = sorted(set(int(np.searchsorted(offs, x, side="right")) - 1 for x in bad))
        raise AssertionError("%s: %d bytes differ from the oracle, the first at %d; pictures %s" % (name, len(bad), bad[0], which[:20]))


def test_nv12_and_device_output():
    import torch
    import losslessh264_amd as lh
    names, datas, pics, _ = _table_decode()
    first = names[:8]
    b = lh.decode_batch([_read(n) for n in first], fmt="nv12")
    for i, name in enumerate(first):
        assert b.status(i) == OK and b.pictures(i) == pics[i], name
        got, ref = np.frombuffer(b.data(i), np.uint8), np.frombuffer(datas[i], np.uint8)
        assert len(got) == len(ref)
        for (w, h, _, _, off, nb) in pics[i]:
            y, c = w * h, w * h // 4
            assert np.array_equal(got[off:off + y], ref[off:off + y]), name
            u, v = ref[off + y:off + y + c], ref[off + y + c:off + y + 2 * c]
            assert np.array_equal(got[off + y:off + nb], np.stack([u, v], axis=-1).reshape(-1)), name
    b.free()
    for fmt in ("i420", "nv12"):
        d = lh.decode_batch([_read(n) for n in first], fmt=fmt, device_out=True)
        h = lh.decode_batch([_read(n) for n in first], fmt=fmt) if fmt == "nv12" else None
        for i, name in enumerate(first):
            assert d.status(i) == OK and d.data(i) == b""
            t = d.tensor(i)
            assert t.is_cuda and t.dtype == torch.uint8
            want = datas[i] if fmt == "i420" else h.data(i)
            assert t.cpu().numpy().tobytes() == want, (name, fmt)
        print("device_out tensors are zero-copy views:", getattr(d, "zero_copy", None))
        d.free()
        if h:
            h.free()


def test_the_bytes_do_not_depend_on_the_cuts():
    import losslessh264_amd as lh
    names, datas, pics, _ = _table_decode()
    ins = [_read(n) for n in names]
    for kw in ({"round_pictures": 1}, {"round_pictures": 3}, {"round_pictures": 17}, {"group_mbs": 20000}, {"threads": 1}, {"threads": 16}):
        b = lh.decode_batch(ins, **kw)
        for i, name in enumerate(names):
            assert b.status(i) == OK, (kw, name, b.error(i))
            assert b.pictures(i) == pics[i], (kw, name)
            assert b.data(i) == datas[i], (kw, name)
        b.free()
    # through a sink: the runs of every stream in order, never two calls at once
    got = [[] for _ in names]
    seen = [[] for _ in names]
    busy = threading.Lock()
    overlaps = []

    def sink(stream, first, plist, data):
        if not busy.acquire(False):
            overlaps.append(stream)
            return 1
        try:
            assert first == len(seen[stream])
            assert len(data) == sum(p[5] for p in plist)
            seen[stream].extend(plist)
            got[stream].append(data)
        finally:
            busy.release()
        return 0
    b = lh.decode_batch(ins, sink=sink, round_pictures=5)
    assert not overlaps
    for i, name in enumerate(names):
        assert b.status(i) == OK and b.data(i) == b"", name
        assert seen[i] == pics[i] and b.pictures(i) == pics[i], name
        assert b"".join(got[i]) == datas[i], name
    b.free()


def test_a_stream_that_changes_resolution():
    import losslessh264_amd as lh
    parts = ["BA_MW_D.264", "tibby.264", "Static.264", "BA_MW_D.264"]
    one = b"".join(_read(n) for n in parts)
    sep = lh.decode_batch([_read(n) for n in parts])
    want = b"".join(sep.data(i) for i in range(4))
    want_pics = sum(len(sep.pictures(i)) for i in range(4))
    sizes = [sep.pictures(i)[0][:2] for i in range(4)]
    assert all(sep.status(i) == OK for i in range(4))
    sep.free()
    assert sizes == [(176, 144), (320, 240), (152, 100), (176, 144)] and want_pics == 304
    for kw in ({"round_pictures": 3}, {}):
        b = lh.decode_batch([one], **kw)
        assert (b.status(0), b.error(0)) == (OK, ""), kw
        assert len(b.pictures(0)) == want_pics
        assert b.data(0) == want, kw
        b.free()


def test_failures_stay_local():
    import losslessh264_amd as lh
    names, datas, pics, _ = _table_decode()
    good = {n: (datas[i], pics[i]) for i, n in enumerate(names)}
    ba = _read("BA_MW_D.264")
    err = _read("Error_I_P.264")
    rnd = np.random.default_rng(7).integers(0, 256, 1024, dtype=np.uint8).tobytes()
    cut = _read("SVA_BA2_D.264")
    cut = cut[:len(cut) // 2 + 3]
    # the first picture of the concatenation with a macroblock no slice covers
    frames, _, _ = lh.parse_file(ba + err)
    first_bad = next(i for i, f in enumerate(frames) if not f.covered.all())
    assert first_bad == 100
    assert not lh.parse_file(err)[0][0].covered.all()
    batch = [("g", "BA_MW_D.264"), ("x", err), ("g", "CVFC1_Sony_C.jsv"), ("x", ba + err), ("g", "Static.264"), ("x", b""), ("x", rnd),
             ("g", "SVA_BA2_D.264"), ("x", cut), ("g", "MR1_BT_A.h264")]
    b = lh.decode_batch([_read(v) if k == "g" else v for k, v in batch])
    for i, (k, v) in enumerate(batch):
        if k == "g":
            assert b.status(i) == OK and b.data(i) == good[v][0] and b.pictures(i) == good[v][1], v
    assert b.status(1) == E_UNSUPPORTED and b.pictures(1) == [] and b.data(1) == b"" and "picture 0" in b.error(1)
    assert b.status(3) == E_UNSUPPORTED and "picture 100" in b.error(3), b.error(3)
    assert b.pictures(3) == good["BA_MW_D.264"][1] and b.data(3) == good["BA_MW_D.264"][0]
    assert b.pictures(5) == [] and b.data(5) == b""
    assert b.pictures(6) == [] and b.data(6) == b""
    # the stream cut inside a NAL unit: whatever it delivers in front of the damage is what the whole stream has there
    whole = good["SVA_BA2_D.264"]
    assert b.status(8) == E_UNSUPPORTED and "picture" in b.error(8), (b.status(8), b.error(8))
    k = len(b.pictures(8))
    assert 0 < k < len(whole[1]) and b.pictures(8) == whole[1][:k] and b.data(8) == whole[0][:len(b.data(8))]
    b.free()


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %r)
import losslessh264_amd as lh
K = int(sys.argv[1])
one = open(%r, "rb").read()
h = hashlib.sha1()
count = [0, 0]
def sink(stream, first, pics, data):
    h.update(data); count[0] += len(pics); count[1] += len(data)
    return 0
b = lh.decode_batch([one * K], sink=sink)
dev, pin = lh.decode_arena_bytes()
print(json.dumps({"status": b.status(0), "err": b.error(0), "pictures": len(b.pictures(0)), "seen": count[0], "bytes": count[1], "sha": h.hexdigest(), "device": dev, "pinned": pin}))
"""


def test_memory_follows_the_round_not_the_stream():
    """64 and 256 copies of BA_MW_D.264 as ONE stream through a hashing sink, a fresh process each: the bytes are one copy's repeated,
    and the arena is the same size for both lengths"""
    names, datas, pics, _ = _table_decode()
    one = datas[names.index("BA_MW_D.264")]
    code = _CHILD % (ROOT, os.path.join(STREAMS, "BA_MW_D.264"))
    got = {}
    for K in (64, 256):
        out = subprocess.run([sys.executable, "-c", code, str(K)], check=True, capture_output=True, timeout=900).stdout.decode()
        got[K] = json.loads(out.strip().splitlines()[-1])
        print("K = %d: %s" % (K, got[K]))
        h = hashlib.sha1()
        for _ in range(K):
            h.update(one)
        assert got[K]["status"] == OK and got[K]["err"] == ""
        assert got[K]["pictures"] == got[K]["seen"] == 100 * K and got[K]["bytes"] == len(one) * K
        assert got[K]["sha"] == h.hexdigest()
    assert got[64]["device"] == got[256]["device"] and got[64]["pinned"] == got[256]["pinned"]
    assert 0 < got[64]["device"] < 256 << 20


def test_the_command_lines(tmp_path):
    sha = _table()
    srcs = [os.path.join(STREAMS, n) for n in ("BA_MW_D.264", "CVFC1_Sony_C.jsv")]
    for k, cmd in enumerate(([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"])):
        d = tmp_path / str(k)
        d.mkdir()
        r = subprocess.run(cmd + ["--decode", str(d)] + srcs, capture_output=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
        for s in srcs:
            name = os.path.basename(s)
            assert hashlib.sha1(open(str(d / (name + ".yuv")), "rb").read()).hexdigest() == sha[name], (cmd, name)
    # NV12 through the console application: the same luma, the chroma interleaved
    d = tmp_path / "nv12"
    d.mkdir()
    r = subprocess.run([os.path.join(ROOT, "losslessh264_amd", "lh264dec"), "--decode", "--nv12", str(d), srcs[0]], capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()
    nv = np.fromfile(str(d / "BA_MW_D.264.yuv"), np.uint8).reshape(-1, 176 * 144 * 3 // 2)
    i4 = np.fromfile(str(tmp_path / "0" / "BA_MW_D.264.yuv"), np.uint8).reshape(-1, 176 * 144 * 3 // 2)
    y, c = 176 * 144, 176 * 144 // 4
    assert np.array_equal(nv[:, :y], i4[:, :y])
    assert np.array_equal(nv[:, y:], np.stack([i4[:, y:y + c], i4[:, y + c:]], axis=-1).reshape(len(i4), -1))
