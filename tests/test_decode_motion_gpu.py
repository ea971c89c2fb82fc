"""Motion fields on the device (lh264_decode_batch_ex4): decode_pack_motion_kernel over the directed record tables of
tests/test_decode_motion.py, and the call - every mode of it - against tests/motion_model.py over the host front end's records; the
pictures of a call with fields against the same call without them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import motion_model as MM
from test_decode_motion import GUARD, check, directed_jobs, layout

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# QCIF, 300 x 168 (a window that is not the coded picture), one macroblock, CABAC, 1080p (two chunks a row), back -1 in front of a lost
# IDR, a stream that stops at its first picture, back up to 15
STREAMS = ["streams/BA_MW_D.264", "streams/CVFC1_Sony_C.jsv", "cabac_edge/cabac_skip.264", "streams/test_qcif_cabac.264", "streams/syn1080p_IP_8f.264",
           "streams/BA_MW_D_IDR_LOST.264", "streams/Error_I_P.264", "edge/nref_2_3_15.264"]
VARIANTS = {
    "rounds": dict(round_pictures=1, group_mbs=300),
    "parse_device": dict(parse="device"),
    "parse_device_cabac": dict(parse="device+cabac"),
    "sized_float": dict(size=(224, 224), colour="rgb24", dtype="float16"),
}

_cache = {}


def _read(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _datas():
    if "datas" not in _cache:
        _cache["datas"] = [_read(n) for n in STREAMS]
    return _cache["datas"]


def _result(b, n, data=None, fields=True):
    """what a call delivered, per stream: status, text, picture records, picture bytes, indices, and with fields the geometry and the
    two buffers' bytes"""
    out = []
    for i in range(n):
        r = dict(status=b.status(i), error=b.error(i), pics=b.pictures(i), data=data[i] if data is not None else b.data(i), idx=b.picture_indices(i))
        if fields:
            mot, mbi = b._field_buffers(i)
            if b.device_out:
                mot, mbi = mot.cpu().numpy(), mbi.cpu().numpy()
            r.update(geo=b.motion_geometry(i), mot=mot.tobytes(), mbi=mbi.tobytes())
        out.append(r)
    b.free()
    return out


def _call(motion, **kw):
    """ONE decode_batch over STREAMS per set of arguments, shared by the tests"""
    key = (motion,) + tuple(sorted(kw.items()))
    if key not in _cache:
        import losslessh264_amd as lh
        _cache[key] = _result(lh.decode_batch(_datas(), motion=motion, **kw), len(STREAMS), fields=motion)
    return _cache[key]


def _frames(i, conceal=None):
    if ("frames", i, conceal) not in _cache:
        import losslessh264_amd as lh
        _cache[("frames", i, conceal)] = lh.parse_file(_datas()[i], conceal=conceal)[0]
    return _cache[("frames", i, conceal)]


def _model(i):
    """motion_model over stream i's records, per picture of the front end's list"""
    if ("model", i) not in _cache:
        _cache[("model", i)] = MM.stream_fields(_frames(i))
    return _cache[("model", i)]


def _expected(frames, fields, idx):
    """the two buffers and the geometry of a stream that delivers the pictures idx of `frames`"""
    mot = b"".join(fields[k][0].astype("<i2").tobytes() for k in idx)
    mbi = b"".join(fields[k][1].tobytes() for k in idx)
    geo, mo, io = [], 0, 0
    for k in idx:
        f = frames[k]
        geo.append((f.mb_w, f.mb_h, f.crop_x, f.crop_y, mo, io))
        mo += 96 * f.mb_w * f.mb_h
        io += 8 * f.mb_w * f.mb_h
    return mot, mbi, geo


def _fields_are_the_models(got, what):
    for i, name in enumerate(STREAMS):
        mot, mbi, geo = _expected(_frames(i), _model(i), got[i]["idx"])
        assert got[i]["geo"] == geo, (what, name)
        assert len(got[i]["mbi"]) == len(mbi) and got[i]["mbi"] == mbi, (what, name)
        assert len(got[i]["mot"]) == len(mot), (what, name)
        if got[i]["mot"] != mot:
            a, b = np.frombuffer(got[i]["mot"], "<i2"), np.frombuffer(mot, "<i2")
            k = int(np.flatnonzero(a != b)[0])
            raise AssertionError((what, name, "first difference at cell", k, int(a[k]), int(b[k]), int((a != b).sum())))


def _pictures_are_the_same(got, base, what):
    for i, name in enumerate(STREAMS):
        for key in ("status", "error", "pics", "idx"):
            assert got[i][key] == base[i][key], (what, name, key)
        assert got[i]["data"] == base[i]["data"], (what, name)


# ---- 1: the production kernel over the directed tables -----------------------------------------------------------------------------------
def test_production_kernel_on_directed_tables():
    """lh264_debug_motion_dev - decode_pack_motion_kernel - over the directed tables of tests/test_decode_motion.py in one launch: both
    blocks of every job are the model's and the 0xA5 around and between them is intact"""
    import torch
    from losslessh264_amd import _lib as L
    lib = L.lib()
    jobs = directed_jobs()
    places, nbytes = layout(jobs)
    rec_at, sl_at, at, sat = [], [], 0, 0
    for j in jobs:
        rec_at.append(at)
        sl_at.append(sat)
        at += j.mbs.nbytes
        sat += j.slices.nbytes
    recs = torch.from_numpy(np.concatenate([j.mbs.view(np.uint8).reshape(-1) for j in jobs])).cuda()
    slices = torch.from_numpy(np.concatenate([j.slices.view(np.uint8).reshape(-1) for j in jobs] + [np.zeros(8, np.uint8)])).cuda()
    buf = torch.full((nbytes,), GUARD, dtype=torch.uint8, device="cuda")
    assert recs.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    table = (L.MotionJob * len(jobs))()
    for t, j, (m, i), ra, sa in zip(table, jobs, places, rec_at, sl_at):
        t.mbs, t.slices = recs.data_ptr() + ra, slices.data_ptr() + sa if len(j.slices) else None
        t.motion, t.info = buf.data_ptr() + m, buf.data_ptr() + i
        t.mb_w, t.mb_h, t.n_slices, t.reserved = j.mb_w, j.mb_h, len(j.slices), 0
        for k in range(16):
            t.back[k] = j.back[k]
    assert lib.lh264_debug_motion_dev(table, len(jobs)) == 0
    check(jobs, places, buf.cpu().numpy())


# ---- 2: the call ---------------------------------------------------------------------------------------------------------------------------
def test_fields_are_the_models_and_the_pictures_unchanged():
    """decode_batch (motion=True) over STREAMS in host mode: per delivered picture both blocks are the model's over the front end's
    records, tight one behind the other, the geometry names the coded picture and the window's place in it; statuses, texts, picture
    records, indices and picture bytes are those of the call without motion"""
    got, base = _call(True), _call(False)
    _fields_are_the_models(got, "host")
    _pictures_are_the_same(got, base, "host")
    assert sum(len(r["pics"]) for r in got) > 300 and got[STREAMS.index("streams/Error_I_P.264")]["status"] != 0
    i = STREAMS.index("streams/CVFC1_Sony_C.jsv")
    f = _frames(i)[0]
    assert (f.crop_w, f.crop_h) != (16 * f.mb_w, 16 * f.mb_h) and got[i]["pics"][0][:2] == (f.crop_w, f.crop_h) and got[i]["geo"][0][:2] == (f.mb_w, f.mb_h)
    i = STREAMS.index("edge/nref_2_3_15.264")
    assert max(int(np.frombuffer(got[i]["mot"], "<i2", 16 * g[0] * g[1], g[4] + 64 * g[0] * g[1]).max()) for g in got[i]["geo"]) == 15      # plane 2
    lost = np.frombuffer(got[STREAMS.index("streams/BA_MW_D_IDR_LOST.264")]["mot"], "<i2")[:48 * 99].reshape(3, 36, 44)
    assert (lost[2] == -1).all()      # the stream's first picture: P macroblocks with nothing to predict from


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_same_fields_in_every_variant(variant):
    """round_pictures=1 with a small group_mbs, both device parse routes, and a sized float RGB call: the field bytes are those of the
    plain call, and the pictures those of the same call without motion - each is unchanged by the other"""
    kw = VARIANTS[variant]
    got = _call(True, **kw)
    plain = _call(True)
    for i, name in enumerate(STREAMS):
        for key in ("geo", "mot", "mbi"):
            assert got[i][key] == plain[i][key], (variant, name, key)
    _pictures_are_the_same(got, _call(False, **kw), variant)
    if variant.startswith("parse_device"):
        import losslessh264_amd as lh
        b = lh.decode_batch(_datas()[:1], motion=True, **kw)
        assert b.parse_path(0) == "device"
        b.free()


def test_the_same_fields_on_the_device():
    """device_out=True: the fields through the torch views, through motion_copy and through the frames views are the host call's; the
    picture bytes are those of the device call without motion"""
    import torch
    import losslessh264_amd as lh
    plain = _call(True)
    b = lh.decode_batch(_datas(), motion=True, device_out=True)
    for i, name in enumerate(STREAMS):
        views = b.motion(i), b.mb_info(i)
        assert len(views[0]) == len(views[1]) == len(plain[i]["pics"]), name
        assert all(v.is_cuda and v.dtype == torch.int16 for v in views[0]) and all(v.is_cuda and v.dtype == torch.uint8 for v in views[1])
        assert b"".join(v.cpu().numpy().tobytes() for v in views[0]) == plain[i]["mot"], name
        assert b"".join(v.cpu().numpy().tobytes() for v in views[1]) == plain[i]["mbi"], name
        mot, mbi = b.motion_copy(i)
        assert mot.cpu().numpy().tobytes() == plain[i]["mot"] and mbi.cpu().numpy().tobytes() == plain[i]["mbi"], name
        assert b.motion_geometry(i) == plain[i]["geo"], name
        assert b.tensor(i).cpu().numpy().tobytes() == plain[i]["data"], name
    i = STREAMS.index("streams/BA_MW_D.264")
    mf, inf = b.motion_frames(i), b.mb_info_frames(i)
    assert tuple(mf.shape) == (len(plain[i]["pics"]), 3, 36, 44) and tuple(inf.shape) == (len(plain[i]["pics"]), 8, 9, 11)
    assert mf.cpu().numpy().tobytes() == plain[i]["mot"] and inf.cpu().numpy().tobytes() == plain[i]["mbi"]
    i = STREAMS.index("cabac_edge/cabac_skip.264")      # 40 x 30 macroblocks, then 1 x 1
    with pytest.raises(ValueError):
        b.motion_frames(i)
    b.free()
    h = lh.decode_batch(_datas()[:1], motion=True)
    assert isinstance(h.motion_frames(0), np.ndarray) and h.motion_frames(0).shape == (len(plain[0]["pics"]), 3, 36, 44) and h.mb_info(0)[0].shape == (8, 9, 11)
    h.free()
    with pytest.raises(RuntimeError):
        n = lh.decode_batch(_datas()[:1])
        try:
            n.motion(0)
        finally:
            n.free()


def test_the_same_fields_with_a_sink():
    """a sink receives the pictures, the fields stay on the handles"""
    import losslessh264_amd as lh
    plain = _call(True)
    parts = [[] for _ in STREAMS]

    def sink(stream, first, pics, data):
        parts[stream].append(data)
        return 0
    b = lh.decode_batch(_datas(), motion=True, sink=sink)
    got = _result(b, len(STREAMS), data=[b"".join(p) for p in parts])
    for i, name in enumerate(STREAMS):
        for key in ("status", "error", "pics", "data", "geo", "mot", "mbi"):
            assert got[i][key] == plain[i][key], (name, key)


def test_concealed_macroblocks():
    """conceal=: the fields are the model's over the concealing front end's records; concealed macroblocks carry flag bit 1, one vector
    in their sixteen cells and their source's back - one picture, or -1 for the picture of 128s"""
    import losslessh264_amd as lh
    cases = [("conceal/sva_tail56.264", "mv_copy", 1), ("conceal/sva_idr_tail.264", "slice_copy", -1), ("conceal/cvfc1_tail.264", "slice_copy_cross_idr", None)]
    datas = [_read(c[0]) for c in cases]
    for (name, method, back), data in zip(cases, datas):
        b = lh.decode_batch([data], motion=True, conceal=method)
        base = lh.decode_batch([data], conceal=method)
        assert (b.status(0), b.error(0), b.pictures(0), b.data(0), b.concealed(0)) == (base.status(0), base.error(0), base.pictures(0), base.data(0), base.concealed(0))
        frames = lh.parse_file(data, conceal=method)[0]
        got = _result(b, 1)[0]
        base.free()
        mot, mbi, geo = _expected(frames, MM.stream_fields(frames), got["idx"])
        assert got["geo"] == geo and got["mot"] == mot and got["mbi"] == mbi, name
        seen = 0
        for (mb_w, mb_h, _x, _y, mo, io), k in zip(got["geo"], got["idx"]):
            m = np.frombuffer(got["mot"], "<i2", 48 * mb_w * mb_h, mo).reshape(3, mb_h, 4, mb_w, 4)
            flags = np.frombuffer(got["mbi"], np.uint8, 8 * mb_w * mb_h, io).reshape(8, mb_h, mb_w)[3]
            assert int((flags >> 1 & 1).sum()) == frames[k].concealed
            for y, x in zip(*np.nonzero(flags >> 1 & 1)):
                cells = m[:, y, :, x, :]
                assert (cells == cells[:, :1, :1]).all()
                assert back is None or (cells[2] == back).all(), (name, k, y, x)
                seen += 1
        assert seen > 0, name


def test_pick_idr():
    """pick="idr": every delivered picture is intra - every cell 0 - and the kinds are the model's for the selected pictures"""
    got, base = _call(True, pick="idr"), _call(False, pick="idr")
    _pictures_are_the_same(got, base, "pick")
    total = 0
    for i, name in enumerate(STREAMS):
        assert not any(np.frombuffer(got[i]["mot"], "<i2")), name
        if got[i]["status"] == 0:      # (where the header walk stops, the front end's own list ends elsewhere)
            mot, mbi, geo = _expected(_frames(i), _model(i), got[i]["idx"])
            assert got[i]["mbi"] == mbi and got[i]["geo"] == geo and got[i]["mot"] == mot, name
        total += len(got[i]["idx"])
    assert total >= 5 and got[STREAMS.index("streams/BA_MW_D_IDR_LOST.264")]["idx"] == [27, 57, 87]


def test_motion_only():
    """pictures=False with motion=True and no digest: the field bytes, picture records, statuses and stop texts of the full call, no
    picture bytes, and no reconstruct launch (lh264_decode_last_chains 0, 0, 0); with a digest the pictures are reconstructed again and
    the digests are the full call's"""
    import losslessh264_amd as lh
    from losslessh264_amd import _lib as L
    full = _call(True)
    ch = (C.c_longlong * 3)(7, 7, 7)
    for kw in (dict(), dict(parse="device+cabac"), dict(round_pictures=2)):
        got = _result(lh.decode_batch(_datas(), motion=True, pictures=False, **kw), len(STREAMS))
        L.lib().lh264_decode_last_chains(ch)
        assert list(ch) == [0, 0, 0], kw
        for i, name in enumerate(STREAMS):
            for key in ("status", "error", "pics", "idx", "geo", "mot", "mbi"):
                assert got[i][key] == full[i][key], (kw, name, key)
            assert got[i]["data"] == b"", name
        assert got[STREAMS.index("streams/Error_I_P.264")]["error"] != ""
    b = lh.decode_batch(_datas(), motion=True, pictures=False, device_out=True)
    assert all(b.motion_copy(i)[0].cpu().numpy().tobytes() == full[i]["mot"] and b.tensor(i).numel() == 0 for i in range(len(STREAMS)))
    b.free()
    d = lh.decode_batch(_datas(), motion=True, pictures=False, sha1="stream")
    ref = lh.decode_batch(_datas(), sha1="stream", pictures=False)
    L.lib().lh264_decode_last_chains(ch)
    assert ch[0] > 0 and all(d.stream_sha1(i) == ref.stream_sha1(i) for i in range(len(STREAMS)))
    ref.free()
    got = _result(d, len(STREAMS))
    assert all(got[i]["mot"] == full[i]["mot"] and got[i]["data"] == b"" for i in range(len(STREAMS)))


@pytest.mark.parametrize("tool", ["lh264dec", "python"])
def test_the_command_lines(tool, tmp_path):
    """--decode --motion writes <name>.mv and <name>.mbi equal to the handle's buffers beside the pictures; --motion-only writes them
    and no picture file"""
    full = _call(True)
    i = STREAMS.index("streams/BA_MW_D.264")
    src = os.path.join(GOLDEN, STREAMS[i])
    cmd = [os.path.join(ROOT, "losslessh264_amd", "lh264dec")] if tool == "lh264dec" else [sys.executable, "-m", "losslessh264_amd"]
    for flag, files in (("--motion", {"BA_MW_D.264.yuv", "BA_MW_D.264.mv", "BA_MW_D.264.mbi"}), ("--motion-only", {"BA_MW_D.264.mv", "BA_MW_D.264.mbi"})):
        out = tmp_path / flag.strip("-")
        out.mkdir()
        r = subprocess.run(cmd + ["--decode", flag, str(out), src], capture_output=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert set(os.listdir(str(out))) == files
        assert open(str(out / "BA_MW_D.264.mv"), "rb").read() == full[i]["mot"] and open(str(out / "BA_MW_D.264.mbi"), "rb").read() == full[i]["mbi"]
        if flag == "--motion":
            assert open(str(out / "BA_MW_D.264.yuv"), "rb").read() == full[i]["data"]
    r = subprocess.run(cmd + ["--decode", "--motion", "--sha1", str(tmp_path / "x"), src], capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2 and b"--motion" in r.stdout + r.stderr
