"""The options of the batch decode call in combination (lh264_decode_batch_ex4): device parse with views, float RGB, motion fields and
digests in one call, on the host, on the device and - picking, scaled, NV12 - through a sink, each cut into several rounds that not
every stream fits.  Every such call delivers what the same call delivers with host parse, default rounds, no motion and no digests;
its fields are those of the motion-only call; its digests are hashlib's over the bytes it delivered.  Every call is made once."""
import ctypes as C
import hashlib
import os

import pytest

from test_decode_rgb_gpu import _head

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# QCIF CAVLC; CIF CABAC (I, then P); a 300 x 168 window in a 320 x 176 picture, CAVLC - the first few pictures of each
STREAMS = [("streams/BA_MW_D.264", 5), ("streams/test_cif_P_CABAC_slice.264", 6), ("streams/CVFC1_Sony_C.jsv", 5)]
# 2 pictures of a stream per round, and a round holds 1300 macroblocks: the first round is the QCIF stream's alone (an unknown stream
# counts as CIF), the next ones have no room for the third stream behind 2 x 99 + 2 x 396 macroblocks (its pictures are unselected
# again), and it joins the CIF stream when the QCIF stream is through
FORCED = dict(round_pictures=2, group_mbs=1300)
VIEW = dict(size=(64, 48), fit="contain", crop=[(16, 8, 128, 96), None, (2, 4, 200, 120)], colour="rgbp", dtype="float16")
PICKED = dict(pick="intra", fmt="nv12", scale=1)

_cache = {}


def _datas():
    if "datas" not in _cache:
        _cache["datas"] = [_head(open(os.path.join(GOLDEN, n), "rb").read(), k) for n, k in STREAMS]
    return _cache["datas"]


def _result(b, data=None):
    """what a call delivered, per stream; data: the bytes where the handle does not hold them (a sink)"""
    n = len(STREAMS)
    out = []
    for i in range(n):
        r = dict(status=b.status(i), error=b.error(i), pics=b.pictures(i), idx=b.picture_indices(i), views=b.views(i), sizes=b.source_sizes(i), path=b.parse_path(i))
        r["data"] = data[i] if data is not None else b.tensor(i).cpu().numpy().tobytes() if b.device_out else b.data(i)
        if b.has_motion:
            mot, mbi = b._field_buffers(i)
            if b.device_out:
                mot, mbi = mot.cpu().numpy(), mbi.cpu().numpy()
            r.update(geo=b.motion_geometry(i), mot=mot.tobytes(), mbi=mbi.tobytes())
        if b._sha1 in ("pictures", "both"):
            r["pic_sha"] = b.picture_sha1(i)
        if b._sha1 in ("stream", "both"):
            r["stream_sha"] = b.stream_sha1(i)
        out.append(r)
    b.free()
    return out


def _call(name, sink=False, **kw):
    """ONE decode_batch over the three streams per name -> (results, [rounds, chains, jobs] of its reconstruct launches, what a sink saw)"""
    if name not in _cache:
        import losslessh264_amd as lh
        from losslessh264_amd import _lib as L
        seen = [[] for _ in STREAMS]

        def take(stream, first, pics, data):
            seen[stream].append((first, pics, data))
            return 0
        b = lh.decode_batch(_datas(), sink=take if sink else None, **kw)
        ch = (C.c_longlong * 3)(0, 0, 0)
        L.lib().lh264_decode_last_chains(ch)
        b._sha1 = kw.get("sha1")
        _cache[name] = (_result(b, [b"".join(p[2] for p in s) for s in seen] if sink else None), list(ch), seen)
    return _cache[name]


def _same_pictures(got, base, what):
    for i, (name, _) in enumerate(STREAMS):
        for key in ("status", "error", "pics", "idx", "views", "sizes"):
            assert got[i][key] == base[i][key], (what, name, key)
        assert got[i]["status"] == 0 and len(got[i]["pics"]) >= 1, (what, name)
        assert len(got[i]["data"]) == sum(p[5] for p in got[i]["pics"]) > 0 and got[i]["data"] == base[i]["data"], (what, name)


def _same_fields(got, only, what):
    for i, (name, _) in enumerate(STREAMS):
        assert only[i]["idx"] == got[i]["idx"] and only[i]["data"] == b"", (what, name)
        for key in ("geo", "mot", "mbi"):
            assert got[i][key] == only[i][key] and len(got[i][key]) > 0, (what, name, key)


def _digests_of_the_bytes(got, what, stream):
    for i, (name, _) in enumerate(STREAMS):
        data = got[i]["data"]
        assert got[i]["pic_sha"] == [hashlib.sha1(data[p[4]:p[4] + p[5]]).digest() for p in got[i]["pics"]], (what, name)
        if stream:
            assert got[i]["stream_sha"] == hashlib.sha1(data).digest(), (what, name)


def test_the_forcing_reaches_several_rounds():
    """the cuts of FORCED: more than one reconstruct launch, more chains than rounds (streams share a round), and the plain calls'
    single round for comparison"""
    _, ch, _ = _call("A", parse="device+cabac", motion=True, sha1="both", **VIEW, **FORCED)
    _, base_ch, _ = _call("A0", **VIEW)
    assert ch[0] > 1 and ch[1] > ch[0] and base_ch[0] == 1, (ch, base_ch)
    assert ch[2] == base_ch[2] == sum(k for _, k in STREAMS)


def test_device_parse_view_float_rgb_motion_digests_on_the_host():
    """A: parse="device+cabac", size + fit="contain" + a crop per stream, colour="rgbp", dtype="float16", motion, sha1="both"; host
    output, forced rounds"""
    got, ch, _ = _call("A", parse="device+cabac", motion=True, sha1="both", **VIEW, **FORCED)
    assert ch[0] > 1
    assert [r["path"] for r in got] == ["device"] * 3
    _same_pictures(got, _call("A0", **VIEW)[0], "A")
    _same_fields(got, _call("M", motion=True, pictures=False)[0], "A")
    _digests_of_the_bytes(got, "A", stream=True)
    assert got[2]["views"][0] == ((2, 4, 200, 120), (0, 4, 64, 38)) and got[1]["views"][0][0] == (0, 0, 352, 288)
    assert all(p[:2] == (64, 48) and p[5] == 64 * 48 * 3 * 2 for r in got for p in r["pics"])


def test_the_same_on_the_device():
    """B: A with device_out=True - the bytes of the device call with host parse and default rounds, which are A's"""
    got, ch, _ = _call("B", parse="device+cabac", motion=True, sha1="both", device_out=True, **VIEW, **FORCED)
    assert ch[0] > 1
    _same_pictures(got, _call("B0", device_out=True, **VIEW)[0], "B")
    _same_pictures(got, _call("A0", **VIEW)[0], "B against the host call")
    _same_fields(got, _call("M", motion=True, pictures=False)[0], "B")
    _digests_of_the_bytes(got, "B", stream=True)


def test_pick_nv12_scale_motion_digests_through_a_sink():
    """C: pick="intra", fmt="nv12", scale=1, motion, sha1="pictures" through a sink, forced rounds: the sink saw exactly the bytes the
    call without sink, motion and digests returned, in runs that continue one another"""
    got, ch, seen = _call("C", sink=True, motion=True, sha1="pictures", **PICKED, **FORCED)
    assert ch[0] > 1
    base = _call("C0", **PICKED)[0]
    _same_pictures(got, base, "C")
    _same_fields(got, _call("MC", motion=True, pictures=False, pick="intra")[0], "C")
    _digests_of_the_bytes(got, "C", stream=False)
    for i, (name, _) in enumerate(STREAMS):
        assert [p for run in seen[i] for p in run[1]] == base[i]["pics"], name
        assert [run[0] for run in seen[i]] == [sum(len(r[1]) for r in seen[i][:k]) for k in range(len(seen[i]))], name
    assert got[0]["pics"][0][:2] == (88, 72) and got[0]["sizes"][0] == (176, 144)
