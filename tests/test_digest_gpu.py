"""The digests of decoded pictures on the device: sha1_spans_kernel against hashlib (lh264_debug_sha1 with on_device = 1), the
reference's table from a call that delivers no picture, picture digests in every output mode and format against hashlib over a
plain call's bytes, their independence from every cut of the work, local failures, the arena without page-locked output buffers,
and the two command lines.  hashlib and the committed table are the references; every plain decode is made once and shared."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import digest_cases as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
OK, E_ARG, E_UNSUPPORTED = 0, -2, -4
EMPTY = hashlib.sha1(b"").digest()


def _read(name):
    return open(os.path.join(STREAMS, name), "rb").read()


def _table():
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "decoder_sha1.json")))
    return {k: v for k, v in t.items() if not k.startswith("_")}


_cache = {}


def _plain(key, datas, **kw):
    """ONE plain decode_batch (no digest flag) per key -> [(status, error, pictures, bytes)]"""
    if key not in _cache:
        import losslessh264_amd as lh
        b = lh.decode_batch(datas, **kw)
        _cache[key] = [(b.status(i), b.error(i), b.pictures(i), b.data(i)) for i in range(len(datas))]
        b.free()
    return _cache[key]


def _hashes(pictures, data):
    return [hashlib.sha1(data[o:o + nb]).digest() for (_, _, _, _, o, nb) in pictures]


def _lib():
    from losslessh264_amd import _lib as L
    return L, L.lib()


# ---- 1. the kernel against hashlib
def test_padding_edges_at_every_offset_on_the_device():
    L, lib = _lib()
    spans, exp = D.edge_vectors()
    got = D.run(lib, spans, len(exp), 1)
    for s, g, w in zip(spans, got, exp):
        assert g == w, "length %d at offset %d" % (s[2], s[1] & 7)


def test_a_message_fed_in_spans_on_the_device():
    L, lib = _lib()
    spans, n, exp = D.span_vectors()
    assert D.run(lib, spans, n, 1) == exp
    assert D.run(lib, [(1, 5, 3)], 2, 1) == [EMPTY, D.want(5, 3)]


def test_one_launch_of_200_messages_of_different_lengths():
    L, lib = _lib()
    spans, exp = D.many_vectors()
    got = D.run(lib, spans, len(exp), 1)
    bad = [(s[2], s[1] & 3) for s, g, w in zip(spans, got, exp) if g != w]
    assert not bad, bad[:10]


# ---- 2. the reference's table, no picture delivered
def test_the_references_table_without_a_picture_leaving_the_device():
    import losslessh264_amd as lh
    L, lib = _lib()
    sha = _table()
    names = sorted(n for n in os.listdir(STREAMS) if n in sha)
    assert len(names) == 36
    datas = [_read(n) for n in names]
    plain = _plain("table", datas)
    b = lh.decode_batch(datas, sha1="both", pictures=False)
    for i, name in enumerate(names):
        assert (b.status(i), b.error(i)) == (OK, ""), name
        assert b.stream_sha1(i).hex() == sha[name], name
        ln = C.c_size_t(99)
        assert lib.lh264_decoded_bytes(b._h[i], C.byref(ln)) is None and ln.value == 0, name
        ln = C.c_size_t(99)
        assert lib.lh264_decoded_bytes_dev(b._h[i], C.byref(ln)) is None and ln.value == 0, name
        assert b.data(i) == b""
        assert b.pictures(i) == plain[i][2] and len(plain[i][2]) > 0, name
        assert b.picture_sha1(i) == _hashes(plain[i][2], plain[i][3]), name
    # a digest that was not asked for, a bad index
    out = np.zeros(20, np.uint8)
    assert lib.lh264_decoded_picture_sha1(b._h[0], len(plain[0][2]), out.ctypes.data) == E_ARG
    assert lib.lh264_decoded_picture_sha1(b._h[0], -1, out.ctypes.data) == E_ARG
    b.free()
    b = lh.decode_batch(datas[:2], sha1="stream", pictures=False)
    assert lib.lh264_decoded_picture_sha1(b._h[0], 0, out.ctypes.data) == E_ARG
    assert b.stream_sha1(1).hex() == sha[names[1]]
    b.free()
    b = lh.decode_batch(datas[:2], sha1="pictures")
    assert lib.lh264_decoded_stream_sha1(b._h[0], out.ctypes.data) == E_ARG
    assert b.picture_sha1(1) == _hashes(plain[1][2], plain[1][3]) and b.data(1) == plain[1][3]
    b.free()
    b = lh.decode_batch(datas[:1])
    assert lib.lh264_decoded_stream_sha1(b._h[0], out.ctypes.data) == E_ARG and lib.lh264_decoded_picture_sha1(b._h[0], 0, out.ctypes.data) == E_ARG
    b.free()


# ---- 3. picture digests = hashlib over a plain call, in every mode and format
MIX = ["BA_MW_D.264", "CVFC1_Sony_C.jsv", "Static.264"]


def _mix():
    return [_read(n) for n in MIX] + [b"".join(_read(n) for n in ["BA_MW_D.264", "tibby.264", "Static.264", "BA_MW_D.264"])]


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_digests_in_every_output_mode(fmt):
    import losslessh264_amd as lh
    datas = _mix()
    plain = _plain("mix-" + fmt, datas, fmt=fmt)
    assert [p[0] for p in plain] == [OK] * 4
    assert plain[1][2][0][5] == 75600 and plain[1][2][0][:2] == (300, 168) and plain[2][2][0][5] == 22800
    assert len(set(p[:2] for p in plain[3][2])) == 3
    want = [(_hashes(p[2], p[3]), hashlib.sha1(p[3]).digest()) for p in plain]

    def check(b, tag):
        for i in range(4):
            assert b.status(i) == OK and b.pictures(i) == plain[i][2], (tag, i)
            assert b.picture_sha1(i) == want[i][0], (tag, i)
            assert b.stream_sha1(i) == want[i][1], (tag, i)
    b = lh.decode_batch(datas, fmt=fmt, sha1="both")
    check(b, "host")
    for i in range(4):
        assert b.data(i) == plain[i][3]
    b.free()
    b = lh.decode_batch(datas, fmt=fmt, sha1="both", device_out=True)
    check(b, "device_out")
    for i in range(4):
        assert b.tensor(i).cpu().numpy().tobytes() == plain[i][3]
    b.free()
    got = [[] for _ in datas]

    def sink(stream, first, plist, data):
        got[stream].append(data)
        return 0
    b = lh.decode_batch(datas, fmt=fmt, sha1="both", sink=sink, round_pictures=5)
    check(b, "sink")
    for i in range(4):
        assert b"".join(got[i]) == plain[i][3] and b.data(i) == b""
    b.free()
    b = lh.decode_batch(datas, fmt=fmt, sha1="both", pictures=False)
    check(b, "no pictures")
    b.free()


# ---- 4. cuts
def test_the_digests_do_not_depend_on_the_cuts():
    import losslessh264_amd as lh
    two = [_read("CVFC1_Sony_C.jsv"), _read("Static.264")]
    plain = _plain("two", two)
    want = [(_hashes(p[2], p[3]), hashlib.sha1(p[3]).digest()) for p in plain]
    assert plain[0][2][0][5] % 64 and plain[1][2][0][5] % 64          # partial blocks carry across rounds
    sha = _table()
    assert want[0][1].hex() == sha["CVFC1_Sony_C.jsv"] and want[1][1].hex() == sha["Static.264"]
    others = [_read(n) for n in ("BA_MW_D.264", "SVA_BA2_D.264", "MR1_BT_A.h264", "BA_MW_D.264", "SVA_BA2_D.264")]
    among = others[:3] + [two[0]] + others[3:] + others[:2] + [two[1]] + others[2:4] + others[4:]
    assert len(among) == 12
    cases = [(two, (0, 1), kw) for kw in ({"round_pictures": 1}, {"round_pictures": 3}, {"round_pictures": 8}, {"group_mbs": 100}, {"threads": 1}, {"threads": 4})]
    cases += [([two[0]], (0, None), {}), ([two[1]], (None, 0), {}), (among, (3, 8), {}), (among, (3, 8), {"round_pictures": 3, "threads": 4})]
    for datas, where, kw in cases:
        b = lh.decode_batch(datas, sha1="both", pictures=False, **kw)
        for k, i in enumerate(where):
            if i is None:
                continue
            assert b.status(i) == OK, (kw, k)
            assert b.picture_sha1(i) == want[k][0], (kw, k)
            assert b.stream_sha1(i) == want[k][1], (kw, k)
        b.free()


# ---- 5. failures stay local
def test_failures_stay_local():
    import losslessh264_amd as lh
    sha = _table()
    ba, err = _read("BA_MW_D.264"), _read("Error_I_P.264")
    cut = _read("SVA_BA2_D.264")
    cut = cut[:len(cut) // 2 + 3]
    rnd = np.random.default_rng(7).integers(0, 256, 1024, dtype=np.uint8).tobytes()
    batch = [ba, err, _read("CVFC1_Sony_C.jsv"), ba + err, _read("Static.264"), b"", rnd, _read("SVA_BA2_D.264"), cut, _read("MR1_BT_A.h264")]
    good = {0: "BA_MW_D.264", 2: "CVFC1_Sony_C.jsv", 4: "Static.264", 7: "SVA_BA2_D.264", 9: "MR1_BT_A.h264"}
    plain = _plain("local", batch)
    for kw in ({"pictures": False}, {}):
        b = lh.decode_batch(batch, sha1="both", **kw)
        for i in range(len(batch)):
            assert b.status(i) == plain[i][0] and b.pictures(i) == plain[i][2], i
            assert b.picture_sha1(i) == _hashes(plain[i][2], plain[i][3]), i
            assert b.stream_sha1(i) == hashlib.sha1(plain[i][3]).digest(), i
        for i, name in good.items():
            assert b.status(i) == OK and b.stream_sha1(i).hex() == sha[name], name
        # the stream that stops at picture 100 has the 100 digests of the whole stream in front of it
        assert b.status(3) == E_UNSUPPORTED and len(b.picture_sha1(3)) == 100 and b.stream_sha1(3).hex() == sha["BA_MW_D.264"]
        assert b.status(8) == E_UNSUPPORTED and 0 < len(b.picture_sha1(8)) < len(b.picture_sha1(7))
        assert b.picture_sha1(8) == b.picture_sha1(7)[:len(b.picture_sha1(8))]
        for i in (1, 5, 6):
            assert b.picture_sha1(i) == [] and b.stream_sha1(i) == EMPTY, i
        b.free()
    # concealment with a freeze method: withheld pictures have no index and no digest
    for method in ("mv_copy_freeze", "slice_copy_cross_idr_freeze", "slice_copy"):
        pc = _plain("conceal-" + method, [err, ba], conceal=method)
        assert pc[0][0] == OK
        frames = lh.parse_file(err, conceal=method)[0]
        assert len(pc[0][2]) == sum(not f.frozen for f in frames)
        if "freeze" in method:
            assert len(pc[0][2]) < len(frames)
        b = lh.decode_batch([err, ba], conceal=method, sha1="both", pictures=False, round_pictures=2)
        for i in range(2):
            assert b.status(i) == OK and b.pictures(i) == pc[i][2], (method, i)
            assert b.picture_sha1(i) == _hashes(pc[i][2], pc[i][3]), (method, i)
            assert b.stream_sha1(i) == hashlib.sha1(pc[i][3]).digest(), (method, i)
        b.free()


def test_a_sink_that_refuses_keeps_the_digests_of_what_it_took():
    import losslessh264_amd as lh
    ba = _read("BA_MW_D.264")
    plain = _plain("ba", [ba])[0]
    taken = []

    def sink(stream, first, plist, data):
        if first >= 16:
            return 1
        taken.append(data)
        return 0
    b = lh.decode_batch([ba], sha1="both", sink=sink, round_pictures=8)
    assert b.status(0) == E_ARG and b.error(0) == "sink"
    assert len(b.pictures(0)) == 16
    assert b.picture_sha1(0) == _hashes(plain[2], plain[3])[:16]
    assert b.stream_sha1(0) == hashlib.sha1(b"".join(taken)).digest()
    b.free()


# ---- 6. the arena
_CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import losslessh264_amd as lh
from losslessh264_amd import _lib as L
datas = [open(%r, "rb").read()] * 64
out = {}
for key, kw in (("plain", {}), ("digests", {"sha1": "both", "pictures": False})):
    L.lib().lh264_decode_release()
    b = lh.decode_batch(datas, **kw)
    out[key] = {"status": [b.status(i) for i in range(64)].count(0), "arena": lh.decode_arena_bytes()}
    if kw:
        out[key]["sha"] = sorted(set(b.stream_sha1(i).hex() for i in range(64)))
    b.free()
print(json.dumps(out))
"""


def test_no_page_locked_output_buffers_without_pictures():
    code = _CHILD % (ROOT, os.path.join(STREAMS, "BA_MW_D.264"))
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, timeout=300).stdout.decode()
    got = json.loads(out.strip().splitlines()[-1])
    print(got)
    assert got["plain"]["status"] == 64 and got["digests"]["status"] == 64
    assert got["digests"]["sha"] == [_table()["BA_MW_D.264"]]
    # a round of the plain call holds 64 * 8 QCIF pictures twice in page-locked memory; the digests-only call none of them
    assert got["digests"]["arena"][1] < got["plain"]["arena"][1] - 2 * 64 * 8 * 38016 + (1 << 20)
    assert got["digests"]["arena"][1] < got["plain"]["arena"][1]


# ---- 7. the command lines
def test_the_command_lines(tmp_path):
    sha = _table()
    names = ("BA_MW_D.264", "CVFC1_Sony_C.jsv")
    srcs = [os.path.join(STREAMS, n) for n in names]
    plain = _plain("cli", [_read(n) for n in names])
    for k, cmd in enumerate(([os.path.join(ROOT, "losslessh264_amd", "lh264dec")], [sys.executable, "-m", "losslessh264_amd"])):
        d = tmp_path / str(k)
        d.mkdir()
        r = subprocess.run(cmd + ["--decode", "--sha1", str(d)] + srcs, capture_output=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, (r.stdout.decode(), r.stderr.decode())
        assert sorted(os.listdir(str(d))) == sorted(n + ".sha1" for n in names), cmd
        for i, name in enumerate(names):
            lines = open(str(d / (name + ".sha1"))).read().splitlines()
            assert lines[-1] == "stream " + sha[name], (cmd, name)
            want = ["%d %d %d %d %d %s" % (j, w, h, fn, idr, dg.hex()) for j, ((w, h, fn, idr, _, _), dg) in enumerate(zip(plain[i][2], _hashes(plain[i][2], plain[i][3])))]
            assert lines[:-1] == want, (cmd, name)
