"""Concealment of lost slices in the decode direction, on the device, against the reference (tests/golden/conceal/, written by
tests/golden/make_conceal_streams.py from the reference's decoder library driven through DecodeFrame2).

Where the reference's result is a function of the stream - pictures that lose only trailing slices, any loss under
disable_deblocking_filter_idc 1 or 2 - every delivered picture must hash to the reference's SHA-1.  Where it is not (a middle or
first slice lost under idc 0: the reference filters received macroblocks against whatever its recycled picture buffer held), the
concealed macroblocks and every macroblock in front of the lost region must equal the reference's planes, and nothing behind it
is compared."""
import hashlib
import json
import os

import numpy as np
import pytest

import losslessh264_amd as lh
from losslessh264_amd import _lib as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "conceal")
REF = json.load(open(os.path.join(DIR, "ref.json")))
METHODS = ["slice_copy", "slice_copy_cross_idr", "slice_copy_cross_idr_freeze", "mv_copy", "mv_copy_freeze"]
EXACT = sorted(n for n, e in REF.items() if e["kind"] in ("trailing", "idc12"))
IDC0 = sorted(n for n, e in REF.items() if e["kind"] == "idc0")


def stream(name):
    if name == "error_i_p":
        return open(os.path.join(HERE, "golden", "streams", "Error_I_P.264"), "rb").read()
    return open(os.path.join(DIR, name + ".264"), "rb").read()


def sizes(m):
    """[w, h] per delivered picture of a ref.json method entry (`size` where they are all alike)"""
    return m["sizes"] if "sizes" in m else [m["size"]] * len(m["sha1"])


def nv12_to_i420(b, w, h):
    a = np.frombuffer(b, np.uint8)
    c = a[w * h:].reshape(h // 2, w // 2, 2)
    return a[:w * h].tobytes() + c[:, :, 0].tobytes() + c[:, :, 1].tobytes()


def decode(names, method, fmt="i420", device_out=False, round_pictures=None):
    """-> per stream (status, error, [picture bytes as I420], [concealed macroblocks])"""
    b = lh.decode_batch([stream(n) for n in names], fmt=fmt, device_out=device_out, round_pictures=round_pictures, conceal=method)
    out = []
    for i in range(len(names)):
        data = bytes(b.tensor(i).cpu().numpy().tobytes()) if device_out else b.data(i)
        pics = []
        for (w, h, _, _, off, n) in b.pictures(i):
            p = data[off:off + n]
            pics.append(nv12_to_i420(p, w, h) if fmt == "nv12" else p)
        out.append((b.status(i), b.error(i), pics, b.concealed(i)))
    b.free()
    return out


_base = {}


def base(method):
    """every exact stream in one batch, host I420, the default round: decoded once per method"""
    if method not in _base:
        _base[method] = dict(zip(EXACT, decode(EXACT, method)))
    return _base[method]


@pytest.mark.parametrize("method", METHODS)
def test_delivered_pictures_equal_the_reference(method):
    for name, (status, error, pics, concealed) in base(method).items():
        ref = REF[name]["methods"][method]
        assert status == 0, (name, error)
        assert [hashlib.sha1(p).hexdigest() for p in pics] == ref["sha1"], name
        if "freeze" not in method or ref["sha1"]:
            lost = {int(k): v for k, v in REF[name]["lost"].items()}
            assert concealed == [lost.get(k, 0) for k in range(len(pics))], name


@pytest.mark.parametrize("method", ["slice_copy_cross_idr", "mv_copy"])
def test_formats_outputs_rounds_and_batch_companions_give_the_same_bytes(method):
    want = base(method)
    for name in EXACT:                                                       # alone, a picture per launch
        assert decode([name], method, round_pictures=1)[0] == want[name], name
    for got, name in zip(decode(EXACT, method, fmt="nv12", round_pictures=8), EXACT):
        assert got == want[name], name
    for got, name in zip(decode(EXACT, method, device_out=True, round_pictures=1), EXACT):
        assert got == want[name], name
    for got, name in zip(decode(EXACT, method, fmt="nv12", device_out=True), EXACT):
        assert got == want[name], name


@pytest.mark.parametrize("method", ["slice_copy_cross_idr", "mv_copy"])
@pytest.mark.parametrize("name", IDC0)
def test_middle_and_first_slice_under_idc0(name, method):
    ref = REF[name]["methods"][method]
    k = ref["first_concealed"]
    z = np.load(os.path.join(DIR, ref["planes"]))
    frames = lh.parse_file(stream(name), conceal=method)[0]
    f = frames[k]
    lost = np.flatnonzero(f.covered == 0)
    assert len(lost) == REF[name]["lost"][str(k)] == f.concealed
    alone = decode([name], method)[0]
    assert alone[0] == 0 and len(alone[2]) == len(ref["sha1"]), alone[1]
    w, h = sizes(ref)[k]
    a = np.frombuffer(alone[2][k], np.uint8)
    got = {"y": a[:w * h].reshape(h, w), "u": a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), "v": a[w * h * 5 // 4:].reshape(h // 2, w // 2)}
    # pictures in front of the damaged one are the reference's
    assert [hashlib.sha1(p).hexdigest() for p in alone[2][:k]] == ref["sha1"][:k]
    lostset = set(int(m) for m in lost)
    check = list(range(int(lost[0]))) + [int(m) for m in lost]       # everything in front of the lost region, and the region
    for m in check:
        x, y = m % f.mb_w, m // f.mb_w
        # a received macroblock's last 3 luma rows / columns (1 chroma) belong to the filter of the macroblock below / right of it:
        # inside `check` those neighbours are in `check` too, at its end they are not compared
        # (a concealed macroblock is compared whole: nothing filters it, in the reference it is written last)
        below, right = m in lostset or m + f.mb_w in check or y == f.mb_h - 1, m in lostset or m + 1 in check or x == f.mb_w - 1
        hy, wy = (16 if below else 13), (16 if right else 13)
        assert np.array_equal(got["y"][16 * y:16 * y + hy, 16 * x:16 * x + wy], z["y"][16 * y:16 * y + hy, 16 * x:16 * x + wy]), (m, "y")
        hc, wc = (8 if below else 7), (8 if right else 7)
        for p in "uv":
            assert np.array_equal(got[p][8 * y:8 * y + hc, 8 * x:8 * x + wc], z[p][8 * y:8 * y + hc, 8 * x:8 * x + wc]), (m, p)
    # the same bytes in a batch and for both round sizes
    for rp in (1, 8):
        r = decode([EXACT[0], name, EXACT[1]], method, round_pictures=rp)
        assert r[1] == alone, rp


def test_error_i_p_decodes_to_the_end():
    """Error_I_P.264 loses slices in five of its six pictures, three of them IDR pictures, and changes its size twice.  With
    concealment on it decodes to its end.  Which of the reference's pictures do not depend on what was decoded before the stream,
    make_conceal_streams.py finds by decoding it alone and behind its own first four pictures (ref.json: `unstable`): delivered
    pictures 2, 3 and 4 - the whole 640x480 IDR picture, the 640x480 P picture that loses trailing slices, the 352x288 IDR picture
    that loses trailing slices behind the change of size - under every method; pictures 0 and 1 (first slices lost under idc 0) do
    depend on it.  The qualifying pictures must hash to the reference's SHA-1.  The sixth picture, damaged and the stream's last, the
    reference's end-of-stream drain does not deliver; here it is concealed and delivered like any other."""
    for method in METHODS:
        ref = REF["error_i_p"]["methods"][method]
        status, error, pics, concealed = decode(["error_i_p"], method)[0]
        assert status == 0, error
        assert len(pics) == (len(ref["sha1"]) if "freeze" in method else len(ref["sha1"]) + 1), method
        qualify = [k for k in range(len(ref["sha1"])) if k not in ref["unstable"]]
        assert qualify == ([0, 1] if "freeze" in method else [2, 3, 4])
        for k in qualify:
            assert hashlib.sha1(pics[k]).hexdigest() == ref["sha1"][k], (method, k)
    frames = lh.parse_file(stream("error_i_p"), conceal="mv_copy")[0]
    a = decode(["error_i_p"], "mv_copy", round_pictures=1)[0]
    assert a[0] == 0, a[1]
    assert len(a[2]) == len(frames) == 6
    assert a[3] == [f.concealed for f in frames] and sum(a[3]) > 0
    assert decode([EXACT[0], "error_i_p"], "mv_copy", round_pictures=8)[1] == a
    fz = decode(["error_i_p"], "mv_copy_freeze")[0]
    assert fz[0] == 0 and len(fz[2]) == sum(not f.frozen for f in lh.parse_file(stream("error_i_p"), conceal="mv_copy_freeze")[0])


def test_without_the_option_nothing_changes():
    for method in (None, "off"):
        status, error, pics, concealed = decode(["sva_tail5"], method)[0]
        assert status == L.E_UNSUPPORTED
        assert error == "picture 5: macroblocks no slice covers (the reference conceals them, which is not modelled)"
        assert len(pics) == 5 and concealed == [0] * 5
    # the options struct from before `conceal` was added still decodes, concealment off
    lib = L.lib()
    import ctypes as C
    data = stream("sva_tail5")
    ptrs = (C.c_char_p * 1)(data)
    lens = (C.c_size_t * 1)(len(data))
    o = L.DecodeOpts()
    o.struct_bytes = L.DECODE_OPTS_BYTES_V1
    o.conceal = L.CONCEAL["mv_copy"]          # behind the end of the struct the caller declares: not read
    outs = (C.c_void_p * 1)()
    assert lib.lh264_decode_batch(ptrs, lens, 1, 1, C.byref(o), outs) == 0
    assert lib.lh264_decoded_status(outs[0]) == L.E_UNSUPPORTED and lib.lh264_decoded_pictures(outs[0]) == 5
    lib.lh264_decoded_free(outs[0])


def test_isvc_object_conceals_only_with_the_option(tmp_path):
    """tests/conceal_client.cpp linked to liblh264.so: with SetOption (DECODER_OPTION_ERROR_CON_IDC) the damaged access unit yields
    its picture and dsDataErrorConcealed, and every picture is the reference's; without it dsBitstreamError and no picture, as ever"""
    import re
    import subprocess
    root = os.path.dirname(HERE)
    so_dir = os.path.join(root, "losslessh264_amd")
    exe = str(tmp_path / "conceal_client")
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-I", os.path.join(root, "include"), os.path.join(HERE, "conceal_client.cpp"), "-o", exe,
                           os.path.join(so_dir, "liblh264.so"), "-Wl,--allow-shlib-undefined", "-Wl,-rpath," + so_dir, "-Wl,-rpath,/opt/rocm/lib"])
    src, w, h = os.path.join(DIR, "sva_tail5.264"), 176, 144
    for method, idc in (("mv_copy", 6), ("slice_copy", 2)):
        out = str(tmp_path / (method + ".yuv"))
        txt = subprocess.run([exe, src, out, str(idc)], capture_output=True, timeout=120, check=True).stdout.decode()
        ref = REF["sva_tail5"]["methods"][method]
        y = open(out, "rb").read()
        n = w * h * 3 // 2
        assert [hashlib.sha1(y[k:k + n]).hexdigest() for k in range(0, len(y), n)] == ref["sha1"]
        states = [int(m, 16) for m in re.findall(r"^pic \d+ state=0x([0-9a-f]+) ", txt, re.M)]
        assert states[5] & 0x20 and not any(s & 0x04 for s in states)
    txt = subprocess.run([exe, src, str(tmp_path / "off.yuv"), "-1"], capture_output=True, timeout=120, check=True).stdout.decode()
    m = re.search(r"^pictures=(\d+) state=0x([0-9a-f]+)$", txt, re.M)
    assert m and int(m.group(1)) == 16 and int(m.group(2), 16) & 0x04 and not int(m.group(2), 16) & 0x20, txt
    for idc in (1, 3):                                               # the FRAME_COPY pair is refused
        assert subprocess.run([exe, src, str(tmp_path / "x.yuv"), str(idc)], capture_output=True, timeout=120).returncode == 4
