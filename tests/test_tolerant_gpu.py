"""LH264_COMPRESS_TOLERANT through the kernels (include/lh264.h): pictures with lost slices - a macroblock no slice covers takes its nnz
entry from the KEEP image (csrc/lh264_ctx.hip ctx_inherit_chain_kernel), as the restorers' FreqImage buffers hold it - and streams with
NAL units the default stream drops without the flag.  The restorers are the ground truth: every stream comes back byte for byte through
the host restore and both instances of the restore kernel, in both forms of the coder, whole and cut at every picture, alone and in
a batch; or it is refused with a text."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import golden_io
import tolerant_cases as T
import losslessh264_amd as lh

R = sys.modules["losslessh264_amd.restore"]
pytestmark = pytest.mark.gpu

REFUSAL = ("a picture with macroblocks no slice covers: the reference conceals them, which is not modelled (the stream would not restore)")
EXTRA = [(b, c) for b in T.BASES for c in T.EXTRA]
_cache = {}


def _lost():
    if "d" not in _cache:
        _cache["d"] = {n: T.lost(n) for n in T.LOST}
    return _cache["d"]


def _compressed():
    """ONE compress_batch with the flag over all streams with lost slices, default coder path: shared, never changed"""
    if "c" not in _cache:
        d = _lost()
        _cache["c"] = dict(zip(T.LOST, lh.compress_batch([d[n] for n in T.LOST], 16, tolerant=True)))
    return _cache["c"]


def _nonempty(tags):
    return {t: b for t, b in tags.items() if b}


@pytest.mark.parametrize("path", ["sw", "wave"])
def test_lost_slices_compress_and_restore(path, monkeypatch):
    """LH264_OK for every stream, the host restore returns the input, and both forms of the coder write the same bytes"""
    monkeypatch.setenv("LH264_CODER_PATH", path)
    d = _lost()
    res = lh.compress_batch([d[n] for n in T.LOST], 16, tolerant=True)
    monkeypatch.delenv("LH264_CODER_PATH")
    for n, (main, tags, err) in zip(T.LOST, res):
        assert err is None, (n, err)
        assert lh.restore(main, tags) == d[n], n
        assert (main, _nonempty(tags)) == (_compressed()[n][0], _nonempty(_compressed()[n][1])), n


@pytest.mark.parametrize("name", T.SYNTHETIC)
def test_the_kernels_compute_the_keep_rule(name):
    """byte for byte what the rule restated on the host gives (tolerant_cases.cpu_compress, the oracle's model and coder)"""
    main, tags, err = _compressed()[name]
    cm, ct = T.cpu_compress(_lost()[name])
    assert err is None and main == cm and _nonempty(tags) == ct


def test_lost_slices_restore_on_the_device():
    """restore_kernel for the CAVLC streams (the CABAC one goes to the host beside it), then restore_cabac_kernel for all of them"""
    d, c = _lost(), _compressed()
    items = [(c[n][0], c[n][1]) for n in T.LOST]
    outs, paths = lh.restore_batch_device(items, 16)
    for n, o, p in zip(T.LOST, outs, paths):
        assert o == d[n], (n, p)
        assert p == (R.PATH_HOST if n == "cabac_slices" else R.PATH_DEVICE), (n, p)
    outs, paths = lh.restore_batch_device(items, 16, cabac_device=True)
    for n, o, p in zip(T.LOST, outs, paths):
        assert o == d[n] and p == R.PATH_DEVICE, (n, p)


def test_lost_slices_cut_at_every_picture():
    """segment_mbs = 1: every picture a segment of its own, KEEP and PAST cross every cut in the stream's two carried buffers - the
    same bytes as uncut"""
    d, c = _lost(), _compressed()
    b = lh.compress_batch_handles([d[n] for n in T.LOST], 16, segment_mbs=1, tolerant=True)
    try:
        for i, n in enumerate(T.LOST):
            main, tags, err = b.result(i)
            assert err is None, (n, err)
            assert b.segments(i) == b.pictures(i) > 1, n
            assert (main, _nonempty(tags)) == (c[n][0], _nonempty(c[n][1])), n
    finally:
        b.free()


def test_lost_slices_alone_as_in_the_batch():
    d, c = _lost(), _compressed()
    for n in T.LOST:
        (main, tags, err), = lh.compress_batch([d[n]], 4, tolerant=True)
        assert err is None and (main, _nonempty(tags)) == (c[n][0], _nonempty(c[n][1])), n


def test_lost_slices_without_the_flag_are_refused_as_ever():
    d = _lost()
    b = lh.compress_batch_handles([d[n] for n in T.LOST], 16)
    try:
        for i, n in enumerate(T.LOST):
            main, tags, err = b.result(i)
            assert b.status(i) == -4 and err == REFUSAL and not _nonempty(tags), (n, err)       # LH264_E_UNSUPPORTED
    finally:
        b.free()


def test_whole_streams_get_the_same_bytes_with_the_flag():
    """every tag and the default stream byte-identical with the flag on and off - and the reference's files (tests/golden/cli_*.npz)"""
    names = ["BA_MW_D.264", "tibby.264", "test_qcif_cabac.264"]
    datas = [T.data(n) for n in names]
    off = lh.compress_batch(datas, 16)
    on = lh.compress_batch(datas, 16, tolerant=True)
    for n, a, b in zip(names, off, on):
        assert a[2] is None and b[2] is None and a[0] == b[0] and a[1] == b[1], n
        z = np.load(os.path.join(golden_io.GOLDEN_DIR, "cli_%s.npz" % n))
        assert b[0] == z["main"].tobytes() and _nonempty(b[1]) == {int(k[4:]): z[k].tobytes() for k in z.files if k.startswith("tag_") and len(z[k])}, n


def test_extra_nal_units_through_the_whole_call():
    """the streams of tests/test_tolerant.py through lh264_compress_batch_opts: LH264_OK means "restores" under the flag - the tagged
    streams are the unmodified stream's -, the two cases that cannot be carried are refused with lh264_parser_not_carried's text"""
    datas = [T.extra(b, c)[0] for b, c in EXTRA]
    refused = [T.extra(b, c)[0] for b in T.BASES for c in T.REFUSED]
    plain = dict(zip(T.BASES, lh.compress_batch([T.data(b) for b in T.BASES], 16)))
    h = lh.compress_batch_handles(datas + refused, 16, tolerant=True)
    try:
        for i, ((b, c), d) in enumerate(zip(EXTRA, datas)):
            main, tags, err = h.result(i)
            assert err is None, (b, c, err)
            assert tags == plain[b][1], (b, c)
            assert lh.restore(main, tags) == d, (b, c)
        for i, d in enumerate(refused):
            main, tags, err = h.result(len(datas) + i)
            assert h.status(len(datas) + i) == -4 and err == lh.not_carried(d) != "" and not _nonempty(tags), err
    finally:
        h.free()
    outs, paths = lh.restore_batch_device([(h_[0], h_[1]) for h_ in lh.compress_batch(datas, 16, tolerant=True)], 16, cabac_device=True)
    assert outs == datas and all(p == R.PATH_DEVICE for p in paths), paths


def test_error_i_p_against_the_reference_files():
    """the reference conceals, and its own restore fails on this stream: equality is not required.  Which of its files ours equal
    under the flag is written down in DESIGN section 6; the default stream is the reference's"""
    sweep = json.load(open(os.path.join(golden_io.GOLDEN_DIR, "ref_sweep.json")))["Error_I_P.264"]
    main, tags, err = _compressed()["error_i_p"]
    assert err is None
    ours = {"main": main}
    ours.update({str(t): b for t, b in _nonempty(tags).items()})
    equal = sorted(k for k in ours if k in sweep["files"] and hashlib.sha1(ours[k]).hexdigest() == sweep["files"][k][1])
    differ = sorted(k for k in set(ours) | set(sweep["files"]) if k not in equal)
    print("Error_I_P.264 under the flag: equal to the reference's files %s, different %s; %d bytes against the reference's %d, input %d"
          % (equal, differ, sum(len(b) for b in ours.values()), sum(v[0] for v in sweep["files"].values()), sweep["bytes"]))
    assert "main" in equal and not sweep["reference_roundtrip"]


def test_command_lines_take_tolerant(tmp_path):
    """`lh264dec --tolerant` and `python -m losslessh264_amd --tolerant`: a stream with a delimiter in front of every picture and one
    with lost slices go into containers that are not verbatim, and come back; the verification stays behind the option"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "losslessh264_amd", "lh264dec")
    srcs = {"aud": T.extra("BA_MW_D.264", "aud")[0], "rows": _lost()["rows"]}
    for k, cmd in enumerate(([exe], [sys.executable, "-m", "losslessh264_amd"])):
        name = ("aud", "rows")[k]
        src, lhp, back = str(tmp_path / (name + ".264")), str(tmp_path / (name + ".lhp")), str(tmp_path / (name + ".back"))
        open(src, "wb").write(srcs[name])
        out = subprocess.run(cmd + ["--tolerant", src, lhp], check=True, capture_output=True, timeout=300, cwd=root).stdout.decode()
        blob = open(lhp, "rb").read()
        assert "verbatim" not in out and len(blob) < len(srcs[name]), out
        assert lh.restore_file(blob) == srcs[name]
        subprocess.run(cmd + [lhp, back], check=True, capture_output=True, timeout=300, cwd=root)
        assert open(back, "rb").read() == srcs[name]
