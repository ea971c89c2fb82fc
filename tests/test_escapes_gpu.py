"""The escape stream (tag 71, see tests/test_escapes.py) through the kernels: lh264_compress_batch_opts with LH264_COMPRESS_ESCAPES
over every range-edge stream and the three streams of tests/golden/escape/, whole and in segments of one picture, and the device restore
of what it hands out through both kernel instances."""
import sys

import pytest

import edge_cases as E
import escape_cases as X
import restore_cases as RC
import losslessh264_amd as lh

R = sys.modules["losslessh264_amd.restore"]
pytestmark = pytest.mark.gpu

ALL = E.NAMES + X.FIXTURES        # every edge stream, then the fixtures
_cache = {}


def _data(name):
    return X.data(name) if name in X.REF else E.data(name)


def _compressed():
    """ONE compress_batch with the flag over all streams with the default coder path, shared by the restore tests"""
    if "c" not in _cache:
        _cache["c"] = lh.compress_batch([_data(n) for n in ALL], 16, escapes=True)
    return dict(zip(ALL, _cache["c"]))


def _nonempty(tags):
    return {t: b for t, b in tags.items() if b}


@pytest.mark.parametrize("path", ["sw", "wave"])
def test_compress_with_the_flag(path, monkeypatch):
    """no stream is refused; the files are cpu_compress's with tag 71 = lh.escapes beside them; the host restore returns the input; a
    stream inside the range gets what the call without the flag gives"""
    monkeypatch.setenv("LH264_CODER_PATH", path)
    datas = [_data(n) for n in ALL]
    res = lh.compress_batch(datas, 16, escapes=True)
    plain = lh.compress_batch(datas, 16)
    for name, d, (main, tags, err), (pm, pt, perr) in zip(ALL, datas, res, plain):
        assert err is None, (name, err)
        cm, ct = X.cpu_compress(name)
        esc = lh.escapes(d)
        want = dict(ct)
        if esc:
            want[X.TAG_ESC] = esc
        assert (name in X.NAMES) == bool(esc)
        assert main == cm and _nonempty(tags) == want, name
        assert lh.restore(main, tags) == d, name
        if name in X.NAMES:
            assert perr is not None and perr.startswith(lh.out_of_range(d)) and "outside the container's range" in perr, (name, perr)
        else:
            assert perr is None and (pm, _nonempty(pt)) == (main, _nonempty(tags)), name


def test_restore_on_the_device():
    """one launch of restore_kernel over everything the flagged call handed out: bytes equal to the input and to lh264_pip_restore_batch"""
    c = _compressed()
    assert all(c[n][2] is None for n in ALL)
    items = [(c[n][0], c[n][1]) for n in ALL]
    paths = RC.check_same(items, lh.restore_batch_device)
    outs, paths2 = lh.restore_batch_device(items, 16)
    assert paths == paths2 and all(p == R.PATH_DEVICE for p in paths), paths
    for n, o in zip(ALL, outs):
        assert o == _data(n), n


def test_restore_on_the_device_with_the_cabac_writer():
    """the same with a CABAC stream in the batch: restore_cabac_kernel serves the escape streams"""
    c = _compressed()
    cabac = RC.data("test_qcif_cabac.264")
    (cm, ct, cerr), = lh.compress_batch([cabac], 16)
    assert cerr is None
    items = [(c[n][0], c[n][1]) for n in ALL] + [(cm, ct)]
    outs, paths = lh.restore_batch_device(items, 16, cabac_device=True)
    assert all(p == R.PATH_DEVICE for p in paths), paths
    for n, o in zip(ALL, outs):
        assert o == _data(n), n
    assert outs[-1] == cabac


@pytest.mark.parametrize("name,mbs,segments", [("runs_hi", 1664, 6), ("nref16_mixed", 4, 21)])
def test_segments_of_one_picture(name, mbs, segments):
    """the bytes, tag 71 included, do not depend on the cuts (a NUMREF run spans several); restored on the host and on the device"""
    d = X.data(name)
    b = lh.compress_batch_handles([d], 16, segment_mbs=mbs, escapes=True)
    try:
        assert b.segments(0) == segments == X.REF[name]["pictures"]
        main, tags, err = b.result(0)
    finally:
        b.free()
    assert err is None
    whole = _compressed()[name]
    assert main == whole[0] and _nonempty(tags) == _nonempty(whole[1]) and tags[X.TAG_ESC] == lh.escapes(d)
    assert lh.restore(main, tags) == d
    outs, paths = lh.restore_batch_device([(main, tags)], 1)
    assert outs == [d] and paths == [R.PATH_DEVICE]
    # without the flag the stream is refused in segments too
    (_, _, perr), = lh.compress_batch([d], 16, segment_mbs=mbs)
    assert perr is not None and "outside the container's range" in perr


def test_more_than_16_references_stay_refused():
    """17 and 32 active references parse, but no restorer accepts them: refused with the flag as without, beside a stream that is carried"""
    datas = [X.beyond(17)[1], X.beyond(32)[1], X.data("nref16_mixed")]
    for escapes in (True, False):
        res = lh.compress_batch(datas, 16, escapes=escapes)
        for d, (main, tags, err) in zip(datas[:2], res[:2]):
            assert err is not None and err.startswith(lh.out_of_range(d)) and "outside the container's range" in err, err
            assert not _nonempty(tags)
        assert (res[2][2] is None) == escapes
        if escapes:
            assert lh.restore(res[2][0], res[2][1]) == datas[2]


def test_command_lines_take_escapes(tmp_path):
    """`lh264dec --escapes` and `python -m losslessh264_amd --escapes`: skip_all goes out as .pip files with .pip.71 and as a container
    that is not verbatim, and both come back; without the option the files form is refused by lh264dec"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(E.EDGE_DIR, "skip_all.264")
    d = E.data("skip_all")
    exe = os.path.join(root, "losslessh264_amd", "lh264dec")
    for k, cmd in enumerate(([exe], [sys.executable, "-m", "losslessh264_amd"])):
        w = tmp_path / str(k)
        w.mkdir()
        pip, lhp, back = str(w / "out.pip"), str(w / "out.lhp"), str(w / "back.264")
        subprocess.run(cmd + ["--escapes", src, pip], check=True, capture_output=True, timeout=300, cwd=root)
        assert open(pip + ".71", "rb").read() == lh.escapes(d)
        subprocess.run(cmd + [pip, back], check=True, capture_output=True, timeout=300, cwd=root)
        assert open(back, "rb").read() == d
        out = subprocess.run(cmd + ["--escapes", src, lhp], check=True, capture_output=True, timeout=300, cwd=root).stdout.decode()
        assert "verbatim" not in out and len(open(lhp, "rb").read()) < len(d), out
        subprocess.run(cmd + [lhp, back], check=True, capture_output=True, timeout=300, cwd=root)
        assert open(back, "rb").read() == d
    r = subprocess.run([exe, src, str(tmp_path / "no.pip")], capture_output=True, timeout=300, cwd=root)
    assert r.returncode != 0 and b"outside the container's range" in r.stderr
