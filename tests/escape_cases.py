"""What tests/test_escapes.py and tests/test_escapes_gpu.py share: the committed streams of tests/golden/escape/ (written by
tests/golden/make_escape_streams.py), the reference's recorded verdict on them (tests/golden/escape_ref.json), the four refused
streams of tests/golden/edge/, and for all of them the compress direction on the CPU (edge_cases.cpu_compress) with the escape stream,
tag 71, beside it."""
import importlib.util
import json
import os

import edge_cases as E
import golden_io

ESCAPE_DIR = os.path.join(golden_io.GOLDEN_DIR, "escape")
REF = json.load(open(os.path.join(golden_io.GOLDEN_DIR, "escape_ref.json")))
FIXTURES = sorted(REF)
# every stream with a value above its prior table's tree: the three fixtures and the refused edge streams
NAMES = FIXTURES + sorted(E.REFUSED)
TAG_ESC = 71
TB_SKIPRUN, TB_NUMREF = 9, 12


def data(name):
    if name in REF:
        return open(os.path.join(ESCAPE_DIR, name + ".264"), "rb").read()
    return E.data(name)


_made = {}


def made():
    """{name: (bytes, the writer's counters)} from the generator script, run once"""
    if not _made:
        spec = importlib.util.spec_from_file_location("make_escape_streams", os.path.join(golden_io.GOLDEN_DIR, "make_escape_streams.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        _made.update(m.build())
    return _made


_beyond = {}


def beyond(num_ref):
    """a 2x2 stream (tests/h264_synth.py, not committed) whose last picture has `num_ref` > 16 active references: the front end parses
    up to 32, no restorer accepts more than 16, so the escape stream must not carry it.  Registered under "nref<num_ref>" for cpu_compress"""
    name = "nref%d" % num_ref
    if name not in _beyond:
        import h264_synth as H
        import losslessh264_amd as lh

        def mb(k, ref=0):
            return H.p16(ref=ref, mvd=(k % 3, -(k % 2)), cbp_l=1, luma={0: [2 + k % 4] + [0] * 15})
        S = H.Synth(2, 2, num_ref_frames=16)
        S.picture([dict(first_mb=0, type="I", qp=26, mbs=[H.i16(dc=[10 * k - 15] + [0] * 15) for k in range(4)])], idr=True)
        for i in range(1, 16):
            S.picture([dict(first_mb=0, type="P", qp=26, num_ref=None if i == 1 else i, mbs=[mb(i + k, ref=(i - 1) if k == 0 else 0) for k in range(4)])])
        S.picture([dict(first_mb=0, type="P", qp=26, num_ref=num_ref, mbs=[mb(k, ref=(15, 0, 7, 1)[k]) for k in range(4)])])
        _beyond[name] = S.bytes()
        E._parsed[name] = lh.parse_file(_beyond[name], pcm=True)
    return name, _beyond[name]


def cpu_compress(name):
    """-> (default stream, {tag: bytes}) as edge_cases.cpu_compress computes it, the range guard ignored: no tag 71"""
    if name in REF and name not in E._parsed:
        import losslessh264_amd as lh
        E._parsed[name] = lh.parse_file(data(name), pcm=True)
    return E.cpu_compress(name)


def with_escapes(name):
    """-> (default stream, {tag: bytes}) with tag 71 from the front end beside cpu_compress's tags"""
    import losslessh264_amd as lh
    main, tags = cpu_compress(name)
    tags = dict(tags)
    tags[TAG_ESC] = lh.escapes(data(name))
    return main, tags


def leb(*values):
    """unsigned LEB128 varints, concatenated"""
    out = bytearray()
    for v in values:
        while v >= 128:
            out.append((v & 127) | 128); v >>= 7
        out.append(v)
    return bytes(out)


def entries(tag):
    """tag 71 -> [(table, gap, high, repeat)]"""
    vals, v, shift = [], 0, 0
    for b in tag:
        v |= (b & 127) << shift
        shift += 7
        if not b & 128:
            vals.append(v); v, shift = 0, 0
    assert shift == 0 and len(vals) % 4 == 0
    return [tuple(vals[i:i + 4]) for i in range(0, len(vals), 4)]
