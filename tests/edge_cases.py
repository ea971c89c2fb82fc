"""What tests/test_edges.py and tests/test_edges_gpu.py share: the committed range-edge streams (tests/golden/edge/, written by
tests/golden/make_edge_streams.py), the reference's recorded verdict on them (tests/golden/edge_ref.json), the set the compress
direction must refuse, and the compress direction on the CPU (host symbols + the oracle's coefficient symbols through the oracle's
coder) for the tests that run without a device."""
import ctypes as C
import hashlib
import importlib.util
import json
import os

import numpy as np

import golden_io
import oracle_lib as O

EDGE_DIR = os.path.join(golden_io.GOLDEN_DIR, "edge")
REF = json.load(open(os.path.join(golden_io.GOLDEN_DIR, "edge_ref.json")))
NAMES = sorted(REF)
# streams with a value the container's prior tables cannot carry: compress must refuse them (callers store them verbatim)
REFUSED = {"skip512", "skip513", "skip_all", "nref_2_3_15_16"}
TAG_PCM = 70
# files that differ from the reference's, by tag.  align_bits: ones where the alignment zero bits behind a slice's stop bit belong.  The
# reference takes its end-of-slice flag (tag 2) from the bits that are left, is misled by them and does not restore its own files; this
# code takes the flag from the macroblock's position and restores the stream
FILES_DIFFER = {"align_bits": {2}}


def sha(b):
    return hashlib.sha1(bytes(b)).hexdigest()


def data(name, directory=EDGE_DIR):
    return open(os.path.join(directory, name + ".264"), "rb").read()


_made = {}


def made(script="make_edge_streams"):
    """{name: (bytes, the writer's counters)} from the generator script, run once"""
    if script not in _made:
        spec = importlib.util.spec_from_file_location(script, os.path.join(golden_io.GOLDEN_DIR, script + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        _made[script] = m.build()
    return _made[script]


_parsed = {}


def parsed(name, directory=EDGE_DIR):
    """(frames, error text, default stream, I_PCM samples) of the host front end, once per stream (names are unique over directories)"""
    if name not in _parsed:
        import losslessh264_amd as lh
        _parsed[name] = lh.parse_file(data(name, directory), pcm=True)
    return _parsed[name]


def merged_symbols(frames):
    """host symbols of the parser + the oracle's coefficient symbols at the splice markers, as one flat array"""
    from losslessh264_amd.ctx import past_policy
    pol = past_policy(frames)
    imgs = O.model_nnz_images(frames, pol)
    out = []
    for i, f in enumerate(frames):
        ctx = O.model_frame_symbols(f, imgs[i], imgs[pol[i]] if pol[i] is not None else None)
        hs = f.syn_syms.astype(O.ORC_SYM_DTYPE) if f.syn_syms.dtype != O.ORC_SYM_DTYPE else f.syn_syms
        at = 0
        for k in np.flatnonzero(f.syn_syms["kind"] == 15):
            out.append(hs[at:k]); at = k + 1
            mb = int(np.searchsorted(f.syn_off, k, side="right")) - 1
            out.append(ctx[mb])
        out.append(hs[at:])
    return np.ascontiguousarray(np.concatenate(out))


_compressed = {}


def cpu_compress(name, directory=EDGE_DIR):
    """-> (default stream, {tag: bytes}) without a device: what lh264_compress_batch computes with its kernels"""
    if name not in _compressed:
        frames, err, main, pcm = parsed(name, directory)
        assert err == "", (name, err)
        syms = merged_symbols(frames)
        L = O.lib()
        L.orc_coder_new.restype = C.c_void_p
        L.orc_coder_error.restype = C.c_char_p
        c = C.c_void_p(L.orc_coder_new(0))
        assert L.orc_coder_symbols(c, syms.ctypes.data_as(C.c_void_p), C.c_long(len(syms))) == 0, L.orc_coder_error(c)
        L.orc_coder_finish(c)
        tags = {}
        for t in range(72):
            p = C.c_void_p()
            ln = L.orc_coder_tag(c, t, C.byref(p))
            if ln:
                tags[t] = bytes(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(ln,)))
        L.orc_coder_free(c)
        if pcm:
            tags[TAG_PCM] = pcm
        _compressed[name] = (main, tags)
    return _compressed[name]


def oracle_i420(frames):
    """the pictures by the oracle's reconstruction, as the I420 file the reference's console application writes"""
    pics, out = {}, []
    for f in frames:
        dst = O.HostPic(f.mb_w, f.mb_h)
        refs = [pics[r] if r in pics else dst for r in f.ref_ids]
        refs += [dst] * (16 - len(refs))
        O.recon_frame(f.mbs, f.coeffs, f.slices, dst, refs, 0 if f.is_ref else O.NO_EXPAND)
        pics[f.id] = dst
        for p in range(3):
            s = 1 if p else 0
            out.append(np.ascontiguousarray(dst.plane(p)[f.crop_y >> s:(f.crop_y + f.crop_h) >> s, f.crop_x >> s:(f.crop_x + f.crop_w) >> s]).tobytes())
    return b"".join(out)


def same_as_reference_files(name, main, tags, record=None, files_differ=None):
    """the files equal the reference's recorded ones (our additional I_PCM stream and the tags of FILES_DIFFER aside, which must differ);
    record, files_differ: those of another set of streams"""
    ref = (record or REF)[name]["files"]
    ours = {t: b for t, b in tags.items() if t != TAG_PCM and b}
    differ = {t for t in ours if str(t) in ref and sha(ours[t]) != ref[str(t)][1]}
    return set(str(t) for t in ours) == set(k for k in ref if k != "main") and sha(main) == ref["main"][1] and \
        differ == (FILES_DIFFER if files_differ is None else files_differ).get(name, set())
