"""The CABAC paths at their syntax edges on synthetic streams (tests/golden/cabac_edge/, written by
tests/golden/make_cabac_edge_streams.py with the test writer tests/h264_synth_cabac.py): the UEG0 joint at 14 and the UEG3 joint at 9,
Exp-Golomb suffixes up to int16 levels, ref_idx above 0, every ctxIdxInc of mvd, mb_qp_delta, ref_idx, mb_skip_flag and
transform_size_8x8_flag, SliceQPY 0 and 51 under every initialisation table, every last position of every significance map, a chain of
outstanding bits longer than a byte, the engine restart around I_PCM, cabac_alignment_one_bit and the stop bit at every bit phase.

Every edge is asserted twice: from what the writer counted while it wrote, and from what the front end read back.  The reference's
verdict on each stream (tests/golden/cabac_edge_ref.json) was taken once from the unmodified reference on the CPU.

The property every restore path must meet on every stream: either compress refuses it, or the restore equals the input.  Everything
here runs without a device; tests/test_cabac_edges_gpu.py repeats it through the kernels."""
import sys

import numpy as np
import pytest

import cabac_edge_cases as CE
import edge_cases as E
import restore_cases as RC
import losslessh264_amd as lh

R = sys.modules["losslessh264_amd.restore"]
MB_TYPE = {"skip": 0x100, "pcm": 0x200, "p16": 0x8, "i16": 0x2}
MAXN = {0: 16, 1: 15, 2: 16, 3: 4, 4: 15, 5: 64}


def _count(name):
    return CE.made()[name][1]


def _mvd_values():
    """as make_edge_streams.mvd_values()"""
    v = {10, 11}
    for k in range(14):
        v |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    return v - {0}


def test_the_cabac_edge_set():
    assert CE.NAMES == sorted(["cabac_levels", "cabac_sigmap", "cabac_mvd", "cabac_qp", "cabac_refidx", "cabac_refidx16", "cabac_skip", "cabac_pcm",
                               "cabac_phase", "cabac_carry", "cabac_mixed"])
    assert set(CE.made()) == set(CE.NAMES)
    biggest = max(len(E.data(n)) for n in E.NAMES)              # the size range of tests/golden/edge/
    for n in CE.NAMES:
        assert len(CE.data(n)) <= biggest, n


@pytest.mark.parametrize("name", CE.NAMES)
def test_cabac_stream_regenerates_byte_for_byte(name):
    d = CE.data(name)
    assert CE.made()[name][0] == d
    assert (len(d), E.sha(d)) == (CE.REF[name]["bytes"], CE.REF[name]["sha1"])


# ---- what the writer counted ---------------------------------------------------------------------------------------------------------
def test_levels_counters():
    c = _count("cabac_levels")
    want = {0, 1, 12, 13, 14, 15, 16, 32766, 32767}
    for k in range(15):
        want |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    for cat in range(6):
        for v in want:
            assert c["abs_level"].get((cat, v), 0) >= (2 if v < 32767 else 1), (cat, v)      # both signs; 32767 is -32768 alone
        gt1, eq1 = c["gt1_eq1"][cat]
        assert gt1 >= (3 if cat == 3 else 4) and eq1 >= 3, cat                               # where Min() of 9.3.3.1.3 saturates
        assert (gt1, eq1) == (MAXN[cat] - 1, MAXN[cat] - 1)                                  # a full block of ones and one of levels above 1
        assert (cat, MAXN[cat] - 1) in c["last_pos"]
    assert (c["level_min"], c["level_max"]) == (-32768, 32767)


def test_sigmap_counters():
    c = _count("cabac_sigmap")
    for cat in range(6):
        for i in range(MAXN[cat]):
            assert (cat, i) in c["last_pos"], (cat, i)            # the last position included: no last_significant_coeff_flag there
        if cat != 5:
            assert c["cbf_zero"].get(cat, 0) >= 1, cat
    assert (5, 63) in c["last_pos"]


def test_mvd_counters():
    c = _count("cabac_mvd")["mvd"]
    assert {8, 9, 10, 11} <= _mvd_values()
    assert (c["min"], c["max"]) == (-8193, 8193)
    for comp in range(2):
        assert {2, 3, 32, 33} <= c["sums"][comp]
        assert set(c["inc"][comp]) == {0, 1, 2}


def test_qp_counters():
    c = _count("cabac_qp")
    assert (c["qp_min"], c["qp_max"], c["dqp"]["min"], c["dqp"]["max"]) == (0, 51, -26, 25)
    assert {("nonzero", 1), ("skip", 0), ("pcm", 0), ("cbp0", 0), ("first", 0), ("zero", 0)} == c["dqp"]["after"]
    assert {(t, q) for t in ("I", 0, 1, 2) for q in (0, 51)} <= c["slice_qp"]


@pytest.mark.parametrize("name,most", [("cabac_refidx", 15), ("cabac_refidx16", 16)])
def test_ref_idx_counters(name, most):
    c = _count(name)["ref_idx"]
    assert c["top"] == {n: n - 1 for n in range(1, most + 1)}
    assert set(c["inc"]) == {0, 1, 2, 3}
    assert CE.data("cabac_refidx16").startswith(CE.data("cabac_refidx"))
    assert _count(name)["pictures"] == most + 2 - (most == 15)


def test_skip_counters():
    c = _count("cabac_skip")
    assert set(c["skip_inc"]) == {0, 1, 2}
    assert c["slice_bytes_min"] == 2                              # one skip flag and the end of the slice: the smallest slice the pad patch meets
    w = c["written"]
    assert [len(p) for p in w] == [1200, 1200, 1200, 1, 1]
    assert all(r["kind"] == "skip" for r in w[1]) and w[4][0]["kind"] == "skip"


def test_pcm_counters():
    c = _count("cabac_pcm")
    assert {(cat, side) for cat in range(5) for side in "AB"} == c["cbf_pcm"]      # a coded neighbour right of and below an I_PCM
    assert c["epb"] >= 4 * 191 - 191 and c["epb_arith"] == 0      # 384 zero samples: an emulation prevention byte behind every two
    assert len(c["pcm_phase"]) >= 4
    for pic, want in zip(c["written"], (["pcm", "pcm", "i16", "i16", "i16", "i16", "i16", "pcm"], ["pcm", "p16", "skip", "pcm", "p16", "skip", "pcm", "pcm"],
                                        ["skip", "pcm", "p16", "p16", "i16", "pcm", "i16", "i16"])):
        assert [r["kind"] for r in pic] == want


def test_phase_counters():
    c = _count("cabac_phase")
    assert c["hdr_phase"] == set(range(8))                        # 0: no cabac_alignment_one_bit, else 8 - phase of them
    assert c["stop_phase"] == set(range(8))


def test_carry_counters():
    c = _count("cabac_carry")
    assert c["outstanding_max"] == 18 and c["outstanding_max"] >= 9      # the seed's chain: more than a whole output byte
    assert c["epb_arith"] >= 1


def test_mixed_counters():
    c = _count("cabac_mixed")
    assert set(c["t8_inc"]) == {0, 1, 2}
    assert {t for t, _ in c["slice_qp"]} == {"I", 0, 1, 2}
    frames = CE.parsed("cabac_mixed")[0]
    assert [int(f.slice_syn[0, 3]) & 1 for f in frames] == [1, 0, 1, 0, 1, 0]      # CABAC and CAVLC pictures alternate
    assert [len(f.slices) for f in frames] == [2, 2, 3, 2, 2, 1]
    assert {int(t) for f in frames for t in f.syn["t8"]} == {0, 1}


# ---- what the front end reads back ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CE.NAMES)
def test_front_end_reads_what_the_writer_wrote(name):
    frames, err, main, pcm = CE.parsed(name)
    c = _count(name)
    assert err == ""
    assert len(frames) == c["pictures"] == CE.REF[name]["pictures"] == len(c["written"])
    samples = b""
    for f, w in zip(frames, c["written"]):
        assert f.covered.all() and len(f.mbs) == len(w)
        lv = f.levels.reshape(len(w), -1)
        for k, r in enumerate(w):
            if r is None:                                         # a macroblock of a CAVLC slice (cabac_mixed)
                continue
            where = (name, f.id, k)
            assert int(f.mbs["mb_type"][k]) == MB_TYPE[r["kind"]], where
            assert int(f.mbs["qp_y"][k]) == r["qp"], where
            if r["kind"] == "p16":
                assert tuple(int(x) for x in f.syn["mvd"][k, 0, :]) == r["mvd"], where
                assert int(f.syn["ref_idx"][k, 0]) == r["ref"], where
            if "levels" in r:
                assert sorted(int(x) for x in lv[k] if x) == r["levels"], where
            if r["kind"] == "pcm":
                samples += r["pcm"]
    assert pcm == samples


def test_mvd_read_back():
    p = CE.parsed("cabac_mvd")[0][1]
    want = _mvd_values()
    w = p.mb_w
    mvd = p.syn["mvd"][:w, 0, :].astype(np.int64)
    assert set(int(x) for x in mvd[:, 0]) == want | {-v for v in want} == set(int(x) for x in mvd[:, 1])
    assert (p.mbs["mb_type"][w:] == MB_TYPE["skip"]).all()


# ---- against the reference's verdict -------------------------------------------------------------------------------------------------
def test_reference_verdict_as_recorded():
    """the unmodified reference decodes every stream but cabac_refidx16 (16 references: its console application aborts); its own round
    trip holds for cabac_mvd, cabac_refidx and cabac_phase.  For every other stream it decodes, its restore fails on its own files:
    cabac_edge_cases.REFERENCE_DOES_NOT_RESTORE names each with what it said"""
    assert {n for n in CE.NAMES if CE.REF[n]["reference_decodes"]} == set(CE.NOT_REFUSED)
    back = {n for n in CE.NAMES if CE.REF[n]["reference_roundtrip"]}
    assert back == {"cabac_mvd", "cabac_refidx", "cabac_phase"}
    assert set(CE.REFERENCE_DOES_NOT_RESTORE) == set(CE.NOT_REFUSED) - back
    for n, (rc, said, _) in CE.REFERENCE_DOES_NOT_RESTORE.items():
        assert CE.REF[n]["restore_rc"] == rc and said in CE.REF[n]["restore_message"], n
        if rc == 0:
            assert CE.REF[n]["restore_bytes"] < CE.REF[n]["bytes"], n      # it ends well, having written the parameter sets and little else


@pytest.mark.parametrize("name", CE.NOT_REFUSED)
def test_oracle_reconstruction_equals_the_reference_decoder(name):
    yuv = E.oracle_i420(CE.parsed(name)[0])
    assert len(yuv) == CE.REF[name]["yuv_bytes"]
    assert E.sha(yuv) == CE.REF[name]["yuv_sha1"]


@pytest.mark.parametrize("name", CE.NOT_REFUSED)
def test_compressed_files_equal_the_references(name):
    main, tags = CE.cpu_compress(name)
    assert CE.same_as_reference_files(name, main, tags)


def test_refused_set():
    why = {n: lh.out_of_range(CE.data(n)) for n in CE.NAMES}
    assert {n for n in CE.NAMES if why[n]} == CE.REFUSED, why
    assert why["cabac_refidx16"].startswith("num_ref_idx_l0_active 16 ") and "0..15" in why["cabac_refidx16"]


# ---- restore -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CE.NOT_REFUSED)
def test_host_restore_returns_the_input(name):
    main, tags = CE.cpu_compress(name)
    assert lh.restore(main, tags) == CE.data(name)


def _cabac_chain(items, threads=0, out_cap=None, statuses=False):
    return R.restore_batch_cpu_check(items, threads, out_cap, statuses, cabac_device=True)


def test_kernel_chain_on_the_host_restores_every_stream():
    """ONE call: every CABAC edge stream and every CAVLC edge stream that compress hands out, on the kernel's chain stepped on the host
    with its CABAC writer: status, length and bytes as lh264_pip_restore_batch, the kernel's path for all, bytes equal to the input"""
    cav = [n for n in E.NAMES if n not in E.REFUSED]
    items = [CE.cpu_compress(n) for n in CE.NOT_REFUSED] + [E.cpu_compress(n) for n in cav]
    want = [CE.data(n) for n in CE.NOT_REFUSED] + [E.data(n) for n in cav]
    paths = RC.check_same(items, _cabac_chain)
    assert paths == [R.PATH_DEVICE] * len(items), dict(zip(CE.NOT_REFUSED + cav, paths))
    outs, _ = _cabac_chain(items, 16)
    for n, o, w in zip(CE.NOT_REFUSED + cav, outs, want):
        assert o == w, n
    # without the flag the CABAC streams are the host's, with the same bytes
    outs, paths = R.restore_batch_cpu_check(items[:len(CE.NOT_REFUSED)], 16)
    assert outs == want[:len(CE.NOT_REFUSED)] and paths == [R.PATH_HOST] * len(CE.NOT_REFUSED)


def test_sixteen_references_need_the_escape_stream():
    """cabac_refidx16 pins the container's range on the CABAC side: without tag 71 its symbols do not give the input back (so compress
    refuses it); with it both restorers return the input, the CABAC writer of the kernel's chain included"""
    d = CE.data("cabac_refidx16")
    main, tags = CE.cpu_compress("cabac_refidx16")
    try:
        back = lh.restore(main, tags)
    except RuntimeError:
        back = None
    assert back != d
    esc = lh.escapes(d)
    assert esc
    tags = dict(tags)
    tags[CE.TAG_ESC] = esc
    assert lh.restore(main, tags) == d
    for cabac_device in (False, True):
        outs, paths, st = R.restore_batch_cpu_check([(main, tags)], 1, None, statuses=True, cabac_device=cabac_device)
        assert st[0][0] == 0 and outs == [d]
        assert paths == [R.PATH_DEVICE if cabac_device else R.PATH_HOST]
