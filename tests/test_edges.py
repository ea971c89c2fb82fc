"""The container's range edges on synthetic CAVLC streams (tests/golden/edge/, written by tests/golden/make_edge_streams.py with the
test writer tests/h264_synth.py): values the reference's corpus never reaches - skip runs around the 9-bit SKIPRUN tree, 16 active
references, levels up to int16 and level_prefix up to 19, mvd around every power of two, qp 41..51 and the mb_qp_delta wrap, I_PCM at
every bit phase, a zero run of 4159 macroblocks in the model's history.

Every edge is asserted twice: from what the writer counted while it wrote, and from what the front end read back.  The reference's
verdict on each stream (tests/golden/edge_ref.json) was taken once from the unmodified reference on the CPU.

The property every restore path must meet on every stream: either compress refuses it, or the restore equals the input.  Everything
here runs without a device; tests/test_edges_gpu.py repeats it through the kernels."""
import numpy as np
import pytest

import edge_cases as E
import losslessh264_amd as lh

R = __import__("sys").modules["losslessh264_amd.restore"]     # the module (lh.restore is the function)

MB_SKIP, MB_IPCM, MB_P16x16, MB_I16x16 = 0x100, 0x200, 0x8, 0x2
TB_SKIPRUN, SYM_TREE = 9, 6
NOT_REFUSED = [n for n in E.NAMES if n not in E.REFUSED]


def test_the_edge_set():
    assert E.NAMES == sorted(["align_bits", "skip511", "skip512", "skip513", "skip_all", "zero_run_4160", "nref_2_3_15", "nref_2_3_15_16", "levels_ref", "levels_ext",
                              "mvd_edges", "qp_edges", "pcm_zero", "pcm_255"])
    biggest = max(len(open(p, "rb").read()) for p in __import__("glob").glob(E.os.path.join(E.golden_io.GOLDEN_DIR, "streams", "*")))
    for n in E.NAMES:
        assert len(E.data(n)) < biggest


@pytest.mark.parametrize("name", E.NAMES)
def test_stream_regenerates_byte_for_byte(name):
    d = E.data(name)
    assert E.made()[name][0] == d
    assert (len(d), E.sha(d)) == (E.REF[name]["bytes"], E.REF[name]["sha1"])


@pytest.mark.parametrize("name", E.NAMES)
def test_front_end_parses(name):
    frames, err, main, pcm = E.parsed(name)
    assert err == ""
    assert len(frames) == E.made()[name][1]["pictures"] == E.REF[name]["pictures"]
    for f in frames:
        assert f.covered.all()


def _read_skip_runs(name):
    """the longest run of each picture as the front end read it: the values of its SKIPRUN symbols (a run that ends its slice has
    no macroblock record to carry syn['skip_run'])"""
    out = []
    for f in E.parsed(name)[0]:
        s = f.syn_syms
        out.append(int(s["value"][(s["kind"] == SYM_TREE) & (s["prior"] >> 27 == TB_SKIPRUN)].max(initial=0)))
    return out


@pytest.mark.parametrize("name,longest", [("skip511", 511), ("skip512", 512), ("skip513", 513), ("skip_all", 1200)])
def test_skip_run_edges(name, longest):
    c = E.made()[name][1]
    assert max(c["skip_runs"]) == longest and c["mbs"] == 1200
    if name == "skip_all":
        assert c["skip_runs"] == [1200]                       # the run ends the slice: no macroblock follows it
    else:
        assert c["skip_runs"][0] == longest and len(c["skip_runs"]) > 1      # a coded macroblock follows
    frames = E.parsed(name)[0]
    assert _read_skip_runs(name) == [0, longest]
    p = frames[1]
    assert int((p.mbs["mb_type"] == MB_SKIP).sum()) == sum(c["skip_runs"])
    if name != "skip_all":
        assert int(p.syn["skip_run"].max()) == int(p.syn["skip_run"][longest]) == longest
        assert p.mbs["mb_type"][longest] == MB_P16x16 and (p.mbs["mb_type"][:longest] == MB_SKIP).all()


def test_zero_run_4160_reads_a_prior_index_of_512_times_16():
    c = E.made()["zero_run_4160"][1]
    assert max(c["skip_runs"]) == 416 and c["mbs"] == 4160 and c["skip_runs"].count(416) == 19 and c["skip_runs"].count(415) == 1
    frames = E.parsed("zero_run_4160")[0]
    assert max(_read_skip_runs("zero_run_4160")) == 416
    assert [int((f.mbs["mb_type"] == MB_SKIP).sum()) for f in frames] == [0, 4159, 4160]
    s = frames[2].syn_syms
    runs = s[(s["kind"] == SYM_TREE) & (s["prior"] >> 27 == TB_SKIPRUN)]
    idx = runs["prior"] & 0x7ffffff
    assert len(runs) == 10 and int(idx.max()) >= 512 * 16
    assert int(idx.max()) == ((4159 + 7) // 8) * 16 + 11       # the run of 4159 zeroed macroblocks in front of picture 2's last one
    assert all(int((f.syn_syms["prior"][(f.syn_syms["kind"] == SYM_TREE) & (f.syn_syms["prior"] >> 27 == TB_SKIPRUN)] & 0x7ffffff).max(initial=0)) < 512 * 16
               for f in frames[:2])


@pytest.mark.parametrize("name,most", [("nref_2_3_15", 15), ("nref_2_3_15_16", 16)])
def test_num_ref_idx_edges(name, most):
    """nref_2_3_15 is nref_2_3_15_16 without its last two pictures, those of 16 references: it is not refused, so 2 (the inverted
    one-bit ref_idx), 3 and 15 references go through the file comparison and every restore path"""
    c = E.made()[name][1]
    for n in (2, 3, 15, 16)[:3 if most == 15 else 4]:
        assert c["num_ref_idx"][n] == n - 1                    # the highest ref_idx of each
    assert max(c["num_ref_idx"]) == most
    assert E.data("nref_2_3_15_16").startswith(E.data("nref_2_3_15"))
    frames = E.parsed(name)[0]
    assert len(frames) == most + 2 - (most == 15)
    got = {}
    for f in frames[1:]:
        coded = f.syn["mb_type"] == MB_P16x16
        assert coded.all()
        n = set(int(x) for x in f.syn["num_ref_idx_l0"])
        assert len(n) == 1
        n = n.pop()
        got[n] = max(got.get(n, 0), int(f.syn["ref_idx"][:, 0].max()))
        assert int(f.mbs["ref_idx"][:, 0].max()) == n - 1
    assert got == {n: n - 1 for n in range(1, most + 1)}
    assert [int(f.syn["num_ref_idx_l0"][0]) for f in frames[1:]] == ([1] + list(range(2, 17)) + [16])[:len(frames) - 1]


def _largest_prefix15_level(sl):
    """the level of the largest levelCode level_prefix 15 holds at suffixLength sl (12 suffix bits).  At suffixLength 0 the level is the
    first of its block, behind fewer than 3 trailing ones, which adds 2 to the code (9.2.2.1)"""
    code = (15 << sl) + (15 if sl == 0 else 0) + 4095 + (2 if sl == 0 else 0)
    return (code + 2) // 2 if code % 2 == 0 else -((code + 1) // 2)


@pytest.mark.parametrize("name", ["levels_ref", "levels_ext"])
def test_level_edges(name):
    c = E.made()[name][1]
    ext = name == "levels_ext"
    for sl in range(7):
        for prefix in ((16, 17, 18, 19) if ext else (13, 14, 15)):
            assert c["prefix"].get((prefix, sl), 0) >= 2, (prefix, sl)      # once in an Intra16x16 DC block, once in a P luma block
    frames = E.parsed(name)[0]
    lv = np.concatenate([f.levels.ravel() for f in frames]).astype(np.int64)
    assert (int(lv.min()), int(lv.max())) == (c["level_min"], c["level_max"])
    if ext:
        assert (c["level_min"], c["level_max"]) == (-32768, 32767)
        assert max(p for p, _ in c["prefix"]) == 19
        for v in (32767, -32767, -32768):
            assert int((lv == v).sum()) == 4                  # suffixLength 0 and 6, I and P
        return
    assert max(p for p, _ in c["prefix"]) == 15
    for sl in (0, 6):
        v = _largest_prefix15_level(sl)
        assert v == (-2064 if sl == 0 else -2528) and int((lv == v).sum()) == 2, (sl, v)
    assert (c["level_min"], c["level_max"]) == (-2528, 2528)
    tok = c["coeff_token"]
    for cls in range(4):                                       # nC 0-1, 2-3, 4-7, 8 and up
        assert any(k[:3] == (cls, 16, 16) for k in tok), cls
        assert any(k[:3] == (cls, 15, 15) for k in tok), cls
    assert any(k[:3] == (4, 4, 4) for k in tok)                # chroma DC
    assert all(any(k[2] > 10 and k[3] == t1 for k in tok) for t1 in range(3))
    assert c["run_before"].get((7, 14), 0) >= 1                # zerosLeft > 6 and a run of 14
    for total in range(1, 16):
        assert c["total_zeros"][(16, total)] == 16 - total
    for total in range(1, 4):
        assert c["total_zeros"][(4, total)] == 4 - total
    # read back: the blocks of the total_zeros macroblock hold i + 1 levels at the high end of the scan
    nz = (frames[1].levels.reshape(-1, 24, 16) != 0)
    assert any(sorted(int(nz[k, b].sum()) for b in range(16)) == sorted(list(range(1, 16)) + [2]) for k in range(nz.shape[0]))
    assert max(int(nz[k, :16].sum(axis=1).max()) for k in range(nz.shape[0])) == 16


def test_mvd_edges():
    c = E.made()["mvd_edges"][1]
    want = set()
    for k in range(14):
        want |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    want = (want | {10, 11}) - {0}                           # 9 | 10: where the coder's binarisation goes from unary to exp-Golomb
    assert {9, 10, 8191, 8192, 8193} <= want
    assert (c["mvd_min"], c["mvd_max"]) == (-8193, 8193)
    p = E.parsed("mvd_edges")[0][1]
    assert (p.syn["mb_type"] == MB_P16x16).all()
    mvd = p.syn["mvd"][:, 0, :].astype(np.int64)
    assert set(int(x) for x in mvd[:, 0]) == want | {-v for v in want} == set(int(x) for x in mvd[:, 1])
    mv = p.mbs["mv"][:, 0, :].astype(np.int64)
    assert (int(mv.min()), int(mv.max())) == (0, 8193)         # +v then -v: the vector returns to 0, inside int16
    assert np.array_equal(mv[0::2, 0], np.array(sorted(want))) and not mv[1::2].any()


def test_qp_edges():
    c = E.made()["qp_edges"][1]
    assert (c["qp_min"], c["qp_max"], c["dqp_min"], c["dqp_max"]) == (0, 51, -26, 25)
    frames = E.parsed("qp_edges")[0]
    qp, want = 41, []
    for d in [0] + [1] * 10 + [1, -26, 25, 25, -26]:
        qp = (qp + d + 52) % 52
        want.append(qp)
    assert want == list(range(41, 52)) + [0, 26, 51, 24, 50]
    assert [int(x) for x in frames[0].mbs["qp_y"]] == want
    qp, want = 45, []
    for d in [6, 1, -26, 25, 25, -26, 1]:
        qp = (qp + d + 52) % 52
        want.append(qp)
    assert want == [51, 0, 26, 51, 24, 50, 51]
    assert [int(x) for x in frames[1].mbs["qp_y"][:7]] == want
    assert [int(s["deblock_idc"]) for f in frames for s in f.slices] == [0, 0]


@pytest.mark.parametrize("name,sample", [("pcm_zero", 0), ("pcm_255", 255)])
def test_pcm_edges(name, sample):
    c = E.made()[name][1]
    assert c["pcm_phase"] == set(range(8))
    frames, err, main, pcm = E.parsed(name)
    assert len(frames) == 9 and pcm == bytes([sample]) * (8 * 384)
    for f in frames[1:]:
        t = [int(x) for x in f.mbs["mb_type"]]
        assert t.count(MB_IPCM) == 1 and t[0] == MB_SKIP and all(x in (MB_SKIP, MB_IPCM) for x in t)      # I_PCM after a skip run
    if sample == 0:
        assert c["epb"] >= 8 * 191                             # 384 zero bytes: an emulation prevention byte behind every two
        assert E.data(name).count(b"\x00\x00\x03\x00\x00\x03\x00\x00\x03") > 0
    else:
        assert c["epb"] == 0


def test_alignment_bit_edges():
    """1..7 alignment bits behind the stop bit of a slice that ends its picture, all ones, behind a coded macroblock and behind a run"""
    c = E.made()["align_bits"][1]
    assert c["align"] == {(n, (1 << n) - 1) for n in range(8)}
    frames = E.parsed("align_bits")[0]
    read = {}
    for f in frames[1:]:
        ends_in_run = int(f.mbs["mb_type"][-1]) == MB_SKIP
        read.setdefault(ends_in_run, set()).add((int(f.slice_syn[0, 0]), int(f.slice_syn[0, 1])))
    assert read == {False: c["align"], True: c["align"]}


# ---- against the reference's verdict ------------------------------------------------------------------------------------------------
def test_reference_verdict_as_recorded():
    """what the unmodified reference did with the streams: it decodes all but levels_ext (level_prefix above 15), nref_2_3_15_16 and
    zero_run_4160 (its console application aborts on both); its own round trip holds for skip511, mvd_edges and nref_2_3_15 only.
    Of nref_2_3_15_16 it wrote the 16 pictures in front of the first one with 16 references: the pictures of nref_2_3_15"""
    assert E.REF["align_bits"]["reference_decodes"] and not E.REF["align_bits"]["reference_roundtrip"]
    assert {n for n in E.NAMES if E.REF[n]["reference_decodes"]} == set(E.NAMES) - {"levels_ext", "nref_2_3_15_16", "zero_run_4160"}
    assert {n for n in E.NAMES if E.REF[n]["reference_roundtrip"]} == {"skip511", "mvd_edges", "nref_2_3_15"}
    long, short = E.REF["nref_2_3_15_16"], E.REF["nref_2_3_15"]
    assert (long["yuv_bytes"], long["yuv_sha1"]) == (short["yuv_bytes"], short["yuv_sha1"]) == (16 * 4 * 384, short["yuv_sha1"])


@pytest.mark.parametrize("name", [n for n in E.NAMES if E.REF[n]["reference_decodes"]])
def test_oracle_reconstruction_equals_the_reference_decoder(name):
    frames = E.parsed(name)[0]
    yuv = E.oracle_i420(frames)
    assert len(yuv) == E.REF[name]["yuv_bytes"]
    assert E.sha(yuv) == E.REF[name]["yuv_sha1"]


@pytest.mark.parametrize("name", [n for n in E.NAMES if E.REF[n]["reference_decodes"]])
def test_compressed_files_equal_the_references(name):
    """host symbols + the oracle's coefficient symbols through the oracle's coder: the reference's files, for every stream it decoded
    to the end - those its own round trip held for (skip511, mvd_edges, nref_2_3_15), those its restore fails on, and those it codes
    modulo the table (skip512, skip513, skip_all: the same bytes, which is why they are refused).  align_bits: see edge_cases.FILES_DIFFER"""
    main, tags = E.cpu_compress(name)
    assert E.same_as_reference_files(name, main, tags)


def test_refused_set():
    """a stream with a value the prior tables cannot carry is marked by the front end (and refused by lh264_compress_batch, see
    tests/test_edges_gpu.py); the mark names the field and the value"""
    why = {n: lh.out_of_range(E.data(n)) for n in E.NAMES}
    assert {n for n in E.NAMES if why[n]} == E.REFUSED, why
    assert why["skip511"] == ""
    assert why["skip512"].startswith("mb_skip_run 512 ") and why["skip513"].startswith("mb_skip_run 513 ") and why["skip_all"].startswith("mb_skip_run 1200 ")
    assert why["nref_2_3_15_16"].startswith("num_ref_idx_l0_active 16 ")
    for n in E.REFUSED:
        assert "0..511" in why[n] or "0..15" in why[n]
    # every corpus stream stays inside the range
    import glob
    for p in sorted(glob.glob(E.os.path.join(E.golden_io.GOLDEN_DIR, "streams", "*"))):
        assert lh.out_of_range(open(p, "rb").read()) == "", p


@pytest.mark.parametrize("name", NOT_REFUSED)
def test_restore_returns_the_input(name):
    """the host restore and the kernel's code stepped on the host, on what the compress direction computes"""
    main, tags = E.cpu_compress(name)
    d = E.data(name)
    assert lh.restore(main, tags) == d
    outs, paths, st = R.restore_batch_cpu_check([(main, tags)], 1, None, statuses=True)
    assert paths == [R.PATH_DEVICE], (paths, st)
    assert st[0][0] == 0 and outs[0] == d


@pytest.mark.parametrize("name", sorted(E.REFUSED))
def test_a_refused_stream_never_restores_to_other_bytes_unnoticed(name):
    """what the refusal protects from: the symbols of these streams, coded all the same, do not give the input back (an error, or other
    bytes) - so compress must not hand them out.  Should a later extension carry the value, this test and REFUSED change together"""
    frames, err, main, pcm = E.parsed(name)
    assert err == "" and lh.out_of_range(E.data(name)) != ""
    main, tags = E.cpu_compress(name)
    try:
        back = lh.restore(main, tags)
    except RuntimeError:
        back = None
    assert back != E.data(name)
