"""Extra parity cases of the reconstruct kernel for the paths whose work is split across both halves of a wave: chroma motion
compensation (one chroma pair per lane) under many small partitions and weighted prediction, and the deblocking filter with
differing Cb / Cr QPs in intra macroblocks and nonzero alpha / beta offsets.  Streams from tests/synth.py, reshaped, against the oracle."""
import numpy as np
import pytest

import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu

INTER = (synth.P16, synth.P16x8, synth.P8x16, synth.P8x8, synth.P8x8R0)
INTRA = (synth.I4, synth.I16, synth.I8, synth.IPCM)


def _oracle(frames):
    pics, out = {}, []
    for f in frames:
        dst = O.HostPic(f.mb_w, f.mb_h)
        O.recon_frame(f.mbs, f.coeffs, f.slices, dst, [pics[r] for r in f.ref_ids], 0)
        pics[f.id] = dst
        out.append(dst)
    return out


def _to_sub_partitions(frames, seed):
    """every coded inter macroblock becomes P8x8 with random sub-partitions (mostly 4x4) and one vector per 4x4 block of a partition"""
    rng = np.random.default_rng(seed)
    for f in frames:
        for m in f.mbs:
            if int(m["mb_type"]) not in INTER:
                continue
            m["mb_type"] = synth.P8x8
            m["flags"] = int(m["flags"]) & ~1
            nref = max(int(f.slices[int(m["slice_id"])]["n_refs"]), 1)
            mv = np.zeros((16, 2), dtype=np.int16)
            for q in range(4):
                st = int(rng.choice([1, 2, 4, 8, 8, 8]))
                m["sub_type"][q] = st
                m["ref_idx"][q] = int(rng.integers(0, nref))
                vs = [rng.integers(-70, 71, 2) for _ in range(4)]
                for j in range(4):
                    jx, jy = j & 1, j >> 1
                    b4 = ((q >> 1) * 2 + jy) * 4 + (q & 1) * 2 + jx
                    mv[b4] = vs[0] if st == 1 else vs[jy] if st == 2 else vs[jx] if st == 4 else vs[j]
            m["mv"] = mv
    return frames


def _chroma_qp_spread(frames, seed, offsets):
    """intra macroblocks get Cb / Cr QPs far apart; every slice gets the given nonzero alpha / beta offsets"""
    rng = np.random.default_rng(seed)
    for f in frames:
        for s in f.slices:
            s["alpha_c0_offset"], s["beta_offset"] = offsets
        for m in f.mbs:
            if int(m["mb_type"]) in INTRA:
                qp = int(m["qp_y"])
                m["qp_c"] = (min(51, max(0, qp + int(rng.integers(-12, 13)))), min(51, max(0, qp + int(rng.integers(-12, 13)))))
    return frames


def _run(frames):
    import losslessh264_amd as lh
    sess = lh.ReconSession([frames])
    sess.run(); sess.synchronize()
    want = _oracle(frames)
    for i in range(len(frames)):
        got = sess.picture(0, i, padded=True)
        for p in range(3):
            ref = want[i].padded_plane(p)
            assert np.array_equal(got[p], ref), "frame %d plane %d: %d samples differ" % (i, p, int(np.count_nonzero(got[p] != ref)))


# the streams of the tests below (tests/test_deblock_directed.py counts what their filter lines reach)
SUB_PARTITION_SEEDS, SUB_PARTITION_WEIGHTED_SEEDS, WEIGHTED_SEEDS = [101, 102, 103], [111, 112], [121, 122]
CHROMA_QP_CASES = [(131, (6, 6)), (132, (-6, 4)), (133, (4, -6))]


def sub_partition_stream(seed):
    return _to_sub_partitions(synth.make_stream(seed=seed, mb_w=9, mb_h=7, n_frames=4), seed)


def sub_partition_weighted_stream(seed):
    return _to_sub_partitions(synth.make_stream(seed=seed, mb_w=8, mb_h=6, n_frames=4, weighted=True), seed)


def weighted_stream(seed):
    return synth.make_stream(seed=seed, mb_w=11, mb_h=9, n_frames=4, weighted=True, density=0.2)


def chroma_qp_stream(seed, offsets):
    frames = synth.make_stream(seed=seed, mb_w=10, mb_h=8, n_frames=3, t8=(seed % 2 == 0), pcm=(seed == 133))
    return _chroma_qp_spread(frames, seed, offsets)


@pytest.mark.parametrize("seed", SUB_PARTITION_SEEDS)
def test_sub_partitions(seed):
    _run(sub_partition_stream(seed))


@pytest.mark.parametrize("seed", SUB_PARTITION_WEIGHTED_SEEDS)
def test_sub_partitions_weighted(seed):
    _run(sub_partition_weighted_stream(seed))


@pytest.mark.parametrize("seed", WEIGHTED_SEEDS)
def test_weighted_prediction(seed):
    _run(weighted_stream(seed))


@pytest.mark.parametrize("seed,offsets", CHROMA_QP_CASES)
def test_chroma_qp_and_filter_offsets(seed, offsets):
    _run(chroma_qp_stream(seed, offsets))
