"""The motion fields of lh264_decode_batch_ex4 (include/lh264.h at that call) in numpy, over what the host front end returns
(parse_file: mbs, slices, id, ref_ids and a frame's position in the list).  Written from the definition, not from the kernel."""
import numpy as np

MB_INTRA = 0x0001 | 0x0002 | 0x0004 | 0x0200
MB_CONCEAL = 0x0400
# kind: the first of these bits that mb_type has
KIND_BITS = [(0x0001, 1), (0x0004, 2), (0x0002, 3), (0x0200, 4), (0x0100, 5), (0x0008, 6), (0x0010, 7), (0x0020, 8), (0x0040, 9), (0x0080, 10)]
QUAD_OF_BLOCK = [(b >> 3) * 2 + ((b & 3) >> 1) for b in range(16)]


def kinds(mb_type):
    t = np.asarray(mb_type).astype(np.int64)
    k = np.zeros(t.shape, np.int64)
    for bit, kind in reversed(KIND_BITS):
        k = np.where(t & bit, kind, k)
    return k


def picture_fields(mbs, slices, mb_w, mb_h, back):
    """one picture: its mb_w * mb_h records (L.MB_DTYPE), its slice table (L.SLICE_DTYPE), back[slot] for the 16 job reference slots
    -> (motion (3, 4 * mb_h, 4 * mb_w) int16, info (8, mb_h, mb_w) uint8)"""
    n = mb_w * mb_h
    assert len(mbs) == n and len(back) == 16
    back = np.asarray(back, np.int64)
    t = mbs["mb_type"].astype(np.int64)
    kind = kinds(t)
    inter = kind >= 5
    conceal = (t & MB_CONCEAL) != 0
    mv = mbs["mv"].astype(np.int64)                                     # (n, 16, 2)
    mv = np.where(conceal[:, None, None], mv[:, 0:1, :], mv)
    r = mbs["ref_idx"].astype(np.int64)                                 # (n, 4)
    sid = mbs["slice_id"].astype(np.int64)
    ok = (r >= 0) & (r < 16) & (sid[:, None] < len(slices))
    if len(slices):
        slot = slices["ref_slot"].astype(np.int64)[np.clip(sid, 0, len(slices) - 1)[:, None], np.clip(r, 0, 15)]
    else:
        slot = np.full(r.shape, -1, np.int64)
    ok &= (slot >= 0) & (slot < 16)
    bq = np.where(ok, back[np.clip(slot, 0, 15)], -1)                   # (n, 4)
    cells = np.stack([mv[:, :, 0], mv[:, :, 1], bq[:, QUAD_OF_BLOCK]])  # (3, n, 16)
    cells = np.where(inter[None, :, None], cells, 0)
    motion = cells.reshape(3, mb_h, mb_w, 4, 4).transpose(0, 1, 3, 2, 4).reshape(3, 4 * mb_h, 4 * mb_w).astype(np.int16)
    info = np.zeros((8, n), np.int64)
    info[0], info[1], info[2] = kind, mbs["qp_y"], mbs["cbp"]
    info[3] = (mbs["flags"].astype(np.int64) & 1) | (conceal.astype(np.int64) << 1)
    sub = (kind == 9) | (kind == 10)
    for k in range(4):
        info[4 + k] = np.where(sub, mbs["sub_type"][:, k], 0)
    return motion, info.reshape(8, mb_h, mb_w).astype(np.uint8)


def back_table(frames, k):
    """back[slot] of frames[k]: its position in the list minus that of the picture behind job reference `slot`; -1: no decoded picture"""
    pos = {f.id: i for i, f in enumerate(frames[:k])}
    back = [-1] * 16
    for slot, pid in enumerate(frames[k].ref_ids[:16]):
        if pid in pos:
            back[slot] = k - pos[pid]
    return back


def stream_fields(frames, intra_only=False):
    """[(motion, info)] per frame of parse_file's list (withheld ones included: the caller drops them).  intra_only: the frames are
    those of a pick= call, which holds no reference: every back is -1 (and every delivered picture intra)"""
    out = []
    for k, f in enumerate(frames):
        back = [-1] * 16 if intra_only else back_table(frames, k)
        out.append(picture_fields(f.mbs, f.slices, f.mb_w, f.mb_h, back))
    return out
