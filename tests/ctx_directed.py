"""Directed inputs for the context-index kernels (csrc/lh264_ctx.hip): the case builders, what the kernels must answer, the coverage
measures and a small device stager.  tests/test_ctx_directed.py shows on the CPU that the cases reach what they claim,
tests/test_ctx_directed_gpu.py runs the kernels against the expectation.

The expectation is the oracle (oracle_lib.model_nnz_images / model_frame_symbols).  Where the oracle is silent the rule is restated
here in numpy: the symbol's tag (`pad`), the KEEP rule of pictures with lost slices, and the arithmetic of the compact pool.

Every input obeys the parser's contract: levels are zero wherever cbp says "not coded", except the DCs of an Intra16x16 or chroma-DC-only
macroblock (contract_violations)."""
import numpy as np

import oracle_lib as O
from refdump import MB_DTYPE, SLICE_DTYPE

I4, I16, I8, P16, SKIP, IPCM = 1, 2, 4, 8, 0x100, 0x200
LDC, CDC, NZ4, AC4, NZ8, AC8 = range(6)
MAX_SYMS = 432
SYM = O.ORC_SYM_DTYPE
POOL_FILL, GUARD = 0xA5, 64          # what an unwritten symbol byte holds; symbols behind the pool that nothing may touch


def _zigzag(n):
    """raster indices of an n x n block in zig-zag order (even diagonals run up, odd ones down)"""
    return [r for _, _, r in sorted(((x + y, x if (x + y) % 2 == 0 else -x, y * n + x) for y in range(n) for x in range(n)))]


ZZ16 = _zigzag(4)                                  # scan position -> index into the block's 16 levels
ZZ64 = [_zigzag(8).index(r) for r in range(64)]    # scan position -> index into the 64 levels (the reference's kzz64 is the inverse table)
INV16 = [ZZ16.index(r) for r in range(16)]         # index into the levels -> scan position: what the count pass works from
INV64 = [ZZ64.index(r) for r in range(64)]


# ---- pictures ---------------------------------------------------------------------------------------------------------------------------
class Frame:
    pass


def new_frame(mb_w, mb_h, frame_num=0, slice_types=(0,), slice_of=None):
    """a picture of P16x16 macroblocks with nothing coded (no symbols, counts zero); slice_of: slice index per macroblock"""
    f = Frame()
    n = mb_w * mb_h
    f.mb_w, f.mb_h, f.frame_num = mb_w, mb_h, frame_num
    f.mbs = np.zeros(n, dtype=MB_DTYPE)
    f.mbs["mb_type"] = P16
    f.mbs["qp_y"] = 26
    f.mbs["slice_id"] = 0 if slice_of is None else slice_of
    f.slices = np.zeros(len(slice_types), dtype=SLICE_DTYPE)
    f.slices["slice_type"] = slice_types
    f.slices["n_refs"] = 1
    for s in range(len(slice_types)):
        ks = np.flatnonzero(f.mbs["slice_id"] == s)
        f.slices["first_mb"][s], f.slices["n_mbs"][s] = (ks[0], len(ks)) if len(ks) else (0, 0)
    f.levels = np.zeros((n, 384), dtype=np.int16)
    f.covered = np.ones(n, dtype=np.uint8)
    return f


def mask_to_cbp(lv, typ, cbpl, cbpc):
    """zero what cbp says is not coded, as the parser leaves it (the rule of synth.make_stream)"""
    for s in range(4):
        if not (cbpl >> s) & 1:
            dc = lv[s * 64:(s + 1) * 64:16].copy()
            lv[s * 64:(s + 1) * 64] = 0
            if typ == I16:
                lv[s * 64:(s + 1) * 64:16] = dc
    if cbpc == 0:
        lv[256:] = 0
    elif cbpc == 1:
        dc = lv[256::16].copy()
        lv[256:] = 0
        lv[256::16] = dc
    return lv


def put_mb(f, k, typ, cbpl=0, cbpc=0, t8=False, levels=None):
    m = f.mbs[k]
    m["mb_type"], m["cbp"], m["flags"] = typ, cbpl | cbpc << 4, 1 if t8 else 0
    f.levels[k] = 0 if levels is None else levels
    if typ == 0:
        f.covered[k] = 0


def contract_violations(f):
    """macroblocks whose levels are not what the parser would leave for their cbp"""
    bad = []
    for k in range(f.mb_w * f.mb_h):
        typ, cbp = int(f.mbs["mb_type"][k]), int(f.mbs["cbp"][k])
        if typ == IPCM:
            continue
        want = np.zeros(384, np.int16) if typ in (SKIP, 0) else mask_to_cbp(f.levels[k].copy(), typ, cbp & 15, cbp >> 4)
        if not np.array_equal(want, f.levels[k]) or (typ in (SKIP, 0) and cbp) or ((int(f.mbs["flags"][k]) & 1) and typ == I16):
            bad.append(k)
    return bad


class Batch:
    """the pictures of one call: chains of frames; past[c][i]: index in the chain or None (default: the host's policy);
    keep: None (the plain calls) or keep[c][i] = None | index of an earlier picture of the chain | uint8[n, 24] of the caller's;
    fixed: the (chain, picture) pairs in the FIXED layout; targets: (chain, picture, macroblock, what) the case is about"""

    def __init__(self, name, chains, past=None, keep=None, fixed=(), max_mbs=None):
        import losslessh264_amd as lh
        self.name, self.chains = name, chains
        self.past = past if past is not None else [lh.past_policy(ch) for ch in chains]
        self.keep, self.fixed = keep, set(fixed)
        self.max_mbs = max_mbs or max(f.mb_w * f.mb_h for ch in chains for f in ch)
        self.targets = []

    def jobs(self):
        return [(c, i, f) for c, ch in enumerate(self.chains) for i, f in enumerate(ch)]

    def with_layout(self, fixed):
        b = Batch(self.name, self.chains, self.past, self.keep, fixed, self.max_mbs)
        b.targets = self.targets
        return b


# ---- what the kernels must answer -------------------------------------------------------------------------------------------------------
def blocks_of(f, k, syms):
    """the coded blocks of macroblock k in emission order, from the macroblock's record and the oracle's list:
    [(b, n, start, at, nz, n_ac)]  b: storage index of the (first) 4x4 block, n: 16 or 64, start: first scan position that is a symbol,
    at: index of the block's nonzero-count symbol in the list, nz: its value, n_ac: the coefficient symbols behind it"""
    typ, cbp, t8 = int(f.mbs["mb_type"][k]), int(f.mbs["cbp"][k]), int(f.mbs["flags"][k]) & 1
    if typ in (SKIP, IPCM, 0):
        assert len(syms) == 0
        return []
    cbpl, cbpc, i16 = cbp & 15, cbp >> 4, typ == I16
    order = []
    for s in range(4):
        if (cbpl >> s) & 1:
            order += [(s * 4, 64, 0)] if t8 else [(s * 4 + j, 16, 1 if i16 else 0) for j in range(4)]
    if cbpc == 2:
        order += [(16 + i, 16, 1) for i in range(8)]
    at = (16 if i16 else 0) + (8 if cbpc in (1, 2) else 0)
    kinds = syms["kind"]
    assert np.all(kinds[:16 if i16 else 0] == LDC) and np.all(kinds[16 if i16 else 0:at] == CDC)
    out = []
    for b, n, start in order:
        assert kinds[at] == (NZ4 if n == 16 else NZ8), (k, b, at)
        e = at + 1
        while e < len(syms) and kinds[e] == (AC4 if n == 16 else AC8):
            e += 1
        out.append((b, n, start, at, int(syms["value"][at]), e - at - 1))
        at = e
    assert at == len(syms), (k, at, len(syms))
    return out


def tags_of(f, k, syms):
    """the pad byte of every symbol of the list: the tag its decisions are billed to (encode4x4) - from the symbol's place in the list"""
    pad = np.zeros(len(syms), dtype=np.uint8)
    i16 = int(f.mbs["mb_type"][k]) == I16
    pad[syms["kind"] == LDC] = 17
    pad[syms["kind"] == CDC] = 18
    for b, n, start, at, nz, n_ac in blocks_of(f, k, syms):
        pad[at] = 29 if b >= 16 else 19
        pad[at + 1:at + 1 + n_ac] = 29 if b >= 16 else 24
        if b < 16 and not i16 and n_ac:
            pad[at + 1] = 19
    return pad


def ac_tag_base(prior, kind):
    """lh264_coder_dev.h ac_tag_base (prior, kind, 0): the tag taken out of the prior"""
    nco = 16 if kind == AC4 else 64
    outer = prior // 3125
    emitted, color, code = outer % nco, (outer // nco) % 3, (outer // nco // 3) % 16
    return 29 if color else (19 if (emitted == 0 and code != 1) else 24)


def nz_tag(prior):
    """lh264_coder_dev.h nz_tag (prior, 0)"""
    return 29 if (prior // 27) % 3 else 19


def nnz24(lv):
    return (np.asarray(lv).reshape(24, 16) != 0).sum(axis=1).astype(np.uint8)


def nnz_images(frames, past, keep=None):
    """the nnz images by the KEEP rule (tolerant_cases.cpu_compress): a macroblock of type 0 takes the KEEP entry (zeros where there is
    none), a skipped one the PAST entry.  keep None: the plain calls, where type 0 takes PAST like a skipped one"""
    imgs = []
    for i, f in enumerate(frames):
        n = f.mb_w * f.mb_h
        img = np.zeros((n, 24), dtype=np.uint8)
        kp = past[i] if keep is None else keep[i]
        for k in range(n):
            t = int(f.mbs["mb_type"][k])
            if t in (SKIP, 0):
                src = past[i] if t == SKIP else kp
                if src is not None:
                    img[k] = (imgs[src] if isinstance(src, (int, np.integer)) else np.asarray(src).reshape(n, 24))[k]
            else:
                img[k] = nnz24(f.levels[k])
        imgs.append(img)
    return imgs


class Exp:
    """one picture's answer: img uint8[n, 24]; syms: the oracle's list per macroblock with pad filled in; n, off, total: the compact
    layout's counts, dense offsets and the picture's total"""

    def __init__(self, f, img, past_img):
        self.img, self.past_img = img, past_img
        self.syms = O.model_frame_symbols(f, img, past_img)
        for k, s in enumerate(self.syms):
            s["pad"] = tags_of(f, k, s)
        self.n = np.array([len(s) for s in self.syms], dtype=np.int64)
        self.off = np.cumsum(self.n) - self.n
        self.total = int(self.n.sum())
        self.flat = np.concatenate(self.syms) if self.total else np.zeros(0, SYM)


_expect_cache = {}


def expect(batch):
    """-> one Exp per job, in job order; computed once per batch name and never written to afterwards"""
    key = (batch.name, batch.keep is not None)
    if key not in _expect_cache:
        out = []
        for c, ch in enumerate(batch.chains):
            past = batch.past[c]
            if batch.keep is None:
                imgs = O.model_nnz_images(ch, past)
            else:
                imgs = nnz_images(ch, past, batch.keep[c])
            for i, f in enumerate(ch):
                out.append(Exp(f, imgs[i], imgs[past[i]] if past[i] is not None else None))
        _expect_cache[key] = out
    return _expect_cache[key]


def bases(batch, exps):
    """*sym_base of every job (fixed jobs count as 0) and the grand total"""
    tot = np.array([0 if (c, i) in batch.fixed else e.total for (c, i, _), e in zip(batch.jobs(), exps)], dtype=np.int64)
    return np.cumsum(tot) - tot, int(tot.sum())


# ---- level builders ---------------------------------------------------------------------------------------------------------------------
def _nzval(rng, amp):
    return int(rng.integers(1, amp + 1)) * (1 if rng.random() < 0.5 else -1)


def set_scan(lv, b, n, positions, rng, amp=3):
    """nonzero levels at the given scan positions of 4x4 block b (n 16) or of the 8x8 block that starts at storage index b (n 64)"""
    for p in positions:
        lv[b * 16 + (ZZ16[p] if n == 16 else ZZ64[p])] = _nzval(rng, amp)


def sparse_mb(rng, typ, t8, counts=(0, 1, 2), amp=3):
    """every block of the macroblock with a number of nonzero levels drawn from `counts`, none of them a separately coded DC"""
    lv = np.zeros(384, dtype=np.int16)
    if t8:
        for s in range(4):
            set_scan(lv, s * 4, 64, rng.choice(64, int(rng.choice(counts)), replace=False), rng, amp)
    else:
        st = 1 if typ == I16 else 0
        for b in range(16):
            set_scan(lv, b, 16, st + rng.choice(16 - st, int(rng.choice(counts)), replace=False), rng, amp)
    for b in range(16, 24):
        set_scan(lv, b, 16, 1 + rng.choice(15, int(rng.choice(counts)), replace=False), rng, amp)
    return lv


def ending_at(rng, b, n, start, last, lv, amp=3, fill=0.5):
    """block with its last nonzero level at scan position `last` (-1: none) and random ones before it"""
    if last < start:
        return
    ps = [p for p in range(start, last) if rng.random() < fill] + [last]
    set_scan(lv, b, n, ps, rng, amp)


def sparse_picture(rng, mb_w, mb_h, frame_num, st, types, t8=False, counts=(0, 1, 2), skip=(), slice_types=None, slice_of=None):
    f = new_frame(mb_w, mb_h, frame_num, slice_types if slice_types is not None else (st,), slice_of)
    for k in range(mb_w * mb_h):
        if k in skip:
            put_mb(f, k, SKIP)
            continue
        typ = int(rng.choice(types))
        use8 = t8 and typ != I16
        put_mb(f, k, typ, 15, 2, use8, sparse_mb(rng, typ, use8, counts))
    return f


def single_pictures(name, mbs):
    """mbs: [(what, typ, cbpl, cbpc, t8, levels)] -> a batch of one-picture chains of 4 (2x2) or 5 (5x1) macroblocks, one case each at a
    place that moves through the picture; the others have nothing coded"""
    chains, targets = [], []
    for j, (what, typ, cbpl, cbpc, t8, lv) in enumerate(mbs):
        w, h = ((2, 2), (5, 1))[j & 1]
        f = new_frame(w, h, 0, (0 if typ == P16 else 2,))
        k = (j // 2) % (w * h)
        put_mb(f, k, typ, cbpl, cbpc, t8, lv)
        chains.append([f])
        targets.append((j, 0, k, what))
    b = Batch(name, chains)
    b.targets = targets
    return b


# ---- family 1: the last position, raster against scan -----------------------------------------------------------------------------------
FULL_P, FULL_I16, FULL_T8 = 408, 408, 396


def family_last_position():
    rng = np.random.default_rng(101)
    mbs = []
    for r in range(16):
        lv = np.zeros(384, np.int16); lv[(r % 16) * 16 + r] = _nzval(rng, 9)
        mbs.append((("last4", "p16", r), P16, 15, 0, False, lv))
        lv = np.zeros(384, np.int16); lv[((r + 5) % 16) * 16 + r] = _nzval(rng, 9)
        mbs.append((("last4", "i16", r), I16, 15, 0, False, lv))
        lv = np.zeros(384, np.int16); lv[256 + (r % 8) * 16 + r] = _nzval(rng, 9)
        mbs.append((("last4", "chroma", r), P16, 0, 2, False, lv))
    for cls, typ in (("i8", I8), ("p16t8", P16)):
        for s in range(4):
            for r in range(64):
                lv = np.zeros(384, np.int16); lv[s * 64 + r] = _nzval(rng, 9)
                mbs.append((("last8", cls, s, r), typ, 15, 0, True, lv))
    # only the separately coded DC is nonzero: every block is its count symbol alone, value 0
    lv = np.zeros(384, np.int16); lv[0:256:16] = rng.integers(1, 9, 16)
    mbs.append((("dc_only", "i16", 32), I16, 15, 0, False, lv))
    lv = np.zeros(384, np.int16); lv[256::16] = rng.integers(1, 9, 8)
    mbs.append((("dc_only", "chroma", 16), P16, 0, 2, False, lv))
    mbs.append((("i16_empty", 16), I16, 0, 0, False, None))
    lv = np.zeros(384, np.int16); lv[256::16] = rng.integers(1, 9, 8)
    mbs.append((("cbpc", 1), I4, 0, 1, False, lv.copy()))
    lv[256 + 3 * 16 + 7] = 2; lv[256 + 6 * 16 + 15] = -1
    mbs.append((("cbpc", 2), I4, 0, 2, False, lv))
    for t8 in (False, True):
        for cbpl in range(16):
            lv = mask_to_cbp(rng.integers(-2, 3, 384).astype(np.int16), P16, cbpl, 0)
            mbs.append((("cbpl", cbpl, t8), P16, cbpl, 0, t8, lv))
    # run lengths as different as a macroblock allows (a 4x4 block has 16 positions): 16 different luma runs, 8 different chroma runs
    for typ in (P16, I4, I16):
        lv = np.zeros(384, np.int16)
        st = 1 if typ == I16 else 0
        for b, last in enumerate(rng.permutation(16)):
            ending_at(rng, b, 16, st, int(last) if last >= st else -1, lv)
        for i, last in enumerate(rng.permutation(15)[:8] + 1):
            ending_at(rng, 16 + i, 16, 1, int(last), lv)
        mbs.append((("runs", typ), typ, 15, 2, False, lv))
    lv = np.zeros(384, np.int16)
    for s, last in enumerate((5, 63, 22, 40)):
        ending_at(rng, s * 4, 64, 0, last, lv)
    for i, last in enumerate(rng.permutation(15)[:8] + 1):
        ending_at(rng, 16 + i, 16, 1, int(last), lv)
    mbs.append((("runs", "t8"), I8, 15, 2, True, lv))
    full = lambda: (rng.integers(1, 4, 384) * rng.choice([-1, 1], 384)).astype(np.int16)
    mbs.append((("full", "p16"), P16, 15, 2, False, full()))
    mbs.append((("full", "i16"), I16, 15, 2, False, full()))
    mbs.append((("full", "t8"), P16, 15, 2, True, full()))
    return single_pictures("last_position", mbs)


# ---- family 2: the largest last position of a macroblock (the early exit of the walk) -----------------------------------------------------
WMAX4 = (0, 3, 4, 7, 8, 11, 12, 15)
WMAX8 = (15, 16, 31, 32, 47, 48, 63)


def family_wmax():
    rng = np.random.default_rng(202)
    mbs = []
    for typ in (P16, I4):
        for w in WMAX4:
            lv = np.zeros(384, np.int16)
            lasts = rng.integers(-1, w + 1, 24)
            lasts[int(rng.integers(0, 16))] = w
            for b in range(16):
                ending_at(rng, b, 16, 0, int(lasts[b]), lv)
            for b in range(16, 24):
                ending_at(rng, b, 16, 1, int(lasts[b]), lv)
            mbs.append((("wmax4", w, typ), typ, 15, 2, False, lv))
    for typ in (P16, I8):
        for w in WMAX8:
            lv = np.zeros(384, np.int16)
            lasts = rng.integers(-1, w + 1, 4)
            lasts[int(rng.integers(0, 4))] = w
            for s in range(4):
                ending_at(rng, s * 4, 64, 0, int(lasts[s]), lv, fill=0.3)
            for b in range(16, 24):
                ending_at(rng, b, 16, 1, int(rng.integers(-1, 16)), lv)
            mbs.append((("wmax8", w, typ), typ, 15, 2, True, lv))
    for what, l8, lc in (("mixed", 63, 1), ("mixed", 0, 15)):
        lv = np.zeros(384, np.int16)
        for s in range(4):
            ending_at(rng, s * 4, 64, 0, l8, lv, fill=0.3)
        for b in range(16, 24):
            ending_at(rng, b, 16, 1, lc, lv)
        mbs.append(((what, l8, lc), I8, 15, 2, True, lv))
    return single_pictures("wmax", mbs)


# ---- family 3: the context of the walk --------------------------------------------------------------------------------------------------
def family_walk():
    rng = np.random.default_rng(303)
    mbs = []
    for typ, t8 in ((P16, False), (I16, False), (I4, False), (P16, True), (I8, True)):
        for rep in range(3):
            lv = rng.integers(-3, 4, 384).astype(np.int16)           # the clamp edges of prev and prev2, zeros among them
            lv[rng.random(384) < 0.25 * rep] = 0
            mbs.append((("small", typ, t8, rep), typ, 15, 2, t8, lv))
        lv = rng.choice(np.array([-32768, 32767, 0, 1, -1], dtype=np.int16), 384).astype(np.int16)
        mbs.append((("extremes", typ, t8), typ, 15, 2, t8, lv))
        lv = np.zeros(384, np.int16)                                   # 0, 1, 2, ... nonzero levels per block: min (4, left_nz) at every value
        for b in range(24):
            st = 1 if (b >= 16 or typ == I16) else 0
            if t8 and b < 16:
                if b % 4 == 0:
                    set_scan(lv, b, 64, rng.choice(64, (b // 4) * 2 + 1, replace=False), rng)
            else:
                set_scan(lv, b, 16, st + rng.choice(16 - st, b % 8, replace=False), rng)
        mbs.append((("left_nz", typ, t8), typ, 15, 2, t8, lv))
    lv = np.zeros(384, np.int16)                                       # 64 coefficient symbols in one block: `emitted` runs to 63
    lv[0:64] = rng.integers(1, 4, 64); lv[64 + ZZ64[63]] = 1; lv[128 + ZZ64[62]] = -1
    mbs.append((("emitted63",), P16, 7, 0, True, lv))
    return single_pictures("walk", mbs)


# ---- family 4: the neighbours -----------------------------------------------------------------------------------------------------------
NEIGHBOUR_SEED, NEIGHBOUR_SEED_T8 = 41, 43


def family_neighbours():
    rng = np.random.default_rng(NEIGHBOUR_SEED)
    chains = []
    chains.append([sparse_picture(rng, 6, 6, 0, 2, (I4, I16, P16)), sparse_picture(rng, 6, 6, 1, 0, (I4, I16, P16))])
    for w, h in ((1, 7), (7, 1), (1, 1)):
        chains.append([sparse_picture(rng, w, h, 0, 2, (I4, I16, P16)), sparse_picture(rng, w, h, 1, 0, (I4, I16, P16))])
    # a macroblock skipped in pictures 1 and 2: its entry is inherited twice, and read as left / above by its coded neighbours
    chains.append([sparse_picture(rng, 3, 3, 0, 2, (I4, I16)), sparse_picture(rng, 3, 3, 1, 0, (I4, P16), skip=(4,)),
                   sparse_picture(rng, 3, 3, 2, 0, (I16, P16), skip=(4, 0))])
    # two pictures with one frame_num: the second does not flip, its PAST is still the picture before the first
    chains.append([sparse_picture(rng, 3, 2, 0, 2, (I4, I16)), sparse_picture(rng, 3, 2, 1, 0, (I4, P16)), sparse_picture(rng, 3, 2, 1, 0, (I4, P16), skip=(2,))])
    b = Batch("neighbours", chains)
    assert b.past[4] == [None, 0, 1] and b.past[5] == [None, 0, 0]
    return b


def family_neighbours_t8():
    rng = np.random.default_rng(NEIGHBOUR_SEED_T8)
    chains = [[sparse_picture(rng, 6, 6, 0, 2, (I8, P16), t8=True), sparse_picture(rng, 6, 6, 1, 0, (I8, P16), t8=True)]]
    for w, h in ((1, 4), (4, 1), (1, 1)):
        chains.append([sparse_picture(rng, w, h, 0, 2, (I8, I16), t8=True), sparse_picture(rng, w, h, 1, 0, (I8, P16, I4), t8=True)])
    return Batch("neighbours_t8", chains)


def family_slices():
    """20x15 macroblocks, a slice each: slice ids to 299, slice types 0 and 2 in turn - `st` comes from the macroblock's own slice and the
    neighbours are read across every slice boundary"""
    rng = np.random.default_rng(47)
    n = 300
    f = sparse_picture(rng, 20, 15, 0, 0, (I4, I16, P16), slice_types=[(s & 1) * 2 for s in range(n)], slice_of=np.arange(n))
    g = sparse_picture(rng, 20, 15, 1, 0, (I4, I16, P16), slice_types=[((s + 1) & 1) * 2 for s in range(n)], slice_of=np.arange(n), skip=(21, 150, 299))
    return Batch("slices", [[f, g]])


# ---- family 5: KEEP ---------------------------------------------------------------------------------------------------------------------
def family_keep():
    rng = np.random.default_rng(55)
    w, h = 4, 3

    def pic(fn, st, lost, skip):
        f = sparse_picture(rng, w, h, fn, st, (I4, I16, P16), skip=skip)
        for k in lost:
            put_mb(f, k, 0)
        return f
    mine = rng.integers(0, 4, (w * h, 24)).astype(np.uint8)
    a = [pic(0, 2, (5,), ()), pic(1, 0, (1, 6), (2, 5)), pic(2, 0, (5, 6, 10), (1, 9)), pic(3, 0, (0, 5), (4, 6))]
    ka = [None, mine, 0, None]                       # no KEEP and no PAST; a buffer of the caller's; an earlier job; NULL while PAST is not
    c = [pic(0, 2, (), ()), pic(1, 0, (3, 4), (0,)), pic(2, 0, (3, 7), (4,))]
    kc = [None, None, 0]
    return Batch("keep", [a, c], keep=[ka, kc])


def family_keep_null():
    """the same pictures through the _keep calls with keep_dev == NULL: exactly the plain calls (type 0 takes PAST)"""
    k = family_keep()
    return Batch("keep_null", k.chains)


# ---- family 6: layouts and sums ---------------------------------------------------------------------------------------------------------
def family_sizes():
    """pictures of 1, 3 and 20 macroblocks in one call, and of 257, 512 and 513: the carry loop of the offsets"""
    rng = np.random.default_rng(66)
    chains = [[sparse_picture(rng, w, h, 0, 2, (I4, I16, P16), counts=(0, 0, 1, 3))] for w, h in ((1, 1), (3, 1), (5, 4))]
    small = Batch("sizes_small", chains, max_mbs=20)
    chains = [[sparse_picture(rng, w, h, 0, 0, (I4, I16, P16), t8=(w == 32), counts=(0, 0, 0, 1, 4))] for w, h in ((1, 257), (32, 16), (19, 27))]
    return small, Batch("sizes_large", chains)


def family_many_jobs(n_jobs):
    """n_jobs pictures of one macroblock with different counts, in chains of 1, 2 and 7 pictures"""
    rng = np.random.default_rng(600 + n_jobs)
    chains, left, c = [], n_jobs, 0
    while left:
        ln = min((1, 2, 7)[c % 3], left)
        ch = []
        for i in range(ln):
            typ = int(rng.choice((I4, I16, P16, SKIP) if i else (I4, I16, P16)))
            f = new_frame(1, 1, i, (0,))
            if typ == SKIP:
                put_mb(f, 0, SKIP)
            else:
                cbpl, cbpc = (15 if typ == I16 else int(rng.integers(0, 16))), int(rng.integers(0, 3))
                put_mb(f, 0, typ, cbpl, cbpc, False, mask_to_cbp(sparse_mb(rng, typ, False, counts=(0, 1, 2, 5)), typ, cbpl, cbpc))
            ch.append(f)
        chains.append(ch); left -= ln; c += 1
    return Batch("jobs_%d" % n_jobs, chains)


# ---- family 7: a pool that is too small -------------------------------------------------------------------------------------------------
def family_small_pool():
    rng = np.random.default_rng(77)
    ch = [sparse_picture(rng, 3, 2, 0, 2, (I4, I16, P16), counts=(1, 2, 3)), sparse_picture(rng, 3, 2, 1, 0, (I4, I16, P16), counts=(1, 2, 3), skip=(1,))]
    return Batch("small_pool", [ch])


def small_pool_caps(batch):
    """the total, one less, inside a run of the second picture, on a run's boundary there, none"""
    e = expect(batch)
    at = e[0].total + int(e[1].off[3])
    return [e[0].total + e[1].total, e[0].total + e[1].total - 1, at + int(e[1].n[3]) // 2, at, 0]


FAMILIES = {
    "last_position": family_last_position, "wmax": family_wmax, "walk": family_walk, "neighbours": family_neighbours,
    "neighbours_t8": family_neighbours_t8, "slices": family_slices, "keep": family_keep, "keep_null": family_keep_null,
    "sizes_small": lambda: family_sizes()[0], "sizes_large": lambda: family_sizes()[1],
    "jobs_1": lambda: family_many_jobs(1), "jobs_256": lambda: family_many_jobs(256), "jobs_257": lambda: family_many_jobs(257),
    "jobs_513": lambda: family_many_jobs(513), "small_pool": family_small_pool,
}
_batch_cache = {}


def batch(name):
    if name not in _batch_cache:
        _batch_cache[name] = FAMILIES[name]()
        assert _batch_cache[name].name == name
    return _batch_cache[name]


# ---- coverage measures (on the oracle's output alone) -----------------------------------------------------------------------------------
def last_positions(f, k, syms):
    """{b: last scan position that is a symbol of the block, -1 where the block is its count symbol alone}"""
    return {b: (start + n_ac - 1 if n_ac else -1) for b, n, start, at, nz, n_ac in blocks_of(f, k, syms)}


def deciding_index(f, k, syms, b, n):
    """the index into the block's levels whose scan position is the block's last one (what the count pass must find), or None"""
    last = last_positions(f, k, syms)[b]
    if last < 0:
        return None
    r = ZZ16[last] if n == 16 else ZZ64[last]
    assert f.levels[k][b * 16 + r] != 0
    return r


def wmax_of(f, k, syms):
    lp = last_positions(f, k, syms)
    return max(lp.values()) if lp else -1


def nz_contexts(f, k, syms):
    """[(b, n, colour, past, left, above)] of every nonzero-count symbol, the three taken out of the prior"""
    out = []
    for b, n, start, at, nz, n_ac in blocks_of(f, k, syms):
        p = int(syms["prior"][at])
        out.append((b, n, (p // 27) % 3, (p // 9) % 3, (p // 3) % 3, p % 3))
    return out


def inner_coords(syms):
    """(min (4, left_nz), prev + 2 clamped, prev2 + 2 clamped) of every coefficient symbol"""
    ac = syms[(syms["kind"] == AC4) | (syms["kind"] == AC8)]
    inner = ac["prior"].astype(np.int64) % 3125
    assert np.all(inner % 25 == 12)                 # the two constant coordinates
    return inner // 625, (inner // 125) % 5, (inner // 25) % 5


# ---- the kernels' own derivations restated (the oracle derives the same from the scan order / in one pass): the CPU tests hold them to the
# oracle as they stand, and show that the cases tell them from a wrong table entry or a wrong neighbour index ----------------------------------
def count_from_raster(f, k, inv16=INV16, inv64=INV64):
    """n_syms of macroblock k as the count pass finds it: from the levels in storage order through the inverse scan tables"""
    typ, cbp, t8 = int(f.mbs["mb_type"][k]), int(f.mbs["cbp"][k]), int(f.mbs["flags"][k]) & 1
    if typ in (SKIP, IPCM, 0):
        return 0
    cbpl, cbpc, i16 = cbp & 15, cbp >> 4, typ == I16
    lv = f.levels[k]

    def run(block, inv, start):
        last = max([inv[r] for r in np.flatnonzero(block) if inv[r] >= start], default=-1)
        return 1 + (last - start + 1 if last >= start else 0)
    cnt = (16 if i16 else 0) + (8 if cbpc in (1, 2) else 0)
    for s in range(4):
        if (cbpl >> s) & 1:
            cnt += run(lv[s * 64:s * 64 + 64], inv64, 0) if t8 else sum(run(lv[b * 16:b * 16 + 16], inv16, 1 if i16 else 0) for b in range(s * 4, s * 4 + 4))
    if cbpc == 2:
        cnt += sum(run(lv[b * 16:b * 16 + 16], inv16, 1) for b in range(16, 24))
    return cnt


def nz_neighbours(f, k, b, n, img, past_img, left_of_luma=3):
    """(past, left, above) of the nonzero-count prior of block b (n 64: the 8x8 block at storage index b) from the nnz images, by the
    symbol pass's indices; left_of_luma: which block of the left macroblock's row a luma block of the left column reads (b + 3)"""
    zero = np.zeros(24, dtype=np.int64)
    cur = img[k].astype(np.int64)
    lf = img[k - 1].astype(np.int64) if k % f.mb_w else zero
    ab = img[k - f.mb_w].astype(np.int64) if k >= f.mb_w else zero
    pa = past_img[k].astype(np.int64) if past_img is not None else zero
    c8 = lambda p, i: int(p[i:i + 4].sum())
    if n == 64:
        s = b >> 2
        t = (c8(pa, b), c8(lf, (s + 1) * 4) if s % 2 == 0 else c8(cur, (s - 1) * 4), c8(ab, (s + 2) * 4) if s < 2 else c8(cur, (s - 2) * 4))
    elif b < 16:
        t = (pa[b], lf[b + left_of_luma] if b % 4 == 0 else cur[b - 1], ab[b + 12] if b < 4 else cur[b - 4])
    else:
        i = b - 16
        t = (pa[b], lf[b + 1] if i % 2 == 0 else cur[b - 1], ab[b + 2] if i & 2 == 0 else cur[b - 2])
    return tuple(min(2, int(v)) for v in t)


# ---- the device stager ------------------------------------------------------------------------------------------------------------------
class Stage:
    """the pictures of a batch in device memory and the jobs of include/lh264.h over them; count() and index() run the public calls and
    bring back everything they wrote.  Every output buffer is filled with a pattern before each call."""

    def __init__(self, batch, dev=0):
        import torch
        import losslessh264_amd as lh
        from losslessh264_amd import _lib as L
        self.torch, self.L, self.lib, self.batch = torch, L, L.lib(), batch
        L.check(self.lib.lh264_set_device(dev))
        self.dev = d = torch.device("cuda", dev)
        up = self._up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(d)
        jl = self.jl = batch.jobs()
        self.exp = expect(batch)
        self.base, self.total = bases(batch, self.exp)
        ns = [f.mb_w * f.mb_h for _, _, f in jl]
        self.mo = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        so = np.concatenate([[0], np.cumsum([len(f.slices) for _, _, f in jl])]).astype(np.int64)
        self.d_mbs = up(np.concatenate([f.mbs for _, _, f in jl]))
        self.d_lev = up(np.concatenate([np.ascontiguousarray(f.levels, dtype=np.int16).reshape(-1) for _, _, f in jl]))
        self.d_sl = up(np.concatenate([f.slices for _, _, f in jl]))
        nm = int(self.mo[-1])
        self.d_nnz = torch.empty(nm * 24, dtype=torch.uint8, device=d)
        self.d_ns = torch.empty(nm * 2, dtype=torch.uint8, device=d)
        self.d_off = torch.empty(nm * 4, dtype=torch.uint8, device=d)
        self.d_base = torch.empty(len(jl) * 8, dtype=torch.uint8, device=d)
        self.d_total = torch.empty(8, dtype=torch.uint8, device=d)
        self.pool_syms = max(1, self.total) + GUARD
        self.d_pool = torch.empty(self.pool_syms * 8, dtype=torch.uint8, device=d)
        self.d_fixed = {j: torch.empty(ns[j] * MAX_SYMS * 8, dtype=torch.uint8, device=d) for j, (c, i, _) in enumerate(jl) if (c, i) in batch.fixed}
        self.job_at = {(c, i): j for j, (c, i, _) in enumerate(jl)}
        jobs = self.jobs = np.zeros(len(jl), dtype=L.CTX_JOB_DTYPE)
        first, keep, self.d_keepbufs = [0], np.zeros(len(jl), dtype=np.uint64), []
        for j, (c, i, f) in enumerate(jl):
            jb = jobs[j]
            g = int(self.mo[j])
            jb["mbs"], jb["levels"], jb["slices"] = self.d_mbs.data_ptr() + g * 128, self.d_lev.data_ptr() + g * 768, self.d_sl.data_ptr() + int(so[j]) * 232
            jb["nnz_cur"], jb["n_syms"] = self.d_nnz.data_ptr() + g * 24, self.d_ns.data_ptr() + g * 2
            p = batch.past[c][i]
            jb["nnz_past"] = 0 if p is None else self.d_nnz.data_ptr() + int(self.mo[self.job_at[(c, p)]]) * 24
            jb["mb_w"], jb["mb_h"] = f.mb_w, f.mb_h
            if j in self.d_fixed:
                jb["syms"] = self.d_fixed[j].data_ptr()
            else:
                jb["syms"], jb["sym_off"], jb["sym_base"] = self.d_pool.data_ptr(), self.d_off.data_ptr() + g * 4, self.d_base.data_ptr() + j * 8
            if batch.keep is not None:
                kp = batch.keep[c][i]
                if isinstance(kp, np.ndarray):
                    self.d_keepbufs.append(up(kp))
                    keep[j] = self.d_keepbufs[-1].data_ptr()
                elif kp is not None:
                    keep[j] = self.d_nnz.data_ptr() + int(self.mo[self.job_at[(c, kp)]]) * 24
            if i == len(batch.chains[c]) - 1:
                first.append(j + 1)
        self.n_chains = len(batch.chains)
        self.d_first = up(np.array(first, dtype=np.int32))
        self.d_keep = up(keep) if batch.keep is not None else None

    def _fill(self):
        for t, v in ((self.d_nnz, 0xCD), (self.d_ns, 0xFF), (self.d_off, 0xFF), (self.d_base, 0xFF), (self.d_total, 0xFF), (self.d_pool, POOL_FILL)):
            t.fill_(v)
        for t in self.d_fixed.values():
            t.fill_(POOL_FILL)

    def _call(self, symbols, cap, through_keep):
        torch, L = self.torch, self.L
        self._fill()
        jobs = self.jobs.copy()
        jobs["syms_cap"] = self.total if cap is None else cap
        assert int(jobs["syms_cap"].max()) <= self.pool_syms - GUARD           # the pool is never smaller than what the call is told
        d_jobs = self._up(jobs)
        s = torch.cuda.current_stream(self.dev).cuda_stream
        kp = self.d_keep.data_ptr() if self.d_keep is not None else 0
        a = (d_jobs.data_ptr(), self.d_first.data_ptr(), self.n_chains, len(jobs), self.batch.max_mbs)
        if through_keep or self.d_keep is not None:
            a = (a[0], kp) + a[1:]
            rc = self.lib.lh264_ctx_index_chains_keep(*a, s) if symbols else self.lib.lh264_ctx_count_chains_keep(*a, self.d_total.data_ptr(), s)
        else:
            rc = self.lib.lh264_ctx_index_chains(*a, s) if symbols else self.lib.lh264_ctx_count_chains(*a, self.d_total.data_ptr(), s)
        L.check(rc)
        torch.cuda.synchronize(self.dev)
        r = Frame()
        host = lambda t, dt: t.cpu().numpy().view(dt)
        r.nnz, r.n_syms, r.sym_off = host(self.d_nnz, np.uint8).reshape(-1, 24), host(self.d_ns, np.uint16), host(self.d_off, np.uint32)
        r.sym_base, r.total = host(self.d_base, np.uint64), int(host(self.d_total, np.uint64)[0])
        r.pool = host(self.d_pool, np.uint64)
        r.fixed = {j: host(t, np.uint64).reshape(-1, MAX_SYMS) for j, t in self.d_fixed.items()}
        r.symbols, r.cap = symbols, self.total if cap is None else cap
        return r

    def count(self, through_keep=False):
        return self._call(False, None, through_keep)

    def index(self, cap=None, through_keep=False):
        return self._call(True, cap, through_keep)


UNWRITTEN = np.frombuffer(bytes([POOL_FILL] * 8), dtype=np.uint64)[0]


def _first_diff(got, want):
    at = int(np.flatnonzero(got != want)[0])
    return "first at symbol %d: got %s want %s" % (at, got[at:at + 1].view(SYM), want[at:at + 1].view(SYM))


def compare(stage, r):
    """everything a call wrote against the expectation; r.symbols False: the count call (nothing in the pool), else the index call with
    r.cap symbols of room: a macroblock whose run ends at or before the cap is whole, every other reads n_syms 0 and has written nothing"""
    b, exps = stage.batch, stage.exp
    pool = np.full(stage.pool_syms, UNWRITTEN, dtype=np.uint64)
    for j, ((c, i, f), e) in enumerate(zip(stage.jl, exps)):
        where = "%s: chain %d picture %d (job %d, %dx%d)" % (b.name, c, i, j, f.mb_w, f.mb_h)
        g, n = int(stage.mo[j]), f.mb_w * f.mb_h
        got = r.nnz[g:g + n]
        assert np.array_equal(got, e.img), "%s: nnz image, macroblocks %s" % (where, np.flatnonzero((got != e.img).any(axis=1))[:8])
        ns = r.n_syms[g:g + n].astype(np.int64)
        if j in r.fixed:
            want_n, img = e.n, np.full((n, MAX_SYMS), UNWRITTEN, dtype=np.uint64)        # (the count call leaves its counts and no symbol)
            for k in range(n if r.symbols else 0):
                img[k, :e.n[k]] = e.syms[k].view(np.uint64)
            assert np.array_equal(ns, want_n), "%s: n_syms (fixed), macroblocks %s" % (where, np.flatnonzero(ns != want_n)[:8])
            bad = np.flatnonzero((r.fixed[j] != img).any(axis=1))
            assert len(bad) == 0, "%s: fixed slots of macroblocks %s; %s" % (where, bad[:8], _first_diff(r.fixed[j][bad[0]], img[bad[0]]))
            continue
        off = r.sym_off[g:g + n].astype(np.int64)
        assert np.array_equal(off, e.off), "%s: sym_off, macroblocks %s" % (where, np.flatnonzero(off != e.off)[:8])
        assert int(r.sym_base[j]) == int(stage.base[j]), "%s: sym_base %d, want %d" % (where, int(r.sym_base[j]), int(stage.base[j]))
        whole = (stage.base[j] + e.off + e.n <= r.cap) if r.symbols else np.ones(n, dtype=bool)
        want_n = np.where(whole, e.n, 0)
        assert np.array_equal(ns, want_n), "%s: n_syms, macroblocks %s got %s want %s" % (where, np.flatnonzero(ns != want_n)[:8], ns[ns != want_n][:8], want_n[ns != want_n][:8])
        if r.symbols:
            for k in np.flatnonzero(whole & (e.n > 0)):
                at = int(stage.base[j] + e.off[k])
                pool[at:at + e.n[k]] = e.syms[k].view(np.uint64)
    if not r.symbols:
        assert r.total == stage.total, "%s: total %d, want %d" % (b.name, r.total, stage.total)
    if not np.array_equal(r.pool, pool):
        at = int(np.flatnonzero(r.pool != pool)[0])
        j = int(np.searchsorted(stage.base, at, side="right")) - 1
        while j in r.fixed or exps[j].total == 0:
            j -= 1
        k = int(np.searchsorted(exps[j].off, at - stage.base[j], side="right")) - 1
        c, i, f = stage.jl[j]
        raise AssertionError("%s: pool differs at symbol %d of %d (cap %d): chain %d picture %d macroblock %d type %#x cbp %#x flags %d, symbol %d of its %d; got %s want %s"
                             % (b.name, at, stage.total, r.cap, c, i, k, f.mbs["mb_type"][k], f.mbs["cbp"][k], f.mbs["flags"][k],
                                at - stage.base[j] - exps[j].off[k], exps[j].n[k], r.pool[at:at + 1].view(SYM), pool[at:at + 1].view(SYM)))
