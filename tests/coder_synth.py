"""Synthetic streams for the device coder (lh264_code_chains) and the two ways of coding them: the device and the oracle
(oracle/oracle_coder.c orc_coder_symbols).  Test infrastructure only.

A stream is a list of pictures; a picture is, per macroblock, a host symbol list (the front end's row-a10 symbols, at most one
SPLICE marker) and a list of coefficient symbols (what the context-index kernels write), in the product's 8-byte lh264_ctx_sym_t.

The domain - what the product can legitimately be given (csrc/host/pip_symbols.cpp, csrc/lh264_ctx.hip); outside it device and
oracle differ by design:
  TREE    only on MBTYPE, SKIPRUN, SUBMB, NUMREF, CBPC, CBPL, PREDMODE (the tables the host uses it for: 4 / 9 / 8 / 4 / 2 / 4 / 4 bits);
          a table is used by one kind only (the device files a tree's nodes under index * groups + node / 16, lh264_coder.hip tree_at)
  POW2    only on MODE8 (3 bits, preferred value = the index) and QPL (7 bits, preferred 0); values 0 .. 2^bits
  BIT     on STOP and T8
  RAW     widths 0 .. 16 (`prior` is the width); width 0 only on a tag the stream uses anyway (the host's ref_idx bits follow the
          NUMREF tree of their tag): the reference brings a tag's stream into existence by naming it, the product by a decision
  MVD     prior LH264_PRIOR(MVD, type * 16 + block), any int16 value
  host tags (`pad`) in 0 .. 33 or 69
  kinds 0-5: prior indices by the context-index formulas (ctx_prior below); `pad` 0 or the tag the prior implies (lh264_coder.hip
          ac_tag_base, nz_tag); DC and coefficient values over the whole int16 range, nonzero counts 0 .. 16 / 64
  at most LH264_MAX_SYN_SYMS host and LH264_CTX_MAX_SYMS coefficient symbols per macroblock
"""
import ctypes as C
import os

import numpy as np

SYM = np.dtype([("prior", "<u4"), ("value", "<i2"), ("kind", "u1"), ("pad", "u1")])     # lh264_ctx_sym_t
LDC, CDC, NZ4, AC4, NZ8, AC8, TREE, POW2, BIT, RAW, MVD, SPLICE = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 15
(TB_MBTYPE, TB_MVD, TB_MODE8, TB_LDC, TB_CDC, TB_NZ4, TB_NZ8, TB_AC4, TB_AC8, TB_SKIPRUN, TB_QPL, TB_SUBMB, TB_NUMREF, TB_CBPC, TB_CBPL,
 TB_STOP, TB_T8, TB_PREDMODE) = range(18)
MAX_SYN, MAX_CTX, N_SLOTS = 96, 432, 40
TAG_OF_SLOT = list(range(34)) + [69]
# (table, bits, index bound, tag) of every TREE / POW2 / BIT use of the host (pip_symbols.cpp)
TREES = [(TB_MBTYPE, 4, 62, 7), (TB_SKIPRUN, 9, 512 * 16, 1), (TB_SUBMB, 8, 16, 14), (TB_NUMREF, 4, 17 * 16, 9), (TB_CBPC, 2, 64, 4),
         (TB_CBPL, 4, 256, 4), (TB_PREDMODE, 4, 16 * 8 * 9, 13)]
POW2S = [(TB_MODE8, 3, 8, 10), (TB_MODE8, 3, 8, 11), (TB_QPL, 7, 6, 6)]
BITS = [(TB_STOP, 2048, 2), (TB_T8, 2048, 8)]
MVD_TYPES = (0x08, 0x10, 0x20, 0x40, 0x80)


def prior(table, index):
    return (table << 27) | index


def hsym(kind, table, index, value, tag):
    """one host symbol"""
    return (prior(table, index), value, kind, tag)


def raw(nbits, value, tag):
    return (nbits, value, RAW, tag)


def splice():
    return (0, 0, SPLICE, 0)


def ctx_prior(kind, st=0, mbc=2, color=0, emitted=0, inner=0, i=0, ctx=0):
    """the index formulas of lh264_ctx.hip: DC (i * 5 + st) * 16 + mbc; nonzero counts (((st * 16 + mbc) * 3 + color) * 27 + ctx);
    coefficients (((st * 16 + mbc) * 3 + color) * nco + emitted) * 3125 + inner"""
    if kind in (LDC, CDC):
        return (i * 5 + st) * 16 + mbc
    if kind in (NZ4, NZ8):
        return ((st * 16 + mbc) * 3 + color) * 27 + ctx
    nco = 16 if kind == AC4 else 64
    return (((st * 16 + mbc) * 3 + color) * nco + emitted) * 3125 + inner


def implied_tag(kind, pr):
    """the tag the context-index kernel writes into `pad` (lh264_coder.hip ac_tag_base / nz_tag)"""
    if kind == LDC:
        return 17
    if kind == CDC:
        return 18
    if kind in (NZ4, NZ8):
        return 29 if (pr // 27) % 3 else 19
    nco = 16 if kind == AC4 else 64
    outer = pr // 3125
    emitted, color, code = outer % nco, (outer // nco) % 3, (outer // nco // 3) % 16
    return 29 if color else (19 if (emitted == 0 and code != 1) else 24)


def csym(kind, pr, value, pad=None):
    """one coefficient symbol; pad None: the implied tag (as the context-index kernel writes it), 0: none"""
    return (pr, value, kind, implied_tag(kind, pr) if pad is None else pad)


class Picture:
    """host: SYM[], host_off: n_mbs + 1 offsets; ctx: SYM[] of all macroblocks, ctx_n: per macroblock (macroblock k's behind k-1's)"""

    def __init__(self, host, host_off, ctx, ctx_n):
        self.host = np.ascontiguousarray(host, dtype=SYM)
        self.host_off = np.ascontiguousarray(host_off, dtype=np.uint32)
        self.ctx = np.ascontiguousarray(ctx, dtype=SYM)
        self.ctx_n = np.ascontiguousarray(ctx_n, dtype=np.uint16)
        self.n_mbs = len(self.ctx_n)
        assert len(self.host_off) == self.n_mbs + 1 and int(self.ctx_n.sum(dtype=np.int64)) == len(self.ctx)
        assert int(self.host_off[-1]) == len(self.host)
        nh = np.diff(self.host_off.astype(np.int64))
        assert (nh <= MAX_SYN).all() and (self.ctx_n <= MAX_CTX).all(), "beyond the per-macroblock maxima"
        self.ctx_off = np.concatenate([[0], np.cumsum(self.ctx_n, dtype=np.int64)])

    @staticmethod
    def from_lists(mbs):
        """mbs: list of (host list, ctx list) of tuples (hsym / raw / splice / csym)"""
        host = [h for m in mbs for h in m[0]]
        ctx = [c for m in mbs for c in m[1]]
        off = np.concatenate([[0], np.cumsum([len(m[0]) for m in mbs])]) if mbs else np.zeros(1)
        return Picture(np.array(host, dtype=SYM) if host else np.zeros(0, SYM), off, np.array(ctx, dtype=SYM) if ctx else np.zeros(0, SYM),
                       [len(m[1]) for m in mbs])


def empty_picture(n_mbs):
    return Picture(np.zeros(0, SYM), np.zeros(n_mbs + 1, np.uint32), np.zeros(0, SYM), np.zeros(n_mbs, np.uint16))


def stacked_picture(host_rows, ctx_rows=None, splice_at=0):
    """a picture of len(host_rows) macroblocks from per-macroblock SYM arrays (vectorised builder for large pictures: every macroblock
    gets the same counts); ctx_rows: [n, c] coefficient symbols spliced in at host position `splice_at`"""
    host_rows = np.asarray(host_rows, dtype=SYM)
    n, h = host_rows.shape
    if ctx_rows is not None:
        sp = np.zeros((n, 1), SYM)
        sp["kind"] = SPLICE
        host_rows = np.concatenate([host_rows[:, :splice_at], sp, host_rows[:, splice_at:]], axis=1)
        h += 1
        ctx = np.asarray(ctx_rows, dtype=SYM)
        cn = np.full(n, ctx.shape[1], np.uint16)
        ctx = ctx.reshape(-1)
    else:
        ctx, cn = np.zeros(0, SYM), np.zeros(n, np.uint16)
    return Picture(host_rows.reshape(-1), np.arange(n + 1, dtype=np.uint32) * h, ctx, cn)


# ---- random symbols inside the domain -------------------------------------------------------------------------------------------
def random_host(rng, n, amp=32767):
    """n host symbols (no SPLICE) drawn over every kind and table of the domain"""
    out = np.zeros(n, SYM)
    cat = rng.integers(0, 14, n)
    for c in range(14):
        m = cat == c
        k = int(m.sum())
        if not k:
            continue
        if c < 7:
            tb, bits, ib, tag = TREES[c]
            out["prior"][m] = prior(tb, 0) + rng.integers(0, ib, k)
            out["value"][m] = rng.integers(0, 1 << bits, k)
            out["kind"][m], out["pad"][m] = TREE, tag
        elif c < 10:
            tb, bits, ib, tag = POW2S[c - 7]
            idx = rng.integers(0, ib, k)
            pref = idx if tb == TB_MODE8 else np.zeros(k, np.int64)
            val = rng.integers(0, (1 << bits) + 1, k)
            val = np.where(rng.random(k) < 0.4, pref, val)        # at the preferred value and off it
            out["prior"][m] = prior(tb, 0) + idx
            out["value"][m] = val
            out["kind"][m], out["pad"][m] = POW2, tag
        elif c < 12:
            tb, ib, tag = BITS[c - 10]
            out["prior"][m] = prior(tb, 0) + rng.integers(0, ib, k)
            out["value"][m] = rng.integers(0, 2, k)
            out["kind"][m], out["pad"][m] = BIT, tag
        elif c == 12:
            w = rng.integers(1, 17, k)                             # (width 0: scenarios a, b)
            out["prior"][m] = w
            out["value"][m] = (rng.integers(0, 1 << 16, k) & ((1 << w) - 1)).astype(np.uint16).view(np.int16)
            out["kind"][m], out["pad"][m] = RAW, rng.choice([9, 69, 5, 33, 0], k)
        else:
            ty = rng.choice(MVD_TYPES, k)
            out["prior"][m] = prior(TB_MVD, 0) + ty * 16 + rng.integers(0, 16, k)
            out["value"][m] = random_values(rng, k, amp)
            out["kind"][m], out["pad"][m] = MVD, rng.choice([15, 16], k)
    return out


def random_values(rng, n, amp):
    """signed values: mostly small, a share up to +-amp (int16)"""
    small = rng.geometric(0.35, n) - 1
    big = rng.integers(0, amp + 1, n)
    v = np.where(rng.random(n) < 0.1, big, small) * np.where(rng.random(n) < 0.5, -1, 1)
    return np.clip(v, -32768, 32767).astype(np.int16)


def random_ctx(rng, n, amp=32767, pad_zero=0.3, st_max=5):
    """n coefficient symbols over kinds 0-5, prior indices by the context-index formulas"""
    kind = rng.choice([LDC, CDC, NZ4, AC4, NZ8, AC8], n, p=[0.08, 0.06, 0.1, 0.46, 0.05, 0.25])
    st, mbc, color = rng.integers(0, st_max, n), rng.integers(0, 16, n), rng.integers(0, 3, n)
    pr = np.zeros(n, np.int64)
    val = random_values(rng, n, amp).astype(np.int64)
    dc = (kind == LDC) | (kind == CDC)
    pr[dc] = (rng.integers(0, 16, n)[dc] % np.where(kind[dc] == LDC, 16, 8) * 5 + st[dc]) * 16 + mbc[dc]
    nz = (kind == NZ4) | (kind == NZ8)
    pr[nz] = ((st[nz] * 16 + mbc[nz]) * 3 + color[nz]) * 27 + rng.integers(0, 27, n)[nz]
    val[nz] = rng.integers(0, 17, n)[nz] * np.where(kind[nz] == NZ8, 4, 1)
    ac = (kind == AC4) | (kind == AC8)
    nco = np.where(kind == AC4, 16, 64)
    inner = (((rng.integers(0, 5, n) * 5 + rng.integers(0, 5, n)) * 5 + rng.integers(0, 5, n)) * 5 + 2) * 5 + 2
    pr[ac] = ((((st * 16 + mbc) * 3 + color) * nco + rng.integers(0, 64, n) % nco) * 3125 + inner)[ac]
    out = np.zeros(n, SYM)
    out["prior"], out["value"], out["kind"] = pr, val, kind
    tags = np.array([implied_tag(int(k), int(p)) for k, p in zip(kind, pr)], dtype=np.uint8) if n else np.zeros(0, np.uint8)
    out["pad"] = np.where(rng.random(n) < pad_zero, 0, tags)
    return out


def random_picture(rng, n_mbs, host_max=40, ctx_max=120, amp=32767, splice_p=0.8, empty_p=0.1):
    """n_mbs macroblocks with random host lists (a SPLICE at a random place, first and last included) and coefficient symbols"""
    nh = rng.integers(0, host_max + 1, n_mbs)
    nc = rng.integers(0, ctx_max + 1, n_mbs)
    empty = rng.random(n_mbs) < empty_p
    nh[empty], nc[empty] = 0, 0
    has = (rng.random(n_mbs) < splice_p) & ~empty
    host = random_host(rng, int(nh.sum()), amp)
    rows, pos = [], 0
    for k in range(n_mbs):
        h = host[pos:pos + nh[k]]
        pos += nh[k]
        if has[k]:
            p = int(rng.integers(0, nh[k] + 1))
            sp = np.zeros(1, SYM)
            sp["kind"] = SPLICE
            h = np.concatenate([h[:p], sp, h[p:]])
        rows.append(h)
    nc[~has] = np.where(rng.random(int((~has).sum())) < 0.5, 0, nc[~has])    # coefficient symbols without a marker are never coded
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return Picture(np.concatenate(rows) if rows else np.zeros(0, SYM), off, random_ctx(rng, int(nc.sum()), amp), nc)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def flatten(stream):
    """the symbols of a stream in coding order: per macroblock its host list, the coefficient symbols at the marker (none without one)"""
    parts = []
    for pic in stream:
        n = pic.n_mbs
        if n == 0:
            continue
        h0 = pic.host_off[:-1].astype(np.int64)
        nh = np.diff(pic.host_off.astype(np.int64))
        sp = np.full(n, -1, np.int64)
        idx = np.nonzero(pic.host["kind"] == SPLICE)[0]
        if len(idx):
            mb = np.searchsorted(pic.host_off, idx, side="right") - 1
            sp[mb] = idx - h0[mb]
        mc = np.where(sp >= 0, pic.ctx_n.astype(np.int64), 0)
        ln = np.where(sp >= 0, nh - 1 + mc, nh)
        tot = int(ln.sum())
        if tot == 0:
            continue
        mbi = np.repeat(np.arange(n), ln)
        i = np.arange(tot) - np.repeat(np.cumsum(ln) - ln, ln)
        p, m = sp[mbi], mc[mbi]
        both = np.concatenate([pic.host, pic.ctx])
        hsrc = h0[mbi] + np.where((p >= 0) & (i >= p + m), i - m + 1, i)
        csrc = len(pic.host) + pic.ctx_off[mbi] + i - p
        src = np.where((p >= 0) & (i >= p) & (i < p + m), csrc, hsrc)
        parts.append(both[src])
    return np.concatenate(parts) if parts else np.zeros(0, SYM)


class OracleResult:
    def __init__(self, tags, trace=None):
        self.tags, self.trace = tags, trace       # {tag: bytes}; trace: (tag, probability, bit) uint8 arrays


def oracle(stream, trace=False):
    """orc_coder_symbols + orc_coder_finish over the flattened stream"""
    import oracle_lib as O
    L = O.lib()
    L.orc_coder_new.restype = C.c_void_p
    L.orc_coder_error.restype = C.c_char_p
    c = C.c_void_p(L.orc_coder_new(1 if trace else 0))
    try:
        syms = np.ascontiguousarray(flatten(stream))
        assert L.orc_coder_symbols(c, syms.ctypes.data_as(C.c_void_p), C.c_long(len(syms))) == 0, L.orc_coder_error(c)
        tr = None
        if trace:
            t, p, b = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint8)()
            n = L.orc_coder_trace(c, C.byref(t), C.byref(p), C.byref(b))
            tr = tuple(np.ctypeslib.as_array(x, (n,)).copy() if n else np.zeros(0, np.uint8) for x in (t, p, b))
        L.orc_coder_finish(c)
        tags = {}
        for tag in TAG_OF_SLOT:
            ptr = C.POINTER(C.c_uint8)()
            ln = L.orc_coder_tag(c, tag, C.byref(ptr))
            if ln:
                tags[tag] = bytes(np.ctypeslib.as_array(ptr, (ln,)))
        return OracleResult(tags, tr)
    finally:
        L.orc_coder_free(c)


def bool_code(bits, probs):
    """the libvpx bool coder of one tag over (bit, probability) in Python, stop decisions included (oracle_coder.c w_write / w_stop);
    -> (bytes, longest run of 0xff bytes a carry went through)"""
    norm = [0] * 256
    for r in range(1, 256):
        norm[r] = 7 - (r.bit_length() - 1)
    low, rng, count, buf, longest = 0, 255, -24, bytearray(), 0
    for bit, p in list(zip(bits, probs)) + [(0, 128)] * 32:
        split = 1 + (((rng - 1) * int(p)) >> 8)
        r = split
        if bit:
            low += split
            r = rng - split
        shift = norm[r]
        r <<= shift
        count += shift
        if count >= 0:
            off = shift - count
            if (low << (off - 1)) & 0x80000000:
                x, run = len(buf) - 1, 0
                while x >= 0 and buf[x] == 0xff:
                    buf[x] = 0
                    x -= 1
                    run += 1
                buf[x] += 1
                longest = max(longest, run)
            buf.append((low >> (24 - off)) & 0xff)
            low = (low << off) & 0xffffffff
            shift = count
            low &= 0xffffff
            count -= 8
        low = (low << shift) & 0xffffffff
        rng = r
    if (buf[-1] & 0xe0) == 0xc0:
        buf.append(0)
    return bytes(buf), longest


# ---- the device --------------------------------------------------------------------------------------------------------------------
class DeviceResult:
    def __init__(self, lens, status, tags, slots):
        self.lens, self.status, self.tags = lens, status, tags     # lens: 35 slot lengths; tags: {tag: bytes}, each clipped to out_cap
        self.slots = slots                                          # the stream's output buffer as written: [LH264_N_TAG_SLOTS, out_cap]


SENTINEL = 0xa5
GUARD = 64          # bytes behind the last stream's output buffer (DeviceResult.slots / device.tail)


def device(streams, hash_cap=1 << 16, out_cap=1 << 16, layout="compact", split=False, dev=0):
    """codes `streams` in ONE call of lh264_code_chains (split: lh264_code_binarise_chains + lh264_code_finish_chains); hash_cap: one
    value or one per stream.  -> list of DeviceResult (bytes read whatever the status, lengths clipped to out_cap)"""
    import torch
    from losslessh264_amd import _lib as L
    lib = L.lib()
    L.check(lib.lh264_set_device(dev))
    d = torch.device("cuda", dev)
    caps = list(hash_cap) if isinstance(hash_cap, (list, tuple)) else [hash_cap] * len(streams)
    pics = [p for s in streams for p in s]
    n_jobs, n_chains = len(pics), len(streams)
    host = np.concatenate([p.host for p in pics] + [np.zeros(1, SYM)])
    hoff = np.concatenate([p.host_off for p in pics] + [np.zeros(1, np.uint32)])
    cn = np.concatenate([p.ctx_n for p in pics] + [np.zeros(1, np.uint16)])
    if layout == "fixed":        # 432 slots per macroblock
        ctx = np.zeros(sum(p.n_mbs for p in pics) * MAX_CTX + 1, SYM)
        o = 0
        for p in pics:
            slot = (o + np.repeat(np.arange(p.n_mbs), p.ctx_n) * MAX_CTX + np.arange(len(p.ctx)) - np.repeat(p.ctx_off[:-1], p.ctx_n))
            ctx[slot] = p.ctx
            o += p.n_mbs * MAX_CTX
        symoff = np.zeros(1, np.uint32)
    else:                        # one pool; a macroblock's run padded to 8 symbols, the pictures behind one another
        runs = [((p.ctx_n.astype(np.int64) + 7) // 8) * 8 for p in pics]
        offs = [np.concatenate([[0], np.cumsum(r)[:-1]]) if len(r) else np.zeros(0, np.int64) for r in runs]
        bases = np.concatenate([[0], np.cumsum([int(r.sum()) for r in runs])]).astype(np.uint64) + 8      # (a pool that does not start at 0)
        ctx = np.zeros(int(bases[-1]) + 1, SYM)
        for p, o, b in zip(pics, offs, bases):
            dst = int(b) + np.repeat(o, p.ctx_n) + np.arange(len(p.ctx)) - np.repeat(p.ctx_off[:-1], p.ctx_n)
            ctx[dst] = p.ctx
        symoff = np.concatenate(offs + [np.zeros(1, np.int64)]).astype(np.uint32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(d)
    d_host, d_hoff, d_ctx, d_cn, d_symoff = t(host), t(hoff), t(ctx), t(cn), t(symoff)
    jobs = np.zeros(n_jobs, L.CODE_JOB_DTYPE)
    hs = ho = mo = co = 0
    for j, p in enumerate(pics):
        jobs[j]["syn_syms"], jobs[j]["syn_off"] = d_host.data_ptr() + hs * 8, d_hoff.data_ptr() + ho * 4
        jobs[j]["ctx_n_syms"], jobs[j]["n_mbs"] = d_cn.data_ptr() + mo * 2, p.n_mbs
        if layout == "fixed":
            jobs[j]["ctx_syms"] = d_ctx.data_ptr() + mo * MAX_CTX * 8
        else:
            jobs[j]["ctx_syms"], jobs[j]["ctx_sym_off"] = d_ctx.data_ptr(), d_symoff.data_ptr() + co * 4
        hs += len(p.host); ho += p.n_mbs + 1; mo += p.n_mbs; co += p.n_mbs
    d_bases = t(bases[:-1] if layout != "fixed" else np.zeros(1, np.uint64))
    if layout != "fixed":
        for j in range(n_jobs):
            jobs[j]["ctx_sym_base"] = d_bases.data_ptr() + j * 8
    first = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int32)
    cells = [torch.zeros(max(c, 1) * 16, dtype=torch.int32, device=d) for c in caps]
    d_out = torch.full((n_chains * N_SLOTS * out_cap + GUARD,), SENTINEL, dtype=torch.uint8, device=d)   # what is not written stays SENTINEL
    d_keys = torch.zeros(16, dtype=torch.int32, device=d)                        # (lh264_code_stream_t.hash_keys_dev: not used)
    d_len = torch.zeros(n_chains * (N_SLOTS + 1), dtype=torch.int32, device=d)
    sd = np.zeros(n_chains, L.CODE_STREAM_DTYPE)
    for c in range(n_chains):
        sd[c]["hash_keys"], sd[c]["hash_cells"] = d_keys.data_ptr(), cells[c].data_ptr()
        sd[c]["out"], sd[c]["out_len"] = d_out.data_ptr() + c * N_SLOTS * out_cap, d_len.data_ptr() + c * (N_SLOTS + 1) * 4
        sd[c]["hash_cap"], sd[c]["out_cap"] = caps[c], out_cap
    d_jobs, d_first, d_st = t(jobs if n_jobs else np.zeros(1, L.CODE_JOB_DTYPE)), t(first), t(sd)
    total = sum(p.n_mbs for p in pics)
    maxm = max([p.n_mbs for p in pics] + [1])
    s = torch.cuda.current_stream(d).cuda_stream
    torch.cuda.synchronize(d)
    if split:
        L.check(lib.lh264_code_binarise_chains(d_jobs.data_ptr(), d_first.data_ptr(), d_st.data_ptr(), n_chains, n_jobs, total, maxm, s))
        L.check(lib.lh264_code_finish_chains(d_st.data_ptr(), n_chains, s))
    else:
        L.check(lib.lh264_code_chains(d_jobs.data_ptr(), d_first.data_ptr(), d_st.data_ptr(), n_chains, n_jobs, total, maxm, s))
    torch.cuda.synchronize(d)
    lens = d_len.cpu().numpy().reshape(n_chains, N_SLOTS + 1)
    out = d_out.cpu().numpy()
    res = []
    for c in range(n_chains):
        tags = {}
        for slot, tag in enumerate(TAG_OF_SLOT):
            ln = int(lens[c, slot])
            if ln:
                b = c * N_SLOTS * out_cap + slot * out_cap
                tags[tag] = out[b:b + min(ln, out_cap)].tobytes()
        res.append(DeviceResult(lens[c, :35].copy(), int(lens[c, N_SLOTS]), tags, out[c * N_SLOTS * out_cap:(c + 1) * N_SLOTS * out_cap].reshape(N_SLOTS, out_cap)))
    assert (lens[:, 35:N_SLOTS] == 0).all(), "tag slots beyond 34 were written"
    device.tail = out[n_chains * N_SLOTS * out_cap:]
    return res


def last_totals():
    from losslessh264_amd import _lib as L
    a, b = C.c_ulonglong(), C.c_ulonglong()
    L.check(L.lib().lh264_code_last_totals(C.byref(a), C.byref(b)))
    return a.value, b.value


def range_paths():
    """lh264_debug_coder_range_paths of the last call: coarse chunks [first, walked on, one candidate, several, mapped]"""
    from losslessh264_amd import _lib as L
    f = L.lib().lh264_debug_coder_range_paths
    f.restype, f.argtypes = C.c_int, [C.POINTER(C.c_ulonglong)]
    out = (C.c_ulonglong * 5)()
    assert f(out) >= 0
    return [int(x) for x in out]


def coder_parts(chain=0):
    """lh264_debug_coder_parts: P after a call in the wave form, -1 after one in the sw form, -2 when there is nothing to read"""
    from losslessh264_amd import _lib as L
    f = L.lib().lh264_debug_coder_parts
    f.restype, f.argtypes = C.c_int, [C.c_int, C.POINTER(C.c_ulonglong), C.c_int]
    out = (C.c_ulonglong * 128)()
    return f(chain, out, 128)


# ---- the scenarios (tests/test_coder_synth.py checks their properties on the oracle, tests/test_coder_synth_gpu.py codes them) -------
def _pics_of(rows, per_mb=MAX_SYN):
    """host symbols (list of tuples) cut into macroblocks of at most per_mb"""
    mbs = [(rows[i:i + per_mb], []) for i in range(0, len(rows), per_mb)]
    return Picture.from_lists(mbs)


def edge_values():
    v = {0, 1, -1, 32767, -32767, -32768, 14, 15, 16, -14, -15, -16, 9, 10, 11, -9, -10, -11}
    for k in range(1, 16):
        for d in (-1, 0, 1):
            v.update({(1 << k) + d, -((1 << k) + d)})
    return sorted(x for x in v if -32768 <= x <= 32767)


def scenario_a():
    """every kind and table: edge values through every integer binariser, TREE on every value, POW2 at the preferred value and off
    it, RAW widths 0 .. 16"""
    vals = edge_values()
    host = []
    for tb, bits, ib, tag in TREES:
        host += [hsym(TREE, tb, (v * 7) % ib, v, tag) for v in range(1 << bits)]
    for tb, bits, ib, tag in POW2S:
        host += [hsym(POW2, tb, i, v, tag) for i in range(ib) for v in range((1 << bits) + 1)]
    for tb, ib, tag in BITS:
        host += [hsym(BIT, tb, i % ib, i & 1, tag) for i in range(8)]
    host += [raw(w, (0x5a5a & ((1 << w) - 1)) if w < 16 else -1, tag) for w in range(17) for tag in (9, 69)]
    host += [hsym(MVD, TB_MVD, ty * 16 + (i % 16), v, 15 + (i & 1)) for i, v in enumerate(vals) for ty in MVD_TYPES[:2]]
    ctx = []
    for kind in (LDC, CDC, AC4, AC8):
        for i, v in enumerate(vals):
            pr = ctx_prior(kind, st=i % 5, mbc=i % 16, color=i % 3, emitted=i % 3, inner=62, i=i % 8)
            ctx.append(csym(kind, pr, v, None if i & 1 else 0))
    for kind, top in ((NZ4, 16), (NZ8, 64)):
        ctx += [csym(kind, ctx_prior(kind, st=v % 5, color=v % 3, ctx=v % 27), v, None if v & 1 else 0) for v in range(top + 1)]
    pic = _pics_of(host)
    cpic = stacked_picture(np.zeros((len(ctx) // MAX_CTX + 1, 0), SYM), np.zeros((len(ctx) // MAX_CTX + 1, MAX_CTX), SYM))
    cpic.ctx[:len(ctx)] = np.array(ctx, dtype=SYM)
    cn = np.full(cpic.n_mbs, MAX_CTX, np.uint16)
    cn[-1] = len(ctx) - MAX_CTX * (cpic.n_mbs - 1)
    cpic = Picture(cpic.host, cpic.host_off, cpic.ctx[:len(ctx)], cn)
    return [[pic, cpic]]


def scenario_b():
    """degenerate streams: one AC symbol of value 0 (its EXP tag exists without a decision), an empty stream, a stream with no
    pictures, a picture of no macroblocks, macroblocks without symbols"""
    one = Picture.from_lists([([splice()], [csym(AC4, ctx_prior(AC4, mbc=2), 0)])])
    empty = Picture.from_lists([([], [])] * 5)
    mixed = Picture.from_lists([([], []), ([hsym(BIT, TB_STOP, 3, 1, 2)], []), ([], [csym(AC4, ctx_prior(AC4), 5)]),
                                ([splice()], []), ([splice(), raw(0, 0, 17)], [csym(LDC, ctx_prior(LDC), -3)]), ([], [])])
    return [[one], [empty], [], [empty_picture(0), mixed, empty_picture(0)], [mixed]]


def scenario_c(rng):
    """pictures around the segment sizes (64 wave form, 128 sw form), macroblocks at the symbol maxima, SPLICE first and last"""
    streams = [[random_picture(rng, n, host_max=30, ctx_max=60)] for n in (1, 63, 64, 65, 127, 128, 129)]
    full = []
    for k in range(3):
        h = random_host(rng, MAX_SYN - 1)
        sp = [tuple(x) for x in h]
        rows = (sp + [splice()]) if k == 0 else ([splice()] + sp) if k == 1 else (sp[:40] + [splice()] + sp[40:])
        full.append((rows, [tuple(x) for x in random_ctx(rng, MAX_CTX)]))
    streams.append([Picture.from_lists(full), random_picture(rng, 130, host_max=MAX_SYN - 1, ctx_max=MAX_CTX)])
    return streams


def scenario_d():
    """DynProbs driven to probability 0 (700 ones first, then zeros) and 255 (600 zeros first, then ones - a counter that has been
    non-zero never returns to 0: halving rounds up), alternating, runs across the halving (sum > 512); on a BIT prior, on a coefficient
    prior's zero flag, and the ones-first sequence on the shared TEST_PROB (raw bits)"""
    seq_a = [1] * 700 + [0] * 300 + [0, 1] * 150 + [1] * 257 + [0] * 256 + [1] * 513 + [0] * 602 + [1] * 3
    seq_b = [0] * 600 + [1] * 3 + [0, 1] * 100 + [0] * 520 + [1] * 2
    host = [hsym(BIT, TB_STOP, 77, b, 2) for b in seq_a] + [hsym(BIT, TB_STOP, 78, b, 2) for b in seq_b]
    host += [raw(1, b, 69) for b in seq_a]
    ctx = [csym(AC4, ctx_prior(AC4, color=1, inner=7), 0 if b else 1) for b in seq_a]       # zero flag bit = (value == 0)
    ctx += [csym(AC4, ctx_prior(AC4, color=1, inner=8), 0 if b else 1) for b in seq_b]
    p1 = _pics_of(host)
    n = (len(ctx) + MAX_CTX - 1) // MAX_CTX
    p2 = Picture.from_lists([([splice()], ctx[i * MAX_CTX:(i + 1) * MAX_CTX]) for i in range(n)])
    return [[p1, p2]]


def scenario_e(n_cells=80000, passes=3, seed=5):
    """a stream touching n_cells coefficient priors (one DynProb each: value 0 = one zero-flag decision), in `passes` passes in
    different orders, with a few other decisions between"""
    rng = np.random.default_rng(seed)
    ids = rng.choice(5 * 16 * 3 * 16 * 125, n_cells, replace=False)
    st, r = ids // (16 * 3 * 16 * 125), ids % (16 * 3 * 16 * 125)
    mbc, r = r // (3 * 16 * 125), r % (3 * 16 * 125)
    color, r = r // (16 * 125), r % (16 * 125)
    em, inner = r // 125, r % 125
    pr = ((((st * 16 + mbc) * 3 + color) * 16 + em) * 3125 + inner * 25 + 12).astype(np.uint32)
    rows = []
    for p in range(passes):
        o = rng.permutation(n_cells)
        s = np.zeros(n_cells, SYM)
        s["prior"], s["kind"] = pr[o], AC4
        s["value"] = np.where(rng.random(n_cells) < 0.8, 0, 1)
        s["pad"] = 0
        rows.append(s)
    allc = np.concatenate(rows)
    n = len(allc) // MAX_CTX
    allc = allc[:n * MAX_CTX].reshape(n, MAX_CTX)
    host = np.zeros((n, 1), SYM)
    host["prior"], host["kind"], host["pad"] = prior(TB_STOP, 5), BIT, 2
    return [[stacked_picture(host, allc, splice_at=1)]]


def raw_list(n, tag, rng=None, value=None):
    """a picture whose tag `tag` gets exactly n decisions, all raw bits (16 per symbol), random or constant"""
    nfull, rest = divmod(n, 16)
    vals = rng.integers(0, 1 << 16, nfull).astype(np.uint16).view(np.int16) if value is None else np.full(nfull, value, np.int16)
    s = np.zeros(nfull + (1 if rest else 0), SYM)
    s["prior"][:nfull], s["value"][:nfull] = 16, vals
    if rest:
        s["prior"][nfull], s["value"][nfull] = rest, 0x2a5 & ((1 << rest) - 1)
    s["kind"], s["pad"] = RAW, tag
    nmb = (len(s) + MAX_SYN - 1) // MAX_SYN
    s = np.concatenate([s, np.zeros(nmb * MAX_SYN - len(s), SYM)])
    s["kind"][len(s) - (nmb * MAX_SYN - (nfull + (1 if rest else 0))):] = RAW            # the filler: raw symbols of width 0
    s["pad"][:] = tag
    return stacked_picture(s.reshape(nmb, MAX_SYN))


def bit_list(n, tag, bits, index=9):
    """a picture whose tag gets n BIT decisions on ONE DynProb (bits: an array of n)"""
    s = np.zeros(n, SYM)
    s["prior"], s["value"], s["kind"], s["pad"] = prior(TB_STOP, index), bits, BIT, tag
    nmb = (n + MAX_SYN - 1) // MAX_SYN
    rows = np.zeros(nmb * MAX_SYN, SYM)
    rows[:n] = s
    rows["kind"][n:], rows["pad"][n:] = RAW, tag            # filler: raw symbols of width 0 (no decision)
    return stacked_picture(rows.reshape(nmb, MAX_SYN))


LIST_SIZES = [m - 32 + d for m in (256, 512, 65536, 131072, 262144) for d in (-1, 0, 1)]


def scenario_g_small(seed=7):
    """one stream per list length: tag 69 gets n decisions with n + 32 at multiples of 256 and 65,536 (+-1) and 262,144 (+-1)"""
    rng = np.random.default_rng(seed)
    return [[raw_list(n, 69, rng)] for n in LIST_SIZES]


def scenario_gh_large(per_stream=4_400_000, seed=8):
    """two streams of about 4.4 M list entries each (the call's average above 4 M: long_list = 65,536); per stream a skewed list on one
    DynProb - stream 0: zeros only (probability 255: the range states only rotate, the whole state map), stream 1: a one every 300th
    decision (coded at probability 254-255: every state merges into one, one candidate) -, a mixed one (a biased source on one DynProb)
    and an incompressible one (random raw bits: several candidates)"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(2):
        a = per_stream // 3
        skew = bit_list(a, 2, np.zeros(a, np.int16) if s == 0 else (np.arange(a) % 300 == 299).astype(np.int16), index=11 + s)
        mixed = bit_list(a, 8, (rng.random(a) < 0.2 + 0.6 * (np.arange(a) // 70000 % 2)).astype(np.int16), index=300 + s)
        noise = raw_list(per_stream - 2 * a, 69, rng)
        out.append([skew, mixed, noise])
    return out


CARRY_D0 = 134


def carry_bits(carry=True, n=2700):
    """decisions at probability 128 that keep the coder's interval across one boundary of its low register for n decisions: a run of
    0xff bytes, then (carry) a decision that pushes low over it - or none"""
    norm = [0] + [7 - (r.bit_length() - 1) for r in range(1, 256)]
    r, D, bits = 255, CARRY_D0, []
    while True:
        split = 1 + (((r - 1) * 128) >> 8)
        if len(bits) >= n and 0 < D < split:
            bits.append(1 if carry else 0)
            break
        b = 1 if D > split else 0
        assert D != split
        if b:
            D, r = D - split, r - split
        else:
            r = split
        bits.append(b)
        s = norm[r]
        r, D = r << s, D << s
    return bits + [0] * 16


def scenario_i():
    """the zero flags of coefficient symbols on fresh priors (probability 128 each) spell carry_bits: tag 30 (chroma BITMASK) gets
    a carry through a run of > 300 0xff bytes; tag 25 (luma BITMASK) the same run without the carry"""
    out = []
    for color, carry in ((1, True), (0, False)):
        bits = carry_bits(carry)
        ctx = [csym(AC4, ctx_prior(AC4, mbc=(i // 1875) % 16, color=color, emitted=1 + (i // 125) % 15, inner=(i % 125) * 25),
                    0 if b else 1) for i, b in enumerate(bits)]                   # every prior once: probability 128
        n = (len(ctx) + MAX_CTX - 1) // MAX_CTX
        out.append(Picture.from_lists([([splice()], ctx[k * MAX_CTX:(k + 1) * MAX_CTX]) for k in range(n)]))
    return [out]


# ---- the reference's own coder (oracle/ref_coder.cpp, built into oracle/_ref by oracle/Makefile when the reference is present) -------
REF_CODER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libref_coder.so")
REC = np.dtype([("kind", "<i4"), ("cell", "<i4"), ("value", "<i4"), ("tag", "<i4"), ("aux", "<i4")])
TREE_BITS = {t[0]: t[1] for t in TREES}


def ref_records(stream):
    """the flattened stream as refc_rec records: the product's priors numbered as cells of the reference's prior types"""
    f = flatten(stream)
    n = len(f)
    kind, pr, pad = f["kind"].astype(np.int64), f["prior"].astype(np.int64), f["pad"].astype(np.int64)
    table = pr >> 27
    rk = np.full(n, -1, np.int64)
    tag = pad.copy()
    aux = np.zeros(n, np.int64)
    rk[(kind == LDC) | (kind == CDC)] = 0
    tag[kind == LDC], tag[kind == CDC] = 17, 18
    nz = (kind == NZ4) | (kind == NZ8)
    rk[nz] = 1
    tag[nz] = np.where((pr[nz] // 27) % 3 != 0, 29, 19)
    ac = (kind == AC4) | (kind == AC8)
    rk[ac] = 2
    tag[ac] = [implied_tag(int(k), int(p)) for k, p in zip(kind[ac], pr[ac])]
    rk[kind == MVD] = 3
    for tb, bits in TREE_BITS.items():
        rk[(kind == TREE) & (table == tb)] = 3 + bits
    m8, qp = (kind == POW2) & (table == TB_MODE8), (kind == POW2) & (table == TB_QPL)
    rk[m8], rk[qp] = 13, 14
    aux[m8] = pr[m8] & 0x7ffffff
    rk[kind == BIT] = 15
    raw_ = kind == RAW
    rk[raw_], aux[raw_] = 16, pr[raw_]
    assert (rk >= 0).all(), "a symbol outside the domain"
    # one cell per (kind of prior, table + index / flat coefficient index) - as the oracle and the device key them
    fam = np.where(rk >= 4, 4, rk)
    _, cell = np.unique(fam * (1 << 36) + np.where(rk <= 2, kind << 32, 0) + pr, return_inverse=True)
    out = np.zeros(n, REC)
    out["kind"], out["cell"], out["value"], out["tag"], out["aux"] = rk, cell, f["value"], tag, aux
    return out


def ref_code(stream):
    """the stream through the reference's coder -> {tag: bytes}"""
    L = C.CDLL(REF_CODER)
    L.refc_code.argtypes, L.refc_code.restype = [C.c_void_p, C.c_long], C.c_int
    L.refc_tag.argtypes, L.refc_tag.restype = [C.c_int, C.POINTER(C.c_long)], C.POINTER(C.c_uint8)
    r = np.ascontiguousarray(ref_records(stream))
    assert L.refc_code(r.ctypes.data, len(r)) == 0
    tags = {}
    for t in TAG_OF_SLOT:
        ln = C.c_long()
        p = L.refc_tag(t, C.byref(ln))
        if ln.value:
            tags[t] = bytes(np.ctypeslib.as_array(p, (ln.value,)))
    return tags
