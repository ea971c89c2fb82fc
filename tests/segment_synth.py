"""A stream coded in segments (lh264_code_chains_resume): staging and bookkeeping for tests/test_segments_gpu.py, and the fixtures whose
cuts fall at awkward places.  The pictures, the oracle and the unsegmented device call come from tests/coder_synth.py.

A picture of coder_synth is a list of macroblocks, and the coder's symbol stream is the macroblocks' symbols one after the other: a
picture cut into several pictures at macroblock boundaries (`split_picture`) is the same stream with more places to cut it."""
import numpy as np

import coder_synth as S

FIRST, LAST = 1, 2


def split_picture(pic, bounds):
    """pic cut into pictures of macroblocks [b0, b1), [b1, b2), ... (bounds: increasing macroblock indices strictly inside the picture)"""
    edges = [0] + [int(b) for b in bounds] + [pic.n_mbs]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        assert a <= b
        h0, h1 = int(pic.host_off[a]), int(pic.host_off[b])
        c0, c1 = int(pic.ctx_off[a]), int(pic.ctx_off[b])
        out.append(S.Picture(pic.host[h0:h1], pic.host_off[a:b + 1] - pic.host_off[a], pic.ctx[c0:c1], pic.ctx_n[a:b]))
    return out


def even_cuts(n_pics, parts):
    """picture indices that cut n_pics pictures into `parts` about equal runs (fewer when there are not enough pictures)"""
    return sorted({(n_pics * k) // parts for k in range(1, parts)} - {0, n_pics})


class Staged:
    """the pictures of some streams in device memory: `jobs` (host copy of their lh264_code_job_t, stream after stream), first[c]"""

    def __init__(self, jobs, first, keep, dev):
        self.jobs, self.first, self.keep, self.dev = jobs, np.asarray(first, np.int64), keep, dev
        self.n_streams = len(first) - 1

    def n_pics(self, c):
        return int(self.first[c + 1] - self.first[c])


def stage(streams, dev=0):
    """coder_synth streams -> Staged (the compact symbol pool, as coder_synth.device lays it out)"""
    import torch
    from losslessh264_amd import _lib as L
    L.check(L.lib().lh264_set_device(dev))
    d = torch.device("cuda", dev)
    pics = [p for s in streams for p in s]
    SYM = S.SYM
    host = np.concatenate([p.host for p in pics] + [np.zeros(1, SYM)])
    hoff = np.concatenate([p.host_off for p in pics] + [np.zeros(1, np.uint32)])
    cn = np.concatenate([p.ctx_n for p in pics] + [np.zeros(1, np.uint16)])
    runs = [((p.ctx_n.astype(np.int64) + 7) // 8) * 8 for p in pics]
    offs = [np.concatenate([[0], np.cumsum(r)[:-1]]) if len(r) else np.zeros(0, np.int64) for r in runs]
    bases = np.concatenate([[0], np.cumsum([int(r.sum()) for r in runs])]).astype(np.uint64) + 8
    ctx = np.zeros(int(bases[-1]) + 1, SYM)
    for p, o, b in zip(pics, offs, bases):
        dst = int(b) + np.repeat(o, p.ctx_n) + np.arange(len(p.ctx)) - np.repeat(p.ctx_off[:-1], p.ctx_n)
        ctx[dst] = p.ctx
    symoff = np.concatenate(offs + [np.zeros(1, np.int64)]).astype(np.uint32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(d)
    keep = [t(host), t(hoff), t(ctx), t(cn), t(symoff), t(bases)]
    d_host, d_hoff, d_ctx, d_cn, d_symoff, d_bases = keep
    jobs = np.zeros(len(pics), L.CODE_JOB_DTYPE)
    hs = ho = mo = 0
    for j, p in enumerate(pics):
        jobs[j]["syn_syms"], jobs[j]["syn_off"] = d_host.data_ptr() + hs * 8, d_hoff.data_ptr() + ho * 4
        jobs[j]["ctx_n_syms"], jobs[j]["n_mbs"] = d_cn.data_ptr() + mo * 2, p.n_mbs
        jobs[j]["ctx_syms"], jobs[j]["ctx_sym_off"] = d_ctx.data_ptr(), d_symoff.data_ptr() + mo * 4
        jobs[j]["ctx_sym_base"] = d_bases.data_ptr() + j * 8
        hs += len(p.host); ho += p.n_mbs + 1; mo += p.n_mbs
    first = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
    return Staged(jobs, first, keep, dev)


def stage_session(coder):
    """the pictures of a losslessh264_amd.CoderSession (real streams: parsed, context-indexed on the device) -> Staged"""
    from losslessh264_amd import _lib as L
    jobs = coder.d_jobs.cpu().numpy().view(L.CODE_JOB_DTYPE).copy()
    first = coder.ctx.d_first.cpu().numpy().view(np.int32).astype(np.int64)[:coder.n_chains + 1]
    return Staged(jobs, first, [coder, coder.ctx], coder.ctx.dev.index or 0)


class SegRun:
    """the streams of a Staged, each with its carry block, its output buffer and its lengths kept between calls"""

    def __init__(self, staged, hash_cap=1 << 16, out_cap=1 << 16):
        import torch
        from losslessh264_amd import _lib as L
        self.G, self.L, self.lib, self.torch = staged, L, L.lib(), torch
        self.d = torch.device("cuda", staged.dev)
        n = staged.n_streams
        self.hash_cap, self.out_cap = hash_cap, out_cap
        self.carry_bytes = int(self.lib.lh264_code_carry_bytes(hash_cap))
        self.carry = [torch.zeros(self.carry_bytes, dtype=torch.uint8, device=self.d) for _ in range(n)]      # (the caller zero-fills)
        self.out = torch.full((n * S.N_SLOTS * out_cap + S.GUARD,), S.SENTINEL, dtype=torch.uint8, device=self.d)
        self.len = torch.zeros(n * (S.N_SLOTS + 1), dtype=torch.int32, device=self.d)
        self.calls = 0

    def call(self, parts):
        """ONE lh264_code_chains_resume: parts = [(stream, j0, j1, flags)], pictures j0 .. j1-1 of the stream as its next segment"""
        L, torch, G = self.L, self.torch, self.G
        jobs, first, sd, carry, flags = [], [0], np.zeros(len(parts), L.CODE_STREAM_DTYPE), [], []
        for k, (c, j0, j1, fl) in enumerate(parts):
            jobs.append(G.jobs[G.first[c] + j0:G.first[c] + j1])
            first.append(first[-1] + (j1 - j0))
            sd[k]["out"], sd[k]["out_len"] = self.out.data_ptr() + c * S.N_SLOTS * self.out_cap, self.len.data_ptr() + c * (S.N_SLOTS + 1) * 4
            sd[k]["hash_cap"], sd[k]["out_cap"] = self.hash_cap, self.out_cap
            carry.append(self.carry[c].data_ptr()); flags.append(fl)
        jobs = np.concatenate(jobs) if jobs else np.zeros(0, L.CODE_JOB_DTYPE)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(self.d)
        d_jobs = t(jobs if len(jobs) else np.zeros(1, L.CODE_JOB_DTYPE))
        d_first, d_sd = t(np.array(first, np.int32)), t(sd)
        d_carry, d_flags = t(np.array(carry, np.uint64)), t(np.array(flags, np.uint32))
        total = int(jobs["n_mbs"].sum())
        maxm = int(max([1] + [int(x) for x in jobs["n_mbs"]]))
        s = torch.cuda.current_stream(self.d).cuda_stream
        torch.cuda.synchronize(self.d)
        L.check(self.lib.lh264_code_chains_resume(d_jobs.data_ptr(), d_first.data_ptr(), d_sd.data_ptr(), d_carry.data_ptr(), d_flags.data_ptr(),
                                                  len(parts), len(jobs), total, maxm, s))
        torch.cuda.synchronize(self.d)
        self.calls += 1

    def run_cuts(self, cuts_of):
        """every stream in segments, the k-th segments of all streams in the k-th call: cuts_of(c) = picture indices where stream c is cut"""
        cuts = [[0] + list(cuts_of(c)) + [self.G.n_pics(c)] for c in range(self.G.n_streams)]
        for k in range(max(len(x) for x in cuts) - 1):
            parts = []
            for c, x in enumerate(cuts):
                if k < len(x) - 1:
                    parts.append((c, x[k], x[k + 1], (FIRST if k == 0 else 0) | (LAST if k == len(x) - 2 else 0)))
            self.call(parts)
        return self.results()

    def lens(self):
        return self.len.cpu().numpy().reshape(self.G.n_streams, S.N_SLOTS + 1)

    def carry_words(self, c):
        """the header and tag records of stream c's carry block (csrc/lh264_coder.h: 16 header words, 8 per tag slot: bits (64), decisions
        (64), range, exists)"""
        w = self.carry[c][:(16 + 8 * S.N_SLOTS) * 4].cpu().numpy().view(np.uint32)
        return w[:16], w[16:].reshape(S.N_SLOTS, 8)

    def slot_bytes(self, c, slot, n):
        b = (c * S.N_SLOTS + slot) * self.out_cap
        return self.out[b:b + n].cpu().numpy().tobytes()

    def decisions(self, c):
        import ctypes as C
        out = (C.c_uint64 * S.N_SLOTS)()
        self.L.check(self.lib.lh264_code_carry_decisions(self.carry[c].data_ptr(), out, self.torch.cuda.current_stream(self.d).cuda_stream))
        return list(out)

    def results(self):
        lens, out = self.lens(), self.out.cpu().numpy()
        res = []
        for c in range(self.G.n_streams):
            tags = {}
            for slot, tag in enumerate(S.TAG_OF_SLOT):
                ln = int(lens[c, slot])
                if ln:
                    b = (c * S.N_SLOTS + slot) * self.out_cap
                    tags[tag] = out[b:b + min(ln, self.out_cap)].tobytes()
            res.append(S.DeviceResult(lens[c, :35].copy(), int(lens[c, S.N_SLOTS]), tags, None))
        assert (lens[:, 35:S.N_SLOTS] == 0).all(), "tag slots beyond 34 were written"
        assert (out[self.G.n_streams * S.N_SLOTS * self.out_cap:] == S.SENTINEL).all(), "written behind the output buffers"
        return res


# ---- cuts at awkward places --------------------------------------------------------------------------------------------------------
def carry_into_ff_run():
    """coder_synth.scenario_i's stream (tag 30: a run of 0xff bytes and then ONE decision that carries through all of it; tag 25: the same
    run without the carry) with the cut exactly in front of the carrying decision: the first segment ends with the run as tag 30's last
    bytes, and the first addend of the second segment carries into them.  -> (streams, decisions of tag 30 in the first segment)"""
    bits = S.carry_bits(True)
    at = len(bits) - 17                                    # the decision that pushes `low` over the run (carry_bits: 16 zeros follow it)
    assert bits[at] == 1
    ctx = [S.csym(S.AC4, S.ctx_prior(S.AC4, mbc=(i // 1875) % 16, color=1, emitted=1 + (i // 125) % 15, inner=(i % 125) * 25), 0 if b else 1)
           for i, b in enumerate(bits)]                    # every prior once: probability 128 (the symbols of scenario_i)
    pic = lambda cs: S.Picture.from_lists([([S.splice()], cs[k:k + S.MAX_CTX]) for k in range(0, len(cs), S.MAX_CTX)])
    return [[pic(ctx[:at]), pic(ctx[at:]), S.scenario_i()[0][1]]], at


def late_and_absent_tags(rng):
    """four pictures: tag 2 everywhere; tag 8 only in pictures 2 and 3 (it comes into existence in a later segment); tag 69 in pictures 0
    and 3 only (no decision at all in the segments between); picture 1 is a single macroblock with one decision"""
    p0 = S.Picture.from_lists([([S.hsym(S.BIT, S.TB_STOP, 5, int(b), 2) for b in rng.integers(0, 2, 90)] + [S.raw(16, 0x1234, 69)] * 3, [])] * 3)
    p1 = S.Picture.from_lists([([S.hsym(S.BIT, S.TB_STOP, 5, 1, 2)], [])])
    p2 = S.Picture.from_lists([([S.hsym(S.BIT, S.TB_STOP, 5, int(b), 2) for b in rng.integers(0, 2, 40)] +
                                [S.hsym(S.BIT, S.TB_T8, 7, int(b), 8) for b in rng.integers(0, 2, 50)], [])] * 2)
    p3 = S.Picture.from_lists([([S.hsym(S.BIT, S.TB_T8, 7, int(b), 8) for b in rng.integers(0, 2, 30)] + [S.raw(16, -2, 69)] * 4 +
                                [S.hsym(S.BIT, S.TB_STOP, 5, 0, 2)], [])] * 2)
    return [[p0, p1, p2, p3]]
