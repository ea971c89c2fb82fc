// lh264_compress.hip - the compress direction behind one C call (include/lh264.h: lh264_compress_batch): the host
// orchestration the reference does inside its decoder loop (decode_slice.cpp:3085-3112 per macroblock, flushToWriter at
// the end), here per batch of independent streams: parse on host threads, stage records and symbol lists in HBM, one
// launch of the context-index kernels and one of the coder kernel, copy the tagged streams back.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <mutex>
#include <deque>
#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <thread>
#include <string>
#include <vector>
#include "../../include/lh264.h"
#include "host/h264_parser.h"
#include "host/capi_internal.h"
#include "host/device_mem.h"
#include "lh264_coder.h"

struct lh264_compressed {
  int status = LH264_OK;
  std::string error;
  std::vector<uint8_t> main_stream;
  std::vector<uint8_t> tag[72];
  bool has_tag[72] = {false};
  int pictures = 0;
  int segments = 0;                              // coder calls the stream's pictures went through (1: whole)
  uint64_t decisions[LH264_N_TAG_SLOTS] = {0};   // per tag slot, summed over the segments
};

// gathers the tagged streams of a group (one workgroup per stream and tag) into one buffer: one download instead of thousands
struct PackItem { uint64_t src, dst; uint32_t len, pad; };      // src: device address of the bytes; dst: offset in the packed buffer
__global__ void __launch_bounds__ (256) pack_tags_kernel (const PackItem* __restrict__ items, uint8_t* __restrict__ packed) {
  const PackItem it = items[blockIdx.x];
  const uint8_t* s = (const uint8_t*) (uintptr_t)it.src; uint8_t* d = packed + it.dst;
  for (uint32_t i = threadIdx.x; i < it.len; i += blockDim.x) d[i] = s[i];
}

// A long stream between two segments: the bytes of a tag that are final have gone to the host, what is left - the last byte that is not
// 0xff, the 0xff bytes behind it, and the two bytes the next segment's sums start from - moves to the front of the tag's buffer and the
// carry counts its bits from there.  One wave per (stream, tag slot); chunks in ascending order, each read whole before it is written
// (the destination lies below the source).
struct RebaseItem { uint8_t* out; uint32_t* carry; const uint32_t* lens; uint32_t cap, pad; };
__global__ void __launch_bounds__ (64) rebase_tags_kernel (const RebaseItem* __restrict__ items) {
  const RebaseItem it = items[blockIdx.x / 35u];
  const uint32_t slot = blockIdx.x % 35u, lane = threadIdx.x;
  uint32_t* rec = it.carry + LH264_CARRY_HDR_WORDS + slot * LH264_CARRY_TAG_WORDS;
  const uint32_t fin = it.lens[slot];
  if (!rec[LH264_CARRY_TAG_EXISTS] || fin == 0u) return;
  const unsigned long long bits = (unsigned long long)rec[LH264_CARRY_TAG_BITS] | (unsigned long long)rec[LH264_CARRY_TAG_BITS + 1] << 32;
  const unsigned long long end = bits / 8 + 2;
  const uint32_t n = (uint32_t) (end < it.cap ? end : it.cap);
  uint8_t* o = it.out + (size_t)slot * it.cap;
  for (uint32_t k = fin; k < n; k += 64u) {
    const uint32_t v = k + lane < n ? o[k + lane] : 0u;
    __syncthreads();
    if (k + lane < n) o[k + lane - fin] = (uint8_t)v;
    __syncthreads();
  }
  if (lane == 0u) { const unsigned long long b = bits - 8ull * fin; rec[LH264_CARRY_TAG_BITS] = (uint32_t)b; rec[LH264_CARRY_TAG_BITS + 1] = (uint32_t) (b >> 32); }
}

namespace {

using lh264host::DevBuf;
using lh264host::PinBuf;
using lh264host::now_s;
bool trace_on() { static const bool t = lh264host::trace_on ("LH264_TRACE_COMPRESS"); return t; }

struct Arena {
  DevBuf d_mbs, d_lev, d_sl, d_nnz, d_syms, d_nsyms, d_symoff, d_symbase, d_cj, d_first, d_syn, d_off, d_kj, d_st, d_keys, d_cells, d_out, d_len, d_items, d_packed;
  DevBuf d_keep;                                // LH264_COMPRESS_TOLERANT: the KEEP image of every picture (lh264_ctx_index_chains_keep)
  PinBuf h_mbs, h_sparse, h_sl, h_syn, h_off, h_packed;
  DevBuf d_sparse;
  DevBuf d_rebase;
  DevBuf d_carry, d_flags;                      // groups with a segment of a long stream: the carry blocks' addresses, the streams' flags
  size_t device_bytes() const {
    size_t n = d_sparse.cap + d_carry.cap + d_flags.cap + d_rebase.cap + d_keep.cap;
    for (const DevBuf* b : {&d_mbs, &d_lev, &d_sl, &d_nnz, &d_syms, &d_nsyms, &d_symoff, &d_symbase, &d_cj, &d_first, &d_syn, &d_off, &d_kj, &d_st, &d_keys, &d_cells, &d_out, &d_len, &d_items, &d_packed}) n += b->cap;
    return n;
  }
  size_t pinned_bytes() const { return h_mbs.cap + h_sparse.cap + h_sl.cap + h_syn.cap + h_off.cap + h_packed.cap; }
  size_t long_bytes = 0;                        // most device memory the long streams of a call held beside the buffers above
};

// A stream that is coded in segments (more macroblocks than a segment holds): what outlives a group.  Device memory of its own - the
// carry block of lh264_code_chains_resume, the tagged streams' bytes so far, the lengths -, the nnz images of the two pictures the
// reference's FreqImage holds (a later segment's first pictures name them as PAST), and where the PAST policy stands.
struct LongStream {
  int i = 0;                                    // the stream's place in the batch
  uint32_t hash_cap = 0, out_cap = 0;
  DevBuf carry, outb, lens, nnz[2];
  int cur = 0, last_fn = 0; long slot[2] = {-1, -1};          // past_policy, continued: the pictures (counted over the stream) in the two buffers
  int pol_w = 0, pol_h = 0;                     // ... and the size of the last picture (tolerant: a change of size empties both buffers)
  long pics_done = 0;                           // pictures handed to the coder so far
  size_t seg_mbs = 0;                           // the segment size of the call (sizes the output buffers)
  size_t max_pics = (size_t)-1;                 // a segment over one of the coder's counters is sent again with half the pictures
  std::deque<std::unique_ptr<lh264host::FrameOut>> pending;     // parsed, not yet coded
  bool started = false, ended = false;
  // a failure is noted here by whoever meets it (the device stage, a parsing thread) and becomes the stream's result in ONE place, where
  // the next group is cut (lh264_compress_batch_opts: the tags of the segments before are dropped - the result is the error, never a partial file)
  std::atomic<bool> failed {false};
  std::mutex fail_mu; int fail_code = 0; std::string fail_text;
  void fail (int code, const std::string& text) { std::lock_guard<std::mutex> g (fail_mu); if (!failed) { fail_code = code; fail_text = text; failed = true; } }
  size_t device_bytes() const { return carry.cap + outb.cap + lens.cap + nnz[0].cap + nnz[1].cap; }
};
// one chain of a group: a whole stream (ls == nullptr) or the next segment of a long one
struct Part {
  int i = 0;
  std::vector<std::unique_ptr<lh264host::FrameOut>> frames;
  LongStream* ls = nullptr;
  uint32_t flags = LH264_CODE_SEG_FIRST | LH264_CODE_SEG_LAST;
  bool again = false;                           // out: status 8 with more than one picture - nothing was coded, the pictures go back
  // left by the staging of compress_group for where its results are read: the PAST policy behind the part's last picture (a long
  // stream takes it over once the segment is coded) and the first macroblock of every picture in the group's buffers
  int cur = 0, last_fn = 0; long slot[2] = {-1, -1}; int pol_w = 0, pol_h = 0;
  std::vector<size_t> mb_at;
};

// which earlier picture the reference's FreqImage holds as PAST (decoded_macroblock.h:119-123): two buffers, flipped when
// frame_num changes; -1 = none
// For a segment of a long stream the walk starts where the segment before left it: pictures count from the stream's first one, base = the
// segment's first; past[i] < base: that picture's image is in the stream's buffer past_buf[i].
// keep[i]: the picture that last occupied the buffer picture i goes to, slot[cur] before the picture is entered - the picture before when
// frame_num did not change, else the one two flips back; a cell no slice of picture i writes holds that picture's entry (KEEP), in the
// stream's buffer 1 - past_buf[i] when keep[i] < base.  size: {w, h} of the picture before, continued like the rest; given (tolerant), a
// change of size empties both buffers as the restorers do (decode_slice.cpp:3035-3046) - PAST and KEEP of one size never meet a picture
// of another
void past_policy (const std::vector<std::unique_ptr<lh264host::FrameOut>>& fr, std::vector<long>& past, std::vector<int>& past_buf, std::vector<long>& keep, long base, int& cur, int& last_fn, long slot[2], int* size) {
  past.resize (fr.size()); past_buf.resize (fr.size()); keep.resize (fr.size());
  for (size_t i = 0; i < fr.size(); i++) {
    if (fr[i]->frame_num != last_fn) { cur ^= 1; last_fn = fr[i]->frame_num; }
    if (size && (size[0] != fr[i]->mb_w || size[1] != fr[i]->mb_h)) { slot[0] = slot[1] = -1; size[0] = fr[i]->mb_w; size[1] = fr[i]->mb_h; }
    past[i] = slot[1 - cur]; past_buf[i] = 1 - cur; keep[i] = slot[cur];
    slot[cur] = base + (long)i;
  }
}

void fail_all (lh264_compressed_t** out, std::vector<Part>& parts, int code, const char* what) {
  for (Part& p : parts) { if (p.ls) p.ls->fail (code, what); else { out[p.i]->status = code; out[p.i]->error = what; } }
}

// one sub-batch: whole streams and segments of long ones, all parsed without error.  A group without a segment is coded by
// lh264_code_chains as ever; with one, by lh264_code_chains_resume, the whole streams as FIRST | LAST beside the segments.
void compress_group (Arena& A, std::vector<Part>& parts, const size_t* len, lh264_compressed_t** out, int threads, bool tolerant) {
  using lh264host::FrameOut;
  const int n_chains = (int)parts.size();
  std::vector<int> idx (n_chains);
  bool resumable = false;
  for (int c = 0; c < n_chains; c++) { idx[c] = parts[c].i; resumable = resumable || parts[c].ls; }
  // where every stream's records go
  std::vector<size_t> mb0 (n_chains + 1, 0), sl0 (n_chains + 1, 0), sy0 (n_chains + 1, 0), of0 (n_chains + 1, 0), jb0 (n_chains + 1, 0), sp0 (n_chains + 1, 0);
  int max_mbs = 1;
  for (int c = 0; c < n_chains; c++) {
    size_t m = 0, sl = 0, sy = 0, of = 0, jb = 0, sp = 0;
    for (auto& f : parts[c].frames) {
      const size_t n = (size_t)f->mb_w * f->mb_h;
      m += n; sl += f->slices.size(); sy += f->syn_syms.size(); of += n + 1; jb++; sp += f->sparse.size();
      max_mbs = std::max (max_mbs, (int)n);
    }
    sp0[c + 1] = sp0[c] + sp;
    mb0[c + 1] = mb0[c] + m; sl0[c + 1] = sl0[c] + sl; sy0[c + 1] = sy0[c] + sy; of0[c + 1] = of0[c] + of; jb0[c + 1] = jb0[c] + jb;
  }
  const size_t n_sparse = sp0[n_chains];
  const size_t n_mbs = mb0[n_chains], n_slices = sl0[n_chains], n_syn = sy0[n_chains], n_off = of0[n_chains], n_jobs = jb0[n_chains];
  if (n_jobs == 0 && !resumable) return;
  std::vector<lh264_ctx_job_t> h_cj (n_jobs);
  std::vector<lh264_code_job_t> h_kj (n_jobs);
  std::vector<int32_t> h_first (n_chains + 1);
  std::vector<const uint8_t*> h_keep (tolerant ? n_jobs : 0);
  std::vector<lh264_code_stream_t> h_st (n_chains);
  std::vector<uint32_t> hash_cap (n_chains), out_cap (n_chains);
  std::vector<size_t> key0 (n_chains + 1, 0), out0 (n_chains + 1, 0);
  for (int c = 0; c < n_chains; c++) {
    const size_t mbs = mb0[c + 1] - mb0[c];
    uint32_t hc = 1u << 13;                                   // 8 spill entries per cell: four entries per input byte (a stream touches
    while ((size_t)hc * 2 < len[idx[c]] && hc < (1u << 20)) hc <<= 1;      // 0.2 .. 0.5 adaptive probabilities per byte); status 1 reports a full table
    hash_cap[c] = hc;
    const size_t want_cap = std::max<size_t> (1u << 16, 2 * len[idx[c]] + 4096);
    out_cap[c] = (uint32_t)std::min<size_t> (want_cap, 0xffffffffu);
    // (a long stream's table, bytes and lengths are its own; a whole stream in a resumable call has a carry block in front of its table)
    key0[c + 1] = key0[c] + (parts[c].ls ? 0 : (size_t)hc + (resumable ? LH264_CARRY_TABLE_BYTES / 64 : 0));
    out0[c + 1] = out0[c] + (parts[c].ls ? 0 : (size_t)LH264_N_TAG_SLOTS * out_cap[c]);
    if (LongStream* ls = parts[c].ls) {
      if (!ls->started) {
        // the tag buffers of a long stream hold what ONE segment writes (its final bytes go to the host segment by segment): a coded
        // macroblock is at most 3,200 bits of input (I_PCM samples do not pass the coder), and no tag's bytes exceed the input's by more
        // than the slack; status 4 reports a buffer that was too small
        const size_t seg = std::max (ls->seg_mbs, (size_t) (mb0[c + 1] - mb0[c]));
        // (... and one call codes fewer than 2^27 decisions into a stream's lists, each of which shifts out 7 bits at most)
        out_cap[c] = (uint32_t)std::max<size_t> (1u << 16, std::min<size_t> ({want_cap, 400 * seg + 65536, ((size_t)7 << 24) + 65536}));
        ls->hash_cap = hc; ls->out_cap = out_cap[c];
        if (!(ls->carry.alloc (lh264_code_carry_bytes (hc)) && ls->carry.zero (lh264_code_carry_bytes (hc), nullptr) && ls->outb.alloc ((size_t)35 * out_cap[c])      /* (the tag slots that exist) */ &&
              ls->lens.alloc ((LH264_N_TAG_SLOTS + 1) * 4) && ls->lens.zero ((LH264_N_TAG_SLOTS + 1) * 4, nullptr))) {
          fail_all (out, parts, LH264_E_HIP, "device allocation failed"); return;
        }
        ls->started = true;
      }
      hash_cap[c] = ls->hash_cap; out_cap[c] = ls->out_cap;
    }
  }
  static_assert (LH264_CARRY_TABLE_BYTES % 64 == 0, "carry blocks are laid out in units of table cells");
  std::vector<void*> h_carry (n_chains);
  std::vector<uint32_t> h_flags (n_chains);
  const size_t keys_total = key0[n_chains], out_total = out0[n_chains];
  const double t_a = now_s();
  const bool ok = A.d_mbs.alloc (n_mbs * sizeof (lh264_mb_t)) && A.d_lev.alloc (n_mbs * 768) && A.d_lev.zero (n_mbs * 768, nullptr) && A.d_sparse.alloc (n_sparse * 8) && A.d_sl.alloc (n_slices * sizeof (lh264_slice_t)) &&
                  A.d_nnz.alloc (n_mbs * 24) && A.d_nnz.zero (n_mbs * 24, nullptr) && A.d_nsyms.alloc (n_mbs * 2) && A.d_nsyms.zero (n_mbs * 2, nullptr) && A.d_symoff.alloc (n_mbs * 4) && A.d_symbase.alloc ((n_jobs + 2) * 8) &&
                  A.d_cj.alloc (n_jobs * sizeof (lh264_ctx_job_t)) && A.d_first.alloc ((n_chains + 1) * 4) && A.d_syn.alloc (n_syn * sizeof (lh264_ctx_sym_t)) &&
                  A.d_off.alloc (n_off * 4) && A.d_kj.alloc (n_jobs * sizeof (lh264_code_job_t)) && A.d_st.alloc (n_chains * sizeof (lh264_code_stream_t)) &&
                  A.d_keys.alloc (256) && A.d_cells.alloc (keys_total * 64) && A.d_cells.zero (keys_total * 64, nullptr) && A.d_out.alloc (out_total) &&
                  A.d_len.alloc ((size_t)n_chains * (LH264_N_TAG_SLOTS + 1) * 4) && A.d_len.zero ((size_t)n_chains * (LH264_N_TAG_SLOTS + 1) * 4, nullptr) &&
                  A.h_mbs.alloc (n_mbs * sizeof (lh264_mb_t)) && A.h_sparse.alloc (n_sparse * 8) && A.h_sl.alloc (n_slices * sizeof (lh264_slice_t)) &&
                  A.h_syn.alloc (n_syn * sizeof (lh264_ctx_sym_t)) && A.h_off.alloc (n_off * 4) &&
                  (!resumable || (A.d_carry.alloc (n_chains * sizeof (void*)) && A.d_flags.alloc (n_chains * 4))) &&
                  (!tolerant || A.d_keep.alloc (n_jobs * sizeof (void*)));
  if (!ok) { fail_all (out, parts, LH264_E_HIP, "device allocation failed"); return; }
  const double t_b = now_s();
  lh264_mb_t* h_mbs = A.h_mbs.as<lh264_mb_t>(); uint64_t* h_sparse = A.h_sparse.as<uint64_t>(); lh264_slice_t* h_sl = A.h_sl.as<lh264_slice_t>();
  lh264_ctx_sym_t* h_syn = A.h_syn.as<lh264_ctx_sym_t>(); uint32_t* h_off = A.h_off.as<uint32_t>();
  // staging: every stream copies its pictures to its place (host threads), and writes its job records
  run_parallel (n_chains, threads, [&] (int c) {
    auto& fr = parts[c].frames;
    LongStream* ls = parts[c].ls;
    size_t mo = mb0[c], so = sl0[c], yo = sy0[c], oo = of0[c], j = jb0[c], po = sp0[c];
    h_first[c] = (int32_t)j;
    std::vector<long> past, keep; std::vector<int> past_buf;
    Part& pt = parts[c];
    const long base = ls ? ls->pics_done : 0;
    // (a segment that has to be sent again must find the stream's policy as it was: the walk works on a copy in the part, which the
    // stream takes over when the segment was coded)
    pt.cur = 0; pt.last_fn = 0; pt.slot[0] = pt.slot[1] = -1; pt.pol_w = pt.pol_h = 0;
    if (ls) { pt.cur = ls->cur; pt.last_fn = ls->last_fn; pt.slot[0] = ls->slot[0]; pt.slot[1] = ls->slot[1]; pt.pol_w = ls->pol_w; pt.pol_h = ls->pol_h; }
    int pol_size[2] = {pt.pol_w, pt.pol_h};
    past_policy (fr, past, past_buf, keep, base, pt.cur, pt.last_fn, pt.slot, tolerant ? pol_size : nullptr);
    pt.pol_w = pol_size[0]; pt.pol_h = pol_size[1];
    std::vector<size_t>& mb_at = pt.mb_at;
    mb_at.resize (fr.size());
    for (size_t i = 0; i < fr.size(); i++) {
      FrameOut& f = *fr[i];
      const size_t n = (size_t)f.mb_w * f.mb_h;
      mb_at[i] = mo;
      memcpy (&h_mbs[mo], f.mbs.data(), n * sizeof (lh264_mb_t));
      { const uint64_t add = (uint64_t) (mo * 384) << 16; const size_t ns = f.sparse.size(); for (size_t q = 0; q < ns; q++) h_sparse[po + q] = f.sparse[q] + add; po += ns; }
      if (!f.slices.empty()) memcpy (&h_sl[so], f.slices.data(), f.slices.size() * sizeof (lh264_slice_t));
      if (!f.syn_syms.empty()) memcpy (&h_syn[yo], f.syn_syms.data(), f.syn_syms.size() * sizeof (lh264_ctx_sym_t));
      memcpy (&h_off[oo], f.syn_off.data(), (n + 1) * 4);
      lh264_ctx_job_t& cj = h_cj[j];
      cj.mbs_dev = A.d_mbs.as<lh264_mb_t>() + mo; cj.levels_dev = A.d_lev.as<int16_t>() + mo * 384; cj.slices_dev = A.d_sl.as<lh264_slice_t>() + so;
      cj.nnz_cur_dev = A.d_nnz.as<uint8_t>() + mo * 24;
      cj.nnz_past_dev = past[i] < 0 ? nullptr : past[i] < base ? ls->nnz[past_buf[i]].as<uint8_t>() : A.d_nnz.as<uint8_t>() + mb_at[past[i] - base] * 24;
      if (tolerant) h_keep[j] = keep[i] < 0 ? nullptr : keep[i] < base ? ls->nnz[1 - past_buf[i]].as<uint8_t>() : A.d_nnz.as<uint8_t>() + mb_at[keep[i] - base] * 24;
      // (the compact layout: the pool's address and size are set once the count pass has said how many symbols there are)
      cj.syms_dev = nullptr; cj.syms_cap = 0; cj.n_syms_dev = A.d_nsyms.as<uint16_t>() + mo;
      cj.sym_off_dev = A.d_symoff.as<uint32_t>() + mo; cj.sym_base_dev = A.d_symbase.as<uint64_t>() + j;
      cj.mb_w = f.mb_w; cj.mb_h = f.mb_h;
      lh264_code_job_t& kj = h_kj[j];
      kj.syn_syms_dev = A.d_syn.as<lh264_ctx_sym_t>() + yo; kj.syn_off_dev = A.d_off.as<uint32_t>() + oo;
      kj.ctx_syms_dev = nullptr; kj.ctx_n_syms_dev = cj.n_syms_dev; kj.n_mbs = (int32_t)n; kj.reserved = 0;
      kj.ctx_sym_off_dev = cj.sym_off_dev; kj.ctx_sym_base_dev = cj.sym_base_dev;
      mo += n; so += f.slices.size(); yo += f.syn_syms.size(); oo += n + 1; j++;
    }
    lh264_code_stream_t& st = h_st[c];
    st.hash_keys_dev = A.d_keys.as<uint32_t>();
    // (in a resumable call the table is the one in the carry block; a whole stream's block is key0[c]: zero-filled with the tables)
    st.hash_cells_dev = A.d_cells.as<uint32_t>() + (key0[c] + (resumable && !ls ? LH264_CARRY_TABLE_BYTES / 64 : 0)) * 16;
    st.out_dev = ls ? ls->outb.as<uint8_t>() : A.d_out.as<uint8_t>() + out0[c];
    st.out_len_dev = ls ? ls->lens.as<uint32_t>() : A.d_len.as<uint32_t>() + (size_t)c * (LH264_N_TAG_SLOTS + 1);
    st.hash_cap = hash_cap[c]; st.out_cap = out_cap[c];
    h_carry[c] = ls ? ls->carry.p : (void*) (A.d_cells.as<uint32_t>() + key0[c] * 16);
    h_flags[c] = parts[c].flags;
  });
  h_first[n_chains] = (int32_t)n_jobs;
  const double t_c = now_s();
  auto up = [] (DevBuf& d, const void* s, size_t bytes) { return bytes == 0 || hipMemcpyAsync (d.p, s, bytes, hipMemcpyHostToDevice, nullptr) == hipSuccess; };
  if (!(up (A.d_mbs, h_mbs, n_mbs * sizeof (lh264_mb_t)) && up (A.d_sparse, h_sparse, n_sparse * 8) && up (A.d_sl, h_sl, n_slices * sizeof (lh264_slice_t)) &&
        up (A.d_syn, h_syn, n_syn * sizeof (lh264_ctx_sym_t)) && up (A.d_off, h_off, n_off * 4) && up (A.d_cj, h_cj.data(), n_jobs * sizeof (lh264_ctx_job_t)) &&
        up (A.d_kj, h_kj.data(), n_jobs * sizeof (lh264_code_job_t)) && up (A.d_first, h_first.data(), (n_chains + 1) * 4) && up (A.d_st, h_st.data(), n_chains * sizeof (lh264_code_stream_t)) &&
        (!resumable || (up (A.d_carry, h_carry.data(), n_chains * sizeof (void*)) && up (A.d_flags, h_flags.data(), n_chains * 4))) &&
        (!tolerant || up (A.d_keep, h_keep.data(), n_jobs * sizeof (void*))))) {
    fail_all (out, parts, LH264_E_HIP, "upload failed"); return;
  }
  if (n_sparse) lh264host::expand_sparse (A.d_sparse.as<uint64_t>(), n_sparse, A.d_lev.as<int16_t>(), nullptr);
  if (trace_on()) hipDeviceSynchronize();
  const double t_d = now_s();
  // the symbol pool: the count pass says how many symbols the group's pictures have (8 bytes each; the fixed layout took 3,456 bytes per
  // macroblock), then the job tables get the pool's address
  unsigned long long n_syms_total = 0;
  // (tolerant: a macroblock no slice covers takes its nnz entry from the KEEP image; otherwise the calls are the ones without KEEP)
  const uint8_t* const* d_keep = tolerant ? A.d_keep.as<const uint8_t*>() : nullptr;
  int rc = n_jobs == 0 ? LH264_OK : lh264_ctx_count_chains_keep (A.d_cj.as<lh264_ctx_job_t>(), d_keep, A.d_first.as<int32_t>(), n_chains, (int)n_jobs, max_mbs, A.d_symbase.as<unsigned long long>() + n_jobs + 1, nullptr);
  if (rc == LH264_OK && n_jobs && hipMemcpy (&n_syms_total, A.d_symbase.as<unsigned long long>() + n_jobs + 1, 8, hipMemcpyDeviceToHost) != hipSuccess) rc = LH264_E_HIP;
  if (rc == LH264_OK && !A.d_syms.alloc ((size_t)n_syms_total * sizeof (lh264_ctx_sym_t))) rc = LH264_E_HIP;
  if (rc == LH264_OK) {
    for (size_t j = 0; j < n_jobs; j++) { h_cj[j].syms_dev = A.d_syms.as<lh264_ctx_sym_t>(); h_cj[j].syms_cap = n_syms_total; h_kj[j].ctx_syms_dev = A.d_syms.as<lh264_ctx_sym_t>(); }
    if (hipMemcpy (A.d_cj.p, h_cj.data(), n_jobs * sizeof (lh264_ctx_job_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy (A.d_kj.p, h_kj.data(), n_jobs * sizeof (lh264_code_job_t), hipMemcpyHostToDevice) != hipSuccess) rc = LH264_E_HIP;
  }
  if (rc == LH264_OK && n_jobs) rc = lh264_ctx_index_chains_keep (A.d_cj.as<lh264_ctx_job_t>(), d_keep, A.d_first.as<int32_t>(), n_chains, (int)n_jobs, max_mbs, nullptr);
  if (rc == LH264_OK && !resumable) rc = lh264_code_chains (A.d_kj.as<lh264_code_job_t>(), A.d_first.as<int32_t>(), A.d_st.as<lh264_code_stream_t>(), n_chains, (int)n_jobs, (long long)n_mbs, max_mbs, nullptr);
  if (rc == LH264_OK && resumable) rc = lh264_code_chains_resume (A.d_kj.as<lh264_code_job_t>(), A.d_first.as<int32_t>(), A.d_st.as<lh264_code_stream_t>(), A.d_carry.as<void*>(), A.d_flags.as<uint32_t>(),
                                                                  n_chains, (int)n_jobs, (long long)n_mbs, max_mbs, nullptr);
  if (rc != LH264_OK || hipDeviceSynchronize() != hipSuccess) { fail_all (out, parts, rc != LH264_OK ? rc : LH264_E_HIP, "kernel launch failed"); return; }
  const double t_e = now_s();
  std::vector<uint32_t> lens ((size_t)n_chains * (LH264_N_TAG_SLOTS + 1));
  std::vector<uint64_t> decisions ((size_t)n_chains * LH264_N_TAG_SLOTS);
  if (hipMemcpy (lens.data(), A.d_len.p, lens.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      lh264_code_last_decisions (0, n_chains, decisions.data()) != LH264_OK) { fail_all (out, parts, LH264_E_HIP, "download failed"); return; }
  for (int c = 0; c < n_chains; c++) if (LongStream* ls = parts[c].ls) {
    if (hipMemcpy (&lens[(size_t)c * (LH264_N_TAG_SLOTS + 1)], ls->lens.p, (LH264_N_TAG_SLOTS + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess) { fail_all (out, parts, LH264_E_HIP, "download failed"); return; }
  }
  std::vector<PackItem> items;
  std::vector<RebaseItem> rebase;
  size_t packed_bytes = 0;
  // the bytes of chain c's tags that the device has written (L: their lengths), from `bytes` (35 slots of out_cap[c]), go to the host
  auto pack_chain = [&] (int c, const uint32_t* L, const uint8_t* bytes) {
    for (int slot = 0; slot < 35; slot++) if (L[slot]) {
      PackItem it; it.src = (uint64_t) (uintptr_t) (bytes + (size_t)slot * out_cap[c]); it.dst = packed_bytes; it.len = L[slot]; it.pad = (uint32_t)c << 8 | (uint32_t)slot;
      items.push_back (it);
      packed_bytes += (L[slot] + 15u) & ~15u;
    }
  };
  for (int c = 0; c < n_chains; c++) {
    lh264_compressed_t& r = *out[idx[c]];
    const uint32_t* L = &lens[(size_t)c * (LH264_N_TAG_SLOTS + 1)];
    LongStream* ls = parts[c].ls;
    // a segment over one of the coder's counters (status 8: nothing was coded, the carry stands as it was) goes again with fewer pictures
    // (a whole stream that is over them becomes a long one: lh264_compress_batch_opts)
    if (L[LH264_N_TAG_SLOTS] == 8u && parts[c].frames.size() > 1) { parts[c].again = true; continue; }
    if (L[LH264_N_TAG_SLOTS] == 0) {
      r.segments++;
      for (int t = 0; t < LH264_N_TAG_SLOTS; t++) r.decisions[t] += decisions[(size_t)c * LH264_N_TAG_SLOTS + t];
    }
    if (ls && L[LH264_N_TAG_SLOTS] == 0) {
      // the stream's PAST policy moves on, and the images its two buffers name now are kept for the segments to come
      const long base = ls->pics_done;
      ls->cur = parts[c].cur; ls->last_fn = parts[c].last_fn; ls->slot[0] = parts[c].slot[0]; ls->slot[1] = parts[c].slot[1]; ls->pol_w = parts[c].pol_w; ls->pol_h = parts[c].pol_h;
      ls->pics_done += (long)parts[c].frames.size();
      if (!(parts[c].flags & LH264_CODE_SEG_LAST)) {
        const std::vector<size_t>& at = parts[c].mb_at;
        for (int b = 0; b < 2; b++) if (ls->slot[b] >= base) {
          const size_t q = (size_t) (ls->slot[b] - base), bytes = (size_t)parts[c].frames[q]->mb_w * parts[c].frames[q]->mb_h * 24;
          if (!ls->nnz[b].alloc (bytes) || hipMemcpy (ls->nnz[b].p, A.d_nnz.as<uint8_t>() + at[q] * 24, bytes, hipMemcpyDeviceToDevice) != hipSuccess) {
            ls->fail (LH264_E_HIP, "device allocation failed");
          }
        }
        A.long_bytes = std::max (A.long_bytes, ls->device_bytes());
        if (!ls->failed) {
          // the bytes that are final go to the host now; what is left moves to the front of the buffers (rebase_tags_kernel below)
          pack_chain (c, L, ls->outb.as<uint8_t>());
          RebaseItem rb; rb.out = ls->outb.as<uint8_t>(); rb.carry = ls->carry.as<uint32_t>(); rb.lens = ls->lens.as<uint32_t>(); rb.cap = out_cap[c]; rb.pad = 0;
          rebase.push_back (rb);
          continue;
        }
      }
    }
    if (ls && trace_on() && (parts[c].flags & LH264_CODE_SEG_LAST)) {
      // how full the stream's prior table got: the next limit a longer stream meets
      std::vector<uint64_t> tab ((size_t)ls->hash_cap * 8);
      size_t used = 0;
      if (hipMemcpy (tab.data(), ls->carry.as<uint8_t>() + LH264_CARRY_TABLE_BYTES, tab.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) for (uint64_t e : tab) used += e != 0;
      fprintf (stderr, "[lh264 compress] long stream %d: %d segments, prior table %zu of %zu entries in use (%.1f %%)\n", idx[c], r.segments, used, tab.size(), 100.0 * (double)used / (double)tab.size());
    }
    if (ls && ls->failed) continue;
    if (L[LH264_N_TAG_SLOTS] != 0) { const std::string text = "device coder status " + std::to_string (L[LH264_N_TAG_SLOTS]) + " (bits - 1: prior table full or invalid, 4: output overflow, 8: counter overflow, 16: internal hand-off; include/lh264.h)";
      if (ls) ls->fail (LH264_E_HIP, text); else { r.status = LH264_E_HIP; r.error = text; }
      continue; }
    pack_chain (c, L, ls ? ls->outb.as<uint8_t>() : A.d_out.as<uint8_t>() + out0[c]);
  }
  if (!items.empty()) {
    if (!(A.d_items.alloc (items.size() * sizeof (PackItem)) && A.d_packed.alloc (packed_bytes) && A.h_packed.alloc (packed_bytes)) ||
        hipMemcpyAsync (A.d_items.p, items.data(), items.size() * sizeof (PackItem), hipMemcpyHostToDevice, nullptr) != hipSuccess) { fail_all (out, parts, LH264_E_HIP, "download failed"); return; }
    hipLaunchKernelGGL (pack_tags_kernel, dim3 ((unsigned)items.size()), dim3 (256), 0, nullptr, A.d_items.as<PackItem>(), A.d_packed.as<uint8_t>());
    if (hipMemcpy (A.h_packed.p, A.d_packed.p, packed_bytes, hipMemcpyDeviceToHost) != hipSuccess) { fail_all (out, parts, LH264_E_HIP, "download failed"); return; }
    const uint8_t* hp = A.h_packed.as<uint8_t>();
    run_parallel ((int)items.size(), threads, [&] (int k) {
      const PackItem& it = items[k];
      lh264_compressed_t& r = *out[idx[it.pad >> 8]];
      const int slot = (int) (it.pad & 0xff), tag = slot == 34 ? 69 : slot;
      r.tag[tag].insert (r.tag[tag].end(), hp + it.dst, hp + it.dst + it.len); r.has_tag[tag] = true;      // (a long stream: segment after segment)
    });
  }
  if (!rebase.empty()) {
    bool ok2 = A.d_rebase.alloc (rebase.size() * sizeof (RebaseItem)) && hipMemcpy (A.d_rebase.p, rebase.data(), rebase.size() * sizeof (RebaseItem), hipMemcpyHostToDevice) == hipSuccess;
    if (ok2) { hipLaunchKernelGGL (rebase_tags_kernel, dim3 ((unsigned)rebase.size() * 35u), dim3 (64), 0, nullptr, A.d_rebase.as<RebaseItem>()); ok2 = hipDeviceSynchronize() == hipSuccess; }
    if (!ok2) for (Part& p : parts) if (p.ls && !(p.flags & LH264_CODE_SEG_LAST)) p.ls->fail (LH264_E_HIP, "moving a long stream's bytes failed");
  }
  if (trace_on()) fprintf (stderr, "[lh264 compress] group of %d streams, %zu MBs: alloc+clear %.3f s, staging %.3f, upload %.3f, kernels %.3f, download %.3f\n", n_chains, n_mbs,
                           t_b - t_a, t_c - t_b, t_d - t_c, t_e - t_d, now_s() - t_e);
}

lh264host::PerDevice<Arena> g_arena;      // device and page-locked buffers kept between calls; one compress call at a time per device

}  // namespace

extern "C" {

int lh264_compress_batch (const uint8_t* const* data, const size_t* len, int n, int threads, lh264_compressed_t** out) {
  return lh264_compress_batch_opts (data, len, n, threads, nullptr, out);
}
int lh264_compress_batch_opts (const uint8_t* const* data, const size_t* len, int n, int threads, const lh264_compress_opts_t* opts, lh264_compressed_t** out) {
  if (!data || !len || !out || n < 0) return LH264_E_ARG;
  if (opts && (opts->struct_bytes != sizeof (lh264_compress_opts_t) || (opts->reserved & ~ (LH264_COMPRESS_ESCAPES | LH264_COMPRESS_TOLERANT)))) return LH264_E_ARG;
  const bool escapes = opts && (opts->reserved & LH264_COMPRESS_ESCAPES);      // `reserved`: the flags word
  const bool tolerant = opts && (opts->reserved & LH264_COMPRESS_TOLERANT);
  for (int i = 0; i < n; i++) out[i] = new lh264_compressed();
  if (lh264_device_count() <= 0) { for (int i = 0; i < n; i++) { out[i]->status = LH264_E_NODEVICE; out[i]->error = "no HIP device visible"; } return LH264_E_NODEVICE; }
  if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
  if (threads < 1) threads = 1;
  int device = 0;
  hipGetDevice (&device);
  // Streams are parsed in waves on the host threads; parsed streams collect into a group until the group is worth a launch
  // (bounded by macroblock count: the symbol buffer takes 3.4 KB per macroblock); the group's staging, upload, kernels and
  // download run on their own host thread while the next wave is being parsed.
  // the device stage of a group is bound by the per-stream serial chains of the coder (about 15 ms for 100 QCIF pictures, whatever the
  // number of streams above a few hundred), its parse by the host threads (0.2 us per macroblock and thread): groups of this size keep
  // both sides busy, so that a batch of a few hundred streams already overlaps parsing with the device stage.
  // (The budget counts whole streams.  Every long stream adds its next segment - up to kSegment macroblocks - to whatever group is
  // launched: a group holds up to kBudget + long streams x kSegment macroblocks, twice the budget with one long stream and the defaults.)
  const size_t kBudget = 1300000;
  // A stream of more macroblocks than a segment holds is LONG: it is parsed a segment ahead and coded in segments of whole pictures,
  // one per group, in order (lh264_code_chains_resume), beside whatever else fills those groups.  Default: the group budget - no stream
  // that fits a group is cut.
  const size_t kSegment = opts && opts->segment_mbs ? (size_t)opts->segment_mbs : kBudget;
  // The coder's per-call limit is content, not macroblocks: fewer than 2^27 decisions in ALL tag lists of one stream together, which dense
  // HD content reaches in far fewer than 1.3 M macroblocks (77 - 350 decisions a macroblock at 1080p).  The count pass is the judge (a
  // segment over the limit comes back with status 8, nothing coded, and is sent again with half the pictures), but every such answer
  // costs a group, so segments are cut by an ESTIMATE first: 3 decisions per syntax symbol + 8 per nonzero level (BA_MW_D.264: 708 k
  // estimated, 683 k counted; the synthetic 1080p stream: 23 M per 8 pictures), held to half the limit.  LH264_COMPRESS_DECISIONS
  // overrides the budget (experiments, and the tests of the count pass's answer).
  size_t kDecisions = (size_t)1 << 26;
  if (const char* e = getenv ("LH264_COMPRESS_DECISIONS")) { const unsigned long long v = strtoull (e, nullptr, 10); if (v) kDecisions = (size_t)v; }
  auto estimate = [] (const lh264host::FrameOut& f) { return 3 * f.syn_syms.size() + 8 * f.sparse.size(); };
  const int kWave = std::max (8, 4 * threads);
  // device and page-locked buffers live across calls (allocating and releasing ~20 GB costs more than a whole batch):
  // one arena per process, one compress call at a time; lh264_compress_release() gives the memory back
  if (device < 0 || device >= lh264host::kMaxDevices) return LH264_E_ARG;
  auto arena_lock = g_arena.lock (device);
  Arena& arena = arena_lock.get();
  arena.long_bytes = 0;
  const double t_call = now_s();
  std::vector<std::unique_ptr<lh264host::Parser>> parsers (n);
  std::thread device_thread;
  std::vector<Part> running;                      // the group the device thread works on (its pictures and parsers are released when it is done)
  std::vector<std::unique_ptr<LongStream>> active;     // long streams with segments to come, in the order they were met
  double t_blocked = 0, t_serial = 0;
  // what is wrong with a stream's pictures so far (the checks of a whole stream, made piece by piece for a long one)
  auto refuse = [&] (int i, const std::vector<std::unique_ptr<lh264host::FrameOut>>& fr, std::string& why) {
    lh264host::Parser& P = *parsers[i];
    bool symbols = true;
    for (auto& f : fr) symbols = symbols && f->syn_off.size() == (size_t)f->mb_w * f->mb_h + 1 && (f->syn_off.back() == f->syn_syms.size());
    if (!P.error().empty()) why = P.error();
    else if (!symbols) why = "a picture with an incomplete slice";
    else if (!P.out_of_range().empty() && !(escapes && P.escapes_carry_all())) why = P.out_of_range() + " (the stream would not restore)";
    else if (tolerant && !P.not_carried().empty()) why = P.not_carried();
    else if (P.damaged() && !tolerant) why = "a picture with macroblocks no slice covers: the reference conceals them, which is not modelled (the stream would not restore)";
    return !why.empty();
  };
  // the pictures a long stream's parser has completed go to the stream's queue; false: the stream is refused
  auto collect = [&] (LongStream& ls) {
    lh264host::Parser& P = *parsers[ls.i];
    std::string why;
    if (refuse (ls.i, P.frames(), why)) { ls.fail (LH264_E_UNSUPPORTED, why); P.frames().clear(); return false; }
    out[ls.i]->pictures += (int)P.frames().size();
    for (auto& f : P.frames()) ls.pending.push_back (std::move (f));
    P.frames().clear();
    return true;
  };
  auto pending_mbs = [] (const LongStream& ls) { size_t m = 0; for (auto& f : ls.pending) m += (size_t)f->mb_w * f->mb_h; return m; };
  auto launch = [&] (std::vector<Part>& group) {
    // the long streams are parsed a segment ahead, beside the device stage of the group before
    if (!active.empty()) run_parallel ((int)active.size(), threads, [&] (int k) {
      LongStream& ls = *active[k];
      lh264host::Parser& P = *parsers[ls.i];
      const size_t have = pending_mbs (ls);
      if (!ls.failed && !P.file_finished() && have <= kSegment) { P.feed_file_some (kSegment - have); collect (ls); }
    });
    const double t_j = now_s();
    if (device_thread.joinable()) device_thread.join();
    t_blocked += now_s() - t_j;
    // the group that has just finished: a segment that was over one of the coder's counters goes back to the front of its stream's queue
    // (a whole stream that was over them becomes a long stream here: its parser has finished, its pictures are its queue)
    for (Part& p : running) if (p.again) {
      if (!p.ls) {
        active.emplace_back (new LongStream());
        p.ls = active.back().get();
        p.ls->i = p.i; p.ls->seg_mbs = kSegment;
      }
      p.ls->max_pics = std::max<size_t> (1, p.frames.size() / 2);
      for (size_t q = p.frames.size(); q-- > 0; ) p.ls->pending.push_front (std::move (p.frames[q]));
      p.ls->ended = false;
    }
    for (Part& p : running) p.frames.clear();       // the pictures go back to the pool while the next wave is parsed
    for (Part& p : running) if (!p.ls) parsers[p.i].reset();
    running.clear();
    // a long stream that failed - in the device stage or in its parser -: the error is its result, the bytes of its earlier segments are dropped
    for (auto& lsp : active) if (lsp->failed) {
      lh264_compressed_t& r = *out[lsp->i];
      r.status = lsp->fail_code; r.error = lsp->fail_text;
      for (int t = 0; t < 72; t++) { r.tag[t].clear(); r.tag[t].shrink_to_fit(); r.has_tag[t] = false; }
      lsp->pending.clear();
    }
    // the next segment of every long stream
    for (auto& lsp : active) {
      LongStream& ls = *lsp;
      if (ls.failed || ls.ended) continue;
      lh264host::Parser& P = *parsers[ls.i];
      Part part; part.i = ls.i; part.ls = &ls;
      size_t m = 0, e = 0;
      while (!ls.pending.empty() && part.frames.size() < ls.max_pics) {
        const size_t fm = (size_t)ls.pending.front()->mb_w * ls.pending.front()->mb_h, fe = estimate (*ls.pending.front());
        if (!part.frames.empty() && (m + fm > kSegment || e + fe > kDecisions)) break;
        m += fm; e += fe; part.frames.push_back (std::move (ls.pending.front())); ls.pending.pop_front();
      }
      const bool last = P.file_finished() && ls.pending.empty();
      part.flags = (ls.pics_done == 0 ? LH264_CODE_SEG_FIRST : 0u) | (last ? LH264_CODE_SEG_LAST : 0u);
      if (last) {
        lh264_compressed_t& r = *out[ls.i];
        r.main_stream = P.main_stream();
        if (!P.pcm_samples().empty()) { r.tag[LH264_TAG_PCM] = P.pcm_samples(); r.has_tag[LH264_TAG_PCM] = true; }
        if (escapes && !P.out_of_range().empty()) { r.tag[LH264_TAG_ESC] = P.escapes(); r.has_tag[LH264_TAG_ESC] = true; }
        ls.ended = true;
      }
      group.push_back (std::move (part));
    }
    // streams that are through (their last segment is in no group any more) or refused give their memory back
    for (size_t k = 0; k < active.size(); ) {
      LongStream& ls = *active[k];
      bool in_group = false;
      for (Part& p : group) in_group = in_group || p.ls == &ls;
      if (!in_group) { const int i = ls.i; active.erase (active.begin() + (long)k); parsers[i].reset(); } else k++;      // (the pictures before the parser: its arena holds the first ones)
    }
    running.swap (group); group.clear();
    if (running.empty()) return;
    device_thread = std::thread ([&, device] () {
      hipSetDevice (device);
      if (!getenv ("LH264_COMPRESS_PARSE_ONLY"))          // diagnostic: the host side alone
        compress_group (arena, running, len, out, std::max (1, threads / 2), tolerant);
    });
  };
  std::vector<Part> group;
  size_t in_group = 0;
  for (int w0 = 0; w0 < n; w0 += kWave) {
    const int w1 = std::min (n, w0 + kWave);
    const double t_p = now_s();
    run_parallel (w1 - w0, threads, [&] (int k) {
      const int i = w0 + k;
      parsers[i].reset (new lh264host::Parser());
      parsers[i]->set_want_coeffs (false);
      parsers[i]->set_sparse_levels (true);
      parsers[i]->set_stream_arena (true);
      parsers[i]->set_tolerant (tolerant);
      parsers[i]->begin_file (data[i], data[i] ? len[i] : 0);
      parsers[i]->feed_file_some (kSegment);            // (a stream of up to kSegment macroblocks is parsed whole)
    });
    if (trace_on()) fprintf (stderr, "[lh264 compress] wave of %d streams parsed in %.3f s\n", w1 - w0, now_s() - t_p);
    const double t_s = now_s();
    for (int i = w0; i < w1; i++) {
      lh264_compressed_t& r = *out[i];
      lh264host::Parser& P = *parsers[i];
      size_t est = 0;
      for (auto& f : P.frames()) est += estimate (*f);
      if (!P.file_finished() || P.held_mbs() > kSegment || (est > kDecisions && P.frames().size() > 1)) {
        // a long stream: its pictures so far wait in its queue, later ones come from the per-thread cache and go back there segment by segment
        std::unique_ptr<LongStream> ls (new LongStream());
        ls->i = i; ls->seg_mbs = kSegment;
        P.pause_stream_arena();
        if (collect (*ls)) active.push_back (std::move (ls));
        else { r.status = ls->fail_code; r.error = ls->fail_text; ls.reset(); parsers[i].reset(); }
        continue;
      }
      r.main_stream = P.main_stream();
      r.pictures = (int)P.frames().size();
      const size_t mbs = P.held_mbs();
      std::string why;
      if (refuse (i, P.frames(), why)) { r.status = LH264_E_UNSUPPORTED; r.error = why; }
      else {                                            // the streams of the container the coder does not write
        if (!P.pcm_samples().empty()) { r.tag[LH264_TAG_PCM] = P.pcm_samples(); r.has_tag[LH264_TAG_PCM] = true; }
        if (escapes && !P.out_of_range().empty()) { r.tag[LH264_TAG_ESC] = P.escapes(); r.has_tag[LH264_TAG_ESC] = true; }
      }
      if (r.status != LH264_OK || mbs == 0) { parsers[i].reset(); continue; }
      if (in_group && in_group + mbs > kBudget) { launch (group); in_group = 0; }
      Part part; part.i = i; part.frames = std::move (P.frames());
      group.push_back (std::move (part)); in_group += mbs;
    }
    t_serial += now_s() - t_s;
  }
  launch (group);
  while (!active.empty() || !running.empty()) launch (group);      // the long streams' remaining segments, a group each
  if (device_thread.joinable()) device_thread.join();
  if (trace_on()) fprintf (stderr, "[lh264 compress] %d streams: %.3f s (between waves %.3f s, of which waiting for the device stage %.3f s)\n", n, now_s() - t_call, t_serial, t_blocked);
  return LH264_OK;
}
int lh264_compress_arena_bytes (size_t* device, size_t* pinned) {
  const bool ok = lh264_device_count() > 0 && g_arena.read_current ([&] (const Arena* a) {
    if (device) *device = a ? a->device_bytes() + a->long_bytes : 0;
    if (pinned) *pinned = a ? a->pinned_bytes() : 0;
  });
  return ok ? LH264_OK : LH264_E_NODEVICE;
}
void lh264_compress_release (void) { g_arena.release_all(); }

// the same batch over several devices of the node: the streams are cut into contiguous shares of about equal input size, one
// host thread per share drives lh264_compress_batch on its device (streams are independent: no exchange between devices)
int lh264_compress_batch_devices (const uint8_t* const* data, const size_t* len, int n, int threads, const int* devices, int n_devices,
                                  lh264_compressed_t** out) {
  return lh264_compress_batch_devices_opts (data, len, n, threads, devices, n_devices, nullptr, out);
}
int lh264_compress_batch_devices_opts (const uint8_t* const* data, const size_t* len, int n, int threads, const int* devices, int n_devices,
                                       const lh264_compress_opts_t* opts, lh264_compressed_t** out) {
  if (opts && (opts->struct_bytes != sizeof (lh264_compress_opts_t) || (opts->reserved & ~ (LH264_COMPRESS_ESCAPES | LH264_COMPRESS_TOLERANT)))) return LH264_E_ARG;
  if (!data || !len || !out || n < 0 || !devices || n_devices < 1) return LH264_E_ARG;
  if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
  size_t total = 0;
  for (int i = 0; i < n; i++) total += len[i];
  std::vector<int> first (n_devices + 1, n);
  first[0] = 0;
  {
    size_t acc = 0; int s = 1;
    for (int i = 0; i < n && s < n_devices; i++) {
      acc += len[i];
      while (s < n_devices && acc * n_devices >= total * s) first[s++] = i + 1;
    }
  }
  std::vector<int> rcs (n_devices, LH264_OK);
  std::vector<std::thread> th;
  for (int s = 0; s < n_devices; s++) {
    th.emplace_back ([&, s] () {
      const int a = first[s], b = first[s + 1];
      if (hipSetDevice (devices[s]) != hipSuccess) { for (int i = a; i < b; i++) { out[i] = new lh264_compressed(); out[i]->status = LH264_E_HIP; out[i]->error = "hipSetDevice failed"; } rcs[s] = LH264_E_HIP; return; }
      rcs[s] = lh264_compress_batch_opts (data + a, len + a, b - a, std::max (1, threads / n_devices), opts, out + a);
    });
  }
  for (auto& t : th) t.join();
  for (int rc : rcs) if (rc != LH264_OK) return rc;
  return LH264_OK;
}
int lh264_compressed_status (const lh264_compressed_t* c) { return c ? c->status : LH264_E_ARG; }
const char* lh264_compressed_error (const lh264_compressed_t* c) { return c ? c->error.c_str() : ""; }
const uint8_t* lh264_compressed_main (const lh264_compressed_t* c, size_t* len) {
  if (!c) return nullptr;
  if (len) *len = c->main_stream.size();
  return c->main_stream.empty() ? (const uint8_t*)"" : c->main_stream.data();
}
const uint8_t* lh264_compressed_tag (const lh264_compressed_t* c, int tag, size_t* len) {
  if (!c || tag < 0 || tag >= 72 || !c->has_tag[tag]) { if (len) *len = 0; return nullptr; }
  if (len) *len = c->tag[tag].size();
  return c->tag[tag].data();
}
int lh264_compressed_pictures (const lh264_compressed_t* c) { return c ? c->pictures : 0; }
int lh264_compressed_segments (const lh264_compressed_t* c) { return c ? c->segments : 0; }
uint64_t lh264_compressed_decisions (const lh264_compressed_t* c, int tag) {
  const int slot = tag == 69 ? 34 : tag;
  return c && tag >= 0 && slot < 35 && (tag < 34 || tag == 69) ? c->decisions[slot] : 0;
}
void lh264_compressed_free (lh264_compressed_t* c) { delete c; }

}
