// lh264_slice.h - the CAVLC macroblock layer of one slice (7.3.4, 7.3.5, 9.2), host and device from one source: what
// host/h264_parser.cpp does in parse_slice_data_cavlc / parse_mb_cavlc / residual_block and their helpers, in the same decision
// order, without the recompressor's bookkeeping (MbSyn, levels, I_PCM sample stream).  A slice's macroblock layer depends on its own
// header, its parameter sets and its own earlier macroblocks only ("macroblock kk is available to k" is first_mb <= kk < k), so the
// slices of a batch are independent jobs: slice_parse_kernel (lh264_slice.hip) walks one per wave, lh264_debug_slice_parse steps the
// same code over host memory.  Every bound is the task's: the bit reader never leaves [rbsp, rbsp + rbsp_bytes), no macroblock
// outside [first_mb, limit_mb) is written, no coefficient index reaches 384.
//
// The tables are the host's (host/h264_vlc_tables.h, host/h264_tables.h): fill_tables() gathers them into one record that the walk
// reads through a pointer - the host's own copy, or the copy a wave made of the uploaded record in LDS.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/lh264.h"
#include "host/h264_tables.h"
#include "host/h264_vlc_tables.h"
#include "host/capi_internal.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define LH264S_HD __host__ __device__
#else
#define LH264S_HD
#endif

namespace lh264host {
static const uint8_t kChromaNzcIdx[2][4] = {{16, 17, 20, 21}, {18, 19, 22, 23}};   // reference nzc layout (common_tables.cpp:39-47)
}

namespace lh264slice {

using lh264host::SliceResult;
using lh264host::SliceTask;
using lh264host::VlcSym;
using lh264host::VlcTok;

struct alignas (16) Tables {
  VlcTok coeff_token[5][62];
  VlcSym total_zeros[16][16], total_zeros_cdc[4][4], run_before[8][15];
  uint8_t coeff_token_count[5], total_zeros_count[16], total_zeros_cdc_count[4], run_before_count[8];
  uint8_t zigzag4[16], zigzag8[64], cbp_intra[48], cbp_inter[48], chroma_qp[52], norm4[6][3], norm8[6][6], chroma_nzc_idx[2][4];
};
static_assert (sizeof (Tables) % 16 == 0 && sizeof (Tables) < 8192, "the table record is copied into LDS 16 bytes at a time");

#define LH264S_TAKE(dst, src) static_assert (sizeof (dst) == sizeof (src), #src); memcpy (dst, src, sizeof (dst))
inline void fill_tables (Tables& t) {
  using namespace lh264host;
  memset (&t, 0, sizeof (t));
  LH264S_TAKE (t.coeff_token, kCoeffToken); LH264S_TAKE (t.total_zeros, kTotalZeros); LH264S_TAKE (t.total_zeros_cdc, kTotalZerosChromaDc);
  LH264S_TAKE (t.run_before, kRunBefore); LH264S_TAKE (t.coeff_token_count, kCoeffTokenCount); LH264S_TAKE (t.total_zeros_count, kTotalZerosCount);
  LH264S_TAKE (t.total_zeros_cdc_count, kTotalZerosChromaDcCount); LH264S_TAKE (t.run_before_count, kRunBeforeCount);
  LH264S_TAKE (t.zigzag4, kZigzag4x4); LH264S_TAKE (t.zigzag8, kZigzag8x8); LH264S_TAKE (t.cbp_intra, kCbpIntra); LH264S_TAKE (t.cbp_inter, kCbpInter);
  LH264S_TAKE (t.chroma_qp, kChromaQp); LH264S_TAKE (t.norm4, kNormAdjust4x4); LH264S_TAKE (t.norm8, kNormAdjust8x8); LH264S_TAKE (t.chroma_nzc_idx, kChromaNzcIdx);
}
#undef LH264S_TAKE

enum { kLdsLineMbs = 256 };      // pictures up to this many macroblocks wide keep the line of intra modes in LDS; wider ones use SliceTask::line

// ---- the bit reader: lh264host::BitReader bounded by the task ---------------------------------------------------------------------------
struct Bits {
  const uint8_t* p; uint32_t nbytes, nbits, pos; int64_t last_one; bool err;
  uint64_t win; uint32_t wbyte; bool whave;      // the 8 bytes at byte wbyte, big-endian: a peek within its first 4 bytes needs no load
  LH264S_HD void init (const uint8_t* d, uint32_t bytes, uint32_t at) {
    p = d; nbytes = bytes; nbits = bytes * 8; pos = at; err = false; win = 0; wbyte = 0; whave = false;
    // more_rbsp_data asks for the last set bit of the payload (the rbsp stop bit): it does not move while the slice is read
    last_one = -1;
    for (uint32_t b = bytes; b-- > 0; ) if (p[b]) { last_one = (int64_t)b * 8 + 7 - __builtin_ctz ((uint32_t)p[b]); break; }
  }
  LH264S_HD uint64_t load8 (uint32_t b) const {
    uint64_t v = 0;
    if (b < nbytes && nbytes - b >= 8) { for (int i = 0; i < 8; i++) v = (v << 8) | p[b + i]; }
    else { for (uint32_t i = 0; i < 8; i++) v = (v << 8) | (b < nbytes && i < nbytes - b ? p[b + i] : 0); }
    return v;
  }
  // the next n <= 32 bits, zero-extended past the end
  LH264S_HD uint32_t peek (int n) {
    const uint32_t b = pos >> 3;
    if (!whave || b < wbyte || b - wbyte > 3) { win = load8 (b); wbyte = b; whave = true; }
    return n ? (uint32_t) ((win << (pos - wbyte * 8)) >> (64 - n)) : 0;
  }
  LH264S_HD void skip (int n) { pos += (uint32_t)n; if (pos > nbits) err = true; }
  LH264S_HD uint32_t u1() { if (pos >= nbits) { err = true; return 0; } const uint32_t b = peek (1); pos++; return b; }
  LH264S_HD uint32_t u (int n) {             // n <= 32
    if (pos > nbits || (uint32_t)n > nbits - pos) { err = true; pos = nbits; return 0; }
    const uint32_t v = peek (n); pos += (uint32_t)n; return v;
  }
  LH264S_HD uint32_t ue() {
    const uint32_t w = peek (32);
    if (w >> 16) {
      const int z = __builtin_clz (w), len = 2 * z + 1;
      if (pos > nbits || (uint32_t)len > nbits - pos) { err = true; pos = nbits; return 0; }
      pos += (uint32_t)len;
      return (w >> (32 - len)) - 1;
    }
    int z = 0;
    while (!u1()) { if (err || ++z > 31) { err = true; return 0; } }
    return z == 0 ? 0 : ((1u << z) - 1 + u (z));
  }
  LH264S_HD int32_t se() { const uint32_t k = ue(); return (k & 1) ? (int32_t) ((k + 1) >> 1) : - (int32_t) (k >> 1); }
  LH264S_HD bool byte_aligned() const { return (pos & 7) == 0; }
  LH264S_HD bool more_rbsp_data() const { return pos < nbits && last_one > (int64_t)pos; }
};

LH264S_HD inline int imin (int a, int b) { return a < b ? a : b; }
LH264S_HD inline int imax (int a, int b) { return a > b ? a : b; }
LH264S_HD inline int z2x (int z) { return (z & 1) | ((z >> 2) & 1) << 1; }
LH264S_HD inline int z2y (int z) { return ((z >> 1) & 1) | ((z >> 3) & 1) << 1; }
LH264S_HD inline int xy2z (int x, int y) { return (x & 1) | ((y & 1) << 1) | ((x >> 1) << 2) | ((y >> 1) << 3); }

// ---- one residual block (9.2): total_coeff, levels at their scan positions; -1 on error ----------------------------------------------
LH264S_HD inline int residual_block (const Tables& T, Bits& br, int nC, int max_coeff, int* level /*[16]*/) {
  const int tab = nC < 0 ? 4 : nC < 2 ? 0 : nC < 4 ? 1 : nC < 8 ? 2 : 3;
  int total = -1, t1 = 0;
  if (tab == 3) {
    const uint32_t v = br.u (6);
    if (v == 3) { total = 0; t1 = 0; } else { total = (int) (v >> 2) + 1; t1 = (int) (v & 3); }
  } else {
    const uint32_t bits = br.peek (16);
    for (int i = 0; i < T.coeff_token_count[tab]; i++) {
      const VlcTok& t = T.coeff_token[tab][i];
      if (t.len && (bits >> (16 - t.len)) == t.code) { total = t.total_coeff; t1 = t.trailing_ones; br.skip (t.len); break; }
    }
  }
  for (int i = 0; i < 16; i++) level[i] = 0;
  if (total < 0 || br.err) return -1;
  if (total == 0) return 0;
  if (total > max_coeff) return -1;
  int lv[16];
  int suffix_len = (total > 10 && t1 < 3) ? 1 : 0;
  for (int i = 0; i < total; i++) {
    if (i < t1) { lv[i] = br.u1() ? -1 : 1; continue; }
    int prefix = 0;
    {
      const uint32_t w = br.peek (32);
      if (w) { prefix = __builtin_clz (w); br.skip (prefix + 1); if (br.err) return -1; }
      else { while (!br.u1()) { if (br.err || ++prefix > 32) return -1; } }
    }
    int code = imin (15, prefix) << suffix_len;
    const int ssize = (prefix == 14 && suffix_len == 0) ? 4 : (prefix >= 15 ? prefix - 3 : suffix_len);
    if (ssize > 0) code += (int)br.u (ssize);
    if (prefix >= 15 && suffix_len == 0) code += 15;
    if (prefix >= 16) code += (int) ((1u << (prefix - 3)) - 4096u);
    if (i == t1 && t1 < 3) code += 2;
    lv[i] = (code & 1) ? (-code - 1) >> 1 : (code + 2) >> 1;
    if (suffix_len == 0) suffix_len = 1;
    const int a = lv[i] < 0 ? -lv[i] : lv[i];
    if (a > (3 << (suffix_len - 1)) && suffix_len < 6) suffix_len++;
  }
  int zeros_left = 0;
  if (total < max_coeff) {
    const uint32_t bits = br.peek (9);
    bool ok = false;
    if (nC < 0) {
      for (int i = 0; i < T.total_zeros_cdc_count[total]; i++) {
        const VlcSym& s = T.total_zeros_cdc[total][i];
        if ((bits >> (9 - s.len)) == s.code) { zeros_left = s.sym; br.skip (s.len); ok = true; break; }
      }
    } else {
      for (int i = 0; i < T.total_zeros_count[total]; i++) {
        const VlcSym& s = T.total_zeros[total][i];
        if ((bits >> (9 - s.len)) == s.code) { zeros_left = s.sym; br.skip (s.len); ok = true; break; }
      }
    }
    if (!ok) return -1;
  }
  if (zeros_left + total > max_coeff) return -1;
  int pos = zeros_left + total - 1;
  for (int i = 0; i < total; i++) {
    int run = 0;
    if (i < total - 1 && zeros_left > 0) {
      const int zl = imin (zeros_left, 7);
      const uint32_t bits = br.peek (11);
      bool ok = false;
      for (int k = 0; k < T.run_before_count[zl]; k++) {
        const VlcSym& s = T.run_before[zl][k];
        if ((bits >> (11 - s.len)) == s.code) { run = s.sym; br.skip (s.len); ok = true; break; }
      }
      if (!ok || run > zeros_left) return -1;
    } else if (i == total - 1) run = zeros_left;
    if (pos < 0 || pos > 15) return -1;       // (cannot happen: zeros_left + total <= max_coeff <= 16 and the runs sum to at most zeros_left)
    level[pos] = lv[i];
    pos -= run + 1;
    zeros_left -= run;
  }
  return br.err ? -1 : total;
}

// ---- the walk over one slice --------------------------------------------------------------------------------------------------------
// What the walk of either entropy mode does with a macroblock once its syntax elements are known: availability, dequantisation, motion
// vector prediction, the final intra modes, the record's way out.  The walk D (Walk here, CabacWalk in lh264_slice_cabac.h) holds the
// data - T (its table record, with chroma_qp, norm4 and norm8 under these names), t, m, w, first, k - and derives from WalkOps<D>: one
// definition for both, and neither walk's layout depends on the other's.
template <typename D> struct WalkOps {
  LH264S_HD D& self() { return *static_cast<D*> (this); }
  LH264S_HD const D& self() const { return *static_cast<const D*> (this); }
  LH264S_HD bool avail (int kk) const { const D& S = self(); return kk >= S.first && kk < S.k; }
  LH264S_HD bool intra_nb_avail (int kk) const { const D& S = self(); return avail (kk) && (!S.t->constrained_intra_pred || (S.t->mbs[kk].mb_type & LH264_MB_INTRA)); }
  // dequantisation as the host front end does it (flat, or with the PPS's resolved lists: 6 x 16 then 2 x 64 entries, raster)
  LH264S_HD int dq4 (int list, int qp, int j, int level) const {
    const D& S = self();
    const int x = j & 3, y = j >> 2;
    const int cls = ((x & 1) == 0 && (y & 1) == 0) ? 0 : ((x & 1) && (y & 1)) ? 1 : 2;
    const int d = S.T->norm4[qp % 6][cls] << (qp / 6);
    return S.t->use_sl ? (level * (S.t->scaling[list * 16 + j] * d)) >> 4 : level * d;
  }
  LH264S_HD static int cls8 (int x, int y) {
    if ((x & 3) == 0 && (y & 3) == 0) return 0;
    if ((x & 1) && (y & 1)) return 1;
    if ((x & 3) == 2 && (y & 3) == 2) return 2;
    if (((x & 3) == 0 && (y & 1)) || ((x & 1) && (y & 3) == 0)) return 3;
    if (((x & 3) == 0 && (y & 3) == 2) || ((x & 3) == 2 && (y & 3) == 0)) return 4;
    return 5;
  }
  LH264S_HD int dq8 (int list8, int qp, int j, int level) const {
    const D& S = self();
    const int d = (S.t->use_sl ? S.t->scaling[96 + list8 * 64 + j] : 16) * S.T->norm8[qp % 6][cls8 (j & 7, j >> 3)];
    return qp >= 36 ? (level * d) * (1 << (qp / 6 - 6)) : (level * d + (1 << (5 - qp / 6))) >> (6 - qp / 6);
  }
  LH264S_HD void set_qp (int qp) {
    D& S = self();
    S.m->qp_y = (uint8_t)qp;
    for (int p = 0; p < 2; p++) S.m->qp_c[p] = S.T->chroma_qp[imin (51, imax (0, qp + S.t->chroma_qp_offset[p]))];
  }
  LH264S_HD void put (int16_t* coef, int at, int v) const { if ((unsigned)at < 384u) coef[at] = (int16_t)v; }

  // median motion vector prediction (8.4.1.3); motion and references of other macroblocks come from their records
  struct Nb { bool avail; int ref, mvx, mvy; };
  LH264S_HD Nb nb_block (int bx, int by, uint32_t filled) const {
    const D& S = self();
    int kk = S.k, x = bx, y = by;
    if (x < 0) { kk = (kk % S.w) ? kk - 1 : -1; x += 4; } else if (x > 3) { kk = ((kk % S.w) + 1 < S.w) ? kk + 1 : -1; x -= 4; }
    if (kk >= 0 && y < 0) { kk = kk >= S.w ? kk - S.w : -1; y += 4; }
    Nb r = {false, -1, 0, 0};
    if (kk < 0) return r;
    if (kk == S.k) {
      if (bx < 0 || bx > 3 || by < 0) return r;
      if (!((filled >> (y * 4 + x)) & 1)) return r;
    } else if (!avail (kk)) return r;
    r.avail = true;
    const lh264_mb_t* s = kk == S.k ? S.m : &S.t->mbs[kk];
    r.ref = s->ref_idx[(y >> 1) * 2 + (x >> 1)];
    r.mvx = s->mv[y * 4 + x][0]; r.mvy = s->mv[y * 4 + x][1];
    return r;
  }
  LH264S_HD static int median3 (int a, int b, int c) { return imax (imin (a, b), imin (imax (a, b), c)); }
  LH264S_HD void predict_mv (uint32_t filled, int bx, int by, int bw, int ref, int shape, int& px, int& py) const {
    Nb A = nb_block (bx - 1, by, filled), B = nb_block (bx, by - 1, filled), C = nb_block (bx + bw, by - 1, filled);
    if (!C.avail) C = nb_block (bx - 1, by - 1, filled);
    if (shape == 1 && B.avail && B.ref == ref) { px = B.mvx; py = B.mvy; return; }
    if (shape == 2 && A.avail && A.ref == ref) { px = A.mvx; py = A.mvy; return; }
    if (shape == 3 && A.avail && A.ref == ref) { px = A.mvx; py = A.mvy; return; }
    if (shape == 4 && C.avail && C.ref == ref) { px = C.mvx; py = C.mvy; return; }
    if (!B.avail && !C.avail && A.avail) { px = A.mvx; py = A.mvy; return; }
    const int cnt = (A.avail && A.ref == ref) + (B.avail && B.ref == ref) + (C.avail && C.ref == ref);
    if (cnt == 1) {
      if (A.avail && A.ref == ref) { px = A.mvx; py = A.mvy; }
      else if (B.avail && B.ref == ref) { px = B.mvx; py = B.mvy; }
      else { px = C.mvx; py = C.mvy; }
      return;
    }
    px = median3 (A.avail ? A.mvx : 0, B.avail ? B.mvx : 0, C.avail ? C.mvx : 0);
    py = median3 (A.avail ? A.mvy : 0, B.avail ? B.mvy : 0, C.avail ? C.mvy : 0);
  }
  LH264S_HD void fill_part (int bx, int by, int bw, int bh, int mvx, int mvy, uint32_t& filled) {
    D& S = self();
    for (int y = by; y < by + bh; y++) for (int x = bx; x < bx + bw; x++) {
        S.m->mv[y * 4 + x][0] = (int16_t)mvx; S.m->mv[y * 4 + x][1] = (int16_t)mvy;
        filled |= 1u << (y * 4 + x);
      }
  }

  // parsed (standard-numbered) intra modes -> the availability-resolved final modes of the record
  LH264S_HD static int dcmap (bool l, bool t_, int dc, int dcl, int dct, int dc128) { return l && t_ ? dc : l ? dcl : t_ ? dct : dc128; }
  LH264S_HD void finalize_intra_modes (const int* raw, bool is8, int i16mode, int chroma_mode) {
    D& S = self();
    const bool L = (S.k % S.w) && intra_nb_avail (S.k - 1);
    const bool Tp = S.k >= S.w && intra_nb_avail (S.k - S.w);
    const bool TL = (S.k % S.w) && S.k >= S.w && intra_nb_avail (S.k - S.w - 1);
    const bool TR = S.k >= S.w && ((S.k % S.w) + 1 < S.w) && intra_nb_avail (S.k - S.w + 1);
    S.m->intra_avail = (uint8_t) ((Tp ? LH264_AVAIL_T : 0) | (TL ? LH264_AVAIL_TL : 0) | (L ? LH264_AVAIL_L : 0) | (TR ? LH264_AVAIL_TR : 0));
    if (raw) {
      if (!is8) {
        for (int z = 0; z < 16; z++) {
          const int bx = z2x (z), by = z2y (z);
          const bool l = bx > 0 || L, tt = by > 0 || Tp;
          bool tr;
          if (by == 0) tr = bx < 3 ? Tp : TR;
          else tr = bx < 3 && xy2z (bx + 1, by - 1) < z;
          int mode = raw[by * 4 + bx];
          if (mode == 2) mode = dcmap (l, tt, LH264_I4_DC, LH264_I4_DC_L, LH264_I4_DC_T, LH264_I4_DC_128);
          else if (mode == 3 && !tr) mode = LH264_I4_DDL_TOP;
          else if (mode == 7 && !tr) mode = LH264_I4_VL_TOP;
          S.m->intra_mode[by * 4 + bx] = (int8_t)mode;
        }
      } else {
        for (int i8 = 0; i8 < 4; i8++) {
          const int bx = i8 & 1, by = i8 >> 1;
          const bool l = bx > 0 || L, tt = by > 0 || Tp;
          const bool tr = i8 == 0 ? Tp : i8 == 1 ? TR : i8 == 2;
          int mode = raw[by * 8 + bx * 2];
          if (mode == 2) mode = dcmap (l, tt, LH264_I4_DC, LH264_I4_DC_L, LH264_I4_DC_T, LH264_I4_DC_128);
          else if (mode == 3 && !tr) mode = LH264_I4_DDL_TOP;
          else if (mode == 7 && !tr) mode = LH264_I4_VL_TOP;
          for (int j = 0; j < 4; j++) S.m->intra_mode[(by * 2 + (j >> 1)) * 4 + bx * 2 + (j & 1)] = (int8_t)mode;
        }
      }
    } else if (i16mode >= 0) {
      int mode = i16mode;
      if (mode == 2) mode = dcmap (L, Tp, LH264_I16_DC, LH264_I16_DC_L, LH264_I16_DC_T, LH264_I16_DC_128);
      S.m->intra_mode[0] = (int8_t)mode;
    }
    if (chroma_mode >= 0) {
      int mode = chroma_mode;
      if (mode == 0) mode = dcmap (L, Tp, LH264_C_DC, LH264_C_DC_L, LH264_C_DC_T, LH264_C_DC_128);
      S.m->chroma_mode = (int8_t)mode;
    }
  }

  // the macroblock in hand is done: its record goes where recon_chain_kernel reads it (16 bytes at a time; both sides are 16-byte
  // aligned)
  LH264S_HD void store_record() {
    D& S = self();
    const uint4_like* s = (const uint4_like*)S.m; uint4_like* d = (uint4_like*)&S.t->mbs[S.k];
    for (int i = 0; i < 8; i++) d[i] = s[i];
  }
  struct alignas (16) uint4_like { uint32_t x, y, z, w; };
};

struct Walk : WalkOps<Walk> {
  const Tables* T; const SliceTask* t; Bits br;
  lh264_mb_t* m;            // the record in hand (the caller's scratch: LDS on the device); copied to t->mbs[k] when the macroblock is done
  int8_t* line;             // raw intra modes of the bottom row of the macroblock parsed last in every column, 4 per column
  int8_t left[4];           // ... and of the right column of macroblock k - 1
  int8_t ipm[16];           // ... of the macroblock in hand, raster (2 where it is not I_NxN)
  int w, n, first, k;

  LH264S_HD int nz_luma (int bx, int by, bool& a) const {
    int kk = k;
    if (bx < 0) { kk = (k % w) ? k - 1 : -1; bx = 3; }
    if (by < 0) { kk = k >= w ? k - w : -1; by = 3; }
    a = kk == k || avail (kk);
    if (!a) return 0;
    return kk == k ? m->nzc[by * 4 + bx] : t->mbs[kk].nzc[by * 4 + bx];
  }
  LH264S_HD int nz_chroma (int c, int bx, int by, bool& a) const {
    int kk = k;
    if (bx < 0) { kk = (k % w) ? k - 1 : -1; bx = 1; }
    if (by < 0) { kk = k >= w ? k - w : -1; by = 1; }
    a = kk == k || avail (kk);
    if (!a) return 0;
    const int at = T->chroma_nzc_idx[c][by * 2 + bx];
    return kk == k ? m->nzc[at] : t->mbs[kk].nzc[at];
  }
  LH264S_HD static int nC_of (int nA, bool aA, int nB, bool aB) {
    if (aA && aB) return (nA + nB + 1) >> 1;
    if (aA) return nA;
    if (aB) return nB;
    return 0;
  }
  LH264S_HD int luma_nC (int bx, int by) const { bool aA, aB; const int nA = nz_luma (bx - 1, by, aA), nB = nz_luma (bx, by - 1, aB); return nC_of (nA, aA, nB, aB); }

  // ... and its intra modes become the neighbours' context
  LH264S_HD void done() {
    store_record();
    for (int i = 0; i < 4; i++) { line[(k % w) * 4 + i] = ipm[12 + i]; left[i] = ipm[i * 4 + 3]; }
  }

  // one macroblock (7.3.5); false where the host's parse_mb_cavlc returns false
  LH264S_HD bool parse_mb (int& qp_prev, bool is_skip) {
    memset (m, 0, sizeof (*m));
    m->slice_id = (uint16_t)t->slice_index;
    for (int i = 0; i < 16; i++) ipm[i] = 2;
    for (int i = 0; i < 4; i++) m->ref_idx[i] = -1;
    int16_t* coef = t->coeffs + (size_t)k * 384;
    if (is_skip) {                                        // P_Skip: inferred motion (8.4.1.1)
      m->mb_type = LH264_MB_SKIP;
      for (int i = 0; i < 4; i++) m->ref_idx[i] = 0;
      const Nb A = nb_block (-1, 0, 0), B = nb_block (0, -1, 0);
      int px = 0, py = 0;
      if (A.avail && B.avail && !(A.ref == 0 && A.mvx == 0 && A.mvy == 0) && !(B.ref == 0 && B.mvx == 0 && B.mvy == 0))
        predict_mv (0, 0, 0, 4, 0, 0, px, py);
      uint32_t filled = 0;
      fill_part (0, 0, 4, 4, px, py, filled);
      set_qp (qp_prev);
      return true;
    }
    uint32_t mbt = br.ue();
    bool intra = true;
    if (t->slice_type == 0) { if (mbt < 5) intra = false; else mbt -= 5; }
    if (br.err) return false;
    int cbp = 0;
    bool t8 = false;
    int raw_modes[16]; bool have_raw = false; int i16mode = -1, chroma_mode = -1;
    if (intra) {
      if (mbt > 25) return false;
      if (mbt == 25) {                                    // I_PCM
        m->mb_type = LH264_MB_IPCM;
        while (!br.byte_aligned()) br.u1();
        for (int i = 0; i < 384; i++) coef[i] = (int16_t)br.u (8);
        m->flags |= LH264_MBF_PCM_IN_COEFF;
        memset (m->nzc, 16, 24);
        m->qp_y = 0; m->qp_c[0] = m->qp_c[1] = 0;
        finalize_intra_modes (nullptr, false, -1, -1);
        return !br.err;
      }
      if (mbt == 0) {                                     // I_NxN
        if (t->transform_8x8) t8 = br.u1() != 0;
        m->mb_type = t8 ? LH264_MB_I8x8 : LH264_MB_I4x4;
        const int nblk = t8 ? 4 : 16;
        for (int i = 0; i < nblk; i++) {
          const int bx = t8 ? (i & 1) * 2 : z2x (i), by = t8 ? (i >> 1) * 2 : z2y (i);
          int modeA = 2, modeB = 2; bool dcpred = false;
          if (bx > 0) modeA = ipm[by * 4 + bx - 1];
          else if (!((k % w) && intra_nb_avail (k - 1))) dcpred = true;
          else modeA = left[by];
          if (by > 0) modeB = ipm[(by - 1) * 4 + bx];
          else if (!(k >= w && intra_nb_avail (k - w))) dcpred = true;
          else modeB = line[(k % w) * 4 + bx];
          const int pred = dcpred ? 2 : imin (modeA, modeB);
          int mode = pred;
          if (!br.u1()) { const int rem = (int)br.u (3); mode = rem < pred ? rem : rem + 1; }
          const int nn = t8 ? 2 : 1;
          for (int yy = 0; yy < nn; yy++) for (int x = 0; x < nn; x++) { ipm[(by + yy) * 4 + bx + x] = (int8_t)mode; raw_modes[(by + yy) * 4 + bx + x] = mode; }
        }
        have_raw = true;
        chroma_mode = (int)br.ue();
        const uint32_t ci = br.ue();
        if (ci > 47 || chroma_mode < 0 || chroma_mode > 3) return false;
        cbp = T->cbp_intra[ci];
      } else {                                            // Intra16x16
        m->mb_type = LH264_MB_I16x16;
        i16mode = (int) ((mbt - 1) & 3);
        cbp = (int) ((((mbt - 1) >> 2) % 3) << 4 | ((mbt - 1) >= 12 ? 15 : 0));
        chroma_mode = (int)br.ue();
        if (chroma_mode < 0 || chroma_mode > 3) return false;
      }
    } else {                                              // P macroblocks
      m->mb_type = (uint16_t) (mbt == 0 ? LH264_MB_P16x16 : mbt == 1 ? LH264_MB_P16x8 : mbt == 2 ? LH264_MB_P8x16 : mbt == 3 ? LH264_MB_P8x8 : LH264_MB_P8x8REF0);
      const int nref = t->num_ref_idx_l0;
      uint32_t filled = 0;
      if (mbt <= 2) {
        const int np = mbt == 0 ? 1 : 2;
        int ref[2];
        for (int i = 0; i < np; i++) { ref[i] = read_ref (nref); if (ref[i] < 0 || ref[i] >= nref) return false; }
        for (int i = 0; i < np; i++) {
          int bx = 0, by = 0, bw = 4, bh = 4, shape = 0;
          if (mbt == 1) { bh = 2; by = i * 2; shape = 1 + i; } else if (mbt == 2) { bw = 2; bx = i * 2; shape = 3 + i; }
          for (int q = 0; q < 4; q++) if ((q >> 1) * 2 >= by && (q >> 1) * 2 < by + bh && (q & 1) * 2 >= bx && (q & 1) * 2 < bx + bw) m->ref_idx[q] = (int8_t)ref[i];
          int px, py;
          predict_mv (filled, bx, by, bw, ref[i], shape, px, py);
          const int dx = br.se(), dy = br.se();
          fill_part (bx, by, bw, bh, px + dx, py + dy, filled);
        }
      } else {
        int sub[4], ref[4] = {0, 0, 0, 0};
        for (int q = 0; q < 4; q++) { const uint32_t sv = br.ue(); if (sv > 3) return false; sub[q] = (int)sv; m->sub_type[q] = (uint8_t) (1 << sub[q]); }
        if (mbt == 3) for (int q = 0; q < 4; q++) { ref[q] = read_ref (nref); if (ref[q] < 0 || ref[q] >= nref) return false; }
        for (int q = 0; q < 4; q++) m->ref_idx[q] = (int8_t)ref[q];
        for (int q = 0; q < 4; q++) {
          const int qx = (q & 1) * 2, qy = (q >> 1) * 2;
          const int nsp = sub[q] == 0 ? 1 : sub[q] == 3 ? 4 : 2;
          for (int j = 0; j < nsp; j++) {
            int bx = qx, by = qy, bw = 2, bh = 2;
            if (sub[q] == 1) { bh = 1; by += j; } else if (sub[q] == 2) { bw = 1; bx += j; } else if (sub[q] == 3) { bw = bh = 1; bx += j & 1; by += j >> 1; }
            int px, py;
            predict_mv (filled, bx, by, bw, ref[q], 0, px, py);
            const int dx = br.se(), dy = br.se();
            fill_part (bx, by, bw, bh, px + dx, py + dy, filled);
          }
        }
      }
      const uint32_t ci = br.ue();
      if (ci > 47) return false;
      cbp = T->cbp_inter[ci];
      bool no_sub_lt8 = true;
      if (mbt >= 3) for (int q = 0; q < 4; q++) if (m->sub_type[q] != LH264_SUB_8x8) no_sub_lt8 = false;
      if ((cbp & 15) && t->transform_8x8 && no_sub_lt8) t8 = br.u1() != 0;
    }
    if (br.err) return false;
    m->cbp = (uint8_t)cbp;
    if (t8) m->flags |= LH264_MBF_T8x8;
    if (intra) finalize_intra_modes (have_raw ? raw_modes : nullptr, t8, i16mode, chroma_mode);
    int qp = qp_prev;
    const bool i16 = m->mb_type == LH264_MB_I16x16;
    if (cbp || i16) {
      const int dqp = br.se();
      if (dqp < -26 || dqp > 25) return false;
      qp = ((qp_prev + dqp) % 52 + 52) % 52;
    }
    set_qp (qp);
    qp_prev = qp;
    if (!(cbp || i16)) return !br.err;

    // ---- residual (7.3.5.3)
    int lv[16];
    const int ylist = intra ? 0 : 3;
    if (i16) {
      if (residual_block (*T, br, luma_nC (0, 0), 16, lv) < 0) return false;
      for (int i = 0; i < 16; i++) if (lv[i]) {
          const int r = T->zigzag4[i], zb = xy2z (r & 3, r >> 2);
          put (coef, zb * 16, lv[i]);                       // dequantised by the DC transform in the reconstruct kernel
        }
    }
    for (int i8 = 0; i8 < 4; i8++) {
      if (!((cbp >> i8) & 1)) continue;
      for (int j = 0; j < 4; j++) {
        const int z = i8 * 4 + j, bx = z2x (z), by = z2y (z);
        const int maxc = i16 ? 15 : 16;
        const int tot = residual_block (*T, br, luma_nC (bx, by), maxc, lv);
        if (tot < 0) return false;
        m->nzc[by * 4 + bx] = (uint8_t)tot;
        for (int i = 0; i < maxc; i++) if (lv[i]) {
            if (t8) { const int pos = T->zigzag8[4 * i + j]; put (coef, i8 * 64 + pos, dq8 (intra ? 0 : 1, qp, pos, lv[i])); }
            else { const int pos = T->zigzag4[i16 ? i + 1 : i]; put (coef, z * 16 + pos, dq4 (ylist, qp, pos, lv[i])); }
          }
      }
    }
    const int cbpc = cbp >> 4;
    if (cbpc) {
      for (int p = 0; p < 2; p++) {                       // chroma DC, nC = -1
        if (residual_block (*T, br, -1, 4, lv) < 0) return false;
        const int qc = m->qp_c[p];
        const int d0 = T->norm4[qc % 6][0] << (qc / 6);
        for (int i = 0; i < 4; i++) if (lv[i]) put (coef, 256 + p * 64 + i * 16, t->use_sl ? (lv[i] * (t->scaling[(ylist + 1 + p) * 16] * d0)) >> 4 : lv[i] * d0);
      }
      if (cbpc == 2) {
        for (int p = 0; p < 2; p++) for (int j = 0; j < 4; j++) {
            const int bx = j & 1, by = j >> 1;
            bool aA, aB;
            const int nA = nz_chroma (p, bx - 1, by, aA), nB = nz_chroma (p, bx, by - 1, aB);
            const int tot = residual_block (*T, br, nC_of (nA, aA, nB, aB), 15, lv);
            if (tot < 0) return false;
            m->nzc[T->chroma_nzc_idx[p][j]] = (uint8_t)tot;
            for (int i = 0; i < 15; i++) if (lv[i]) { const int pos = T->zigzag4[i + 1]; put (coef, 256 + p * 64 + j * 16 + pos, dq4 (ylist + 1 + p, m->qp_c[p], pos, lv[i])); }
          }
      }
    }
    return !br.err;
  }
  LH264S_HD int read_ref (int nref) { if (nref <= 1) return 0; if (nref == 2) return br.u1() ? 0 : 1; return (int)br.ue(); }
};

enum { SLICE_OK = 0, SLICE_SYNTAX = 1, SLICE_OVERRUN = 2, SLICE_BAD_TASK = 3 };
// SliceTask::reserved: 0 for a CAVLC task; for a CABAC task (lh264_slice_cabac.h) bit 7 and cabac_init_idc, 0..2, in bits 0..1
enum { kTaskCabac = 0x80, kTaskCabacIdcMask = 0x03 };
LH264S_HD inline bool task_is_cabac (const SliceTask& t) { return (t.reserved & kTaskCabac) != 0; }

// what the walk takes on trust from the host: checked before anything is read or written
LH264S_HD inline bool task_ok (const SliceTask& t, bool cabac = false) {
  if (!t.rbsp || !t.mbs || !t.coeffs || (t.use_sl && !t.scaling)) return false;      // (slice may be null: n_mbs is in the result too)
  if (t.mb_w <= 0 || t.mb_h <= 0 || t.mb_w > 4096 || t.mb_h > 4096) return false;
  const int n = t.mb_w * t.mb_h;
  if (t.first_mb < 0 || t.first_mb >= t.limit_mb || t.limit_mb > n) return false;
  if (t.rbsp_bytes >= (1u << 28) || t.data_bit > t.rbsp_bytes * 8) return false;
  if ((t.slice_type != 0 && t.slice_type != 2) || t.num_ref_idx_l0 < 1 || t.num_ref_idx_l0 > 32) return false;
  if (t.slice_qp < -1024 || t.slice_qp > 1024 || t.chroma_qp_offset[0] < -12 || t.chroma_qp_offset[0] > 12 || t.chroma_qp_offset[1] < -12 || t.chroma_qp_offset[1] > 12) return false;
  if (((uintptr_t)t.mbs & 15) || ((uintptr_t)t.coeffs & 1) || ((uintptr_t)t.slice & 3)) return false;
  if (t.mb_w > kLdsLineMbs && !t.line) return false;
  if (cabac ? (t.reserved < kTaskCabac || t.reserved > (kTaskCabac | 2)) : t.reserved != 0) return false;      // the entropy mode is the walk's, cabac_init_idc is defined
  return true;
}

// The slice of one task: slice_data() as the host's parse_slice_data_cavlc walks it.  scratch: a record for the macroblock in hand
// (16-byte aligned); line: 4 bytes per macroblock column (contents do not matter).  A status other than SLICE_OK where the host fails -
// or, SLICE_OVERRUN, where the slice is about to write macroblock limit_mb of a picture that has a later slice: the host lets the
// later slice overwrite, here nothing at or beyond limit_mb is ever written.
LH264S_HD inline SliceResult parse_slice (const Tables& T, const SliceTask& t, lh264_mb_t* scratch, int8_t* line) {
  SliceResult r = {SLICE_BAD_TASK, 0, 0};
  if (!task_ok (t) || !scratch || !line) return r;
  Walk W;
  W.T = &T; W.t = &t; W.m = scratch; W.line = line;
  W.w = t.mb_w; W.n = t.mb_w * t.mb_h; W.first = t.first_mb; W.k = t.first_mb;
  for (int i = 0; i < 4; i++) W.left[i] = 2;
  W.br.init (t.rbsp, t.rbsp_bytes, t.data_bit);
  const int n = W.n, limit = t.limit_mb;
  int qp_prev = t.slice_qp, count = 0, status = SLICE_OK;
  bool more = true;
  while (more && W.k < n) {
    if (t.slice_type != 2) {
      const uint32_t run = W.br.ue();
      if (W.br.err || run > (uint32_t) (n - W.k)) { status = SLICE_SYNTAX; break; }
      if (run > (uint32_t) (limit - W.k)) { status = SLICE_OVERRUN; break; }
      for (uint32_t i = 0; i < run; i++, W.k++, count++) { W.parse_mb (qp_prev, true); W.done(); }
      more = W.br.more_rbsp_data();
      if (!more || W.k >= n) break;
    }
    if (W.k >= limit) { status = SLICE_OVERRUN; break; }
    if (!W.parse_mb (qp_prev, false)) { status = SLICE_SYNTAX; break; }
    W.done();
    W.k++; count++;
    more = W.br.more_rbsp_data();
  }
  r.status = status; r.n_mbs = count; r.stop_bit = (int32_t)W.br.pos;
  if (status == SLICE_OK && t.slice) t.slice->n_mbs = count;
  return r;
}

}  // namespace lh264slice
