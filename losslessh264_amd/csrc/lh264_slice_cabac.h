// lh264_slice_cabac.h - the CABAC macroblock layer of one slice (7.3.4, 7.3.5, 9.3), host and device from one source: what
// host/h264_parser.cpp does in Cabac / parse_slice_data_cabac / parse_mb_cabac / cabac_residual, in the same decision order, without the
// recompressor's bookkeeping (MbSyn, levels, I_PCM sample stream, the persist_* arrays).  What a macroblock becomes once its syntax
// elements are known is lh264slice::WalkOps (lh264_slice.h), shared with the CAVLC walk.  slice_parse_cabac_kernel (lh264_slice.hip)
// walks one slice per wave, lh264_debug_slice_parse_opts steps the same code over host memory.
//
// Every bound is the task's: the reader never leaves [rbsp, rbsp + rbsp_bytes) - bits beyond the end read as zeros and the engine
// gives up 64 bits past it, as Cabac::bit() does -, no macroblock outside [first_mb, limit_mb) is written, no coefficient index reaches
// 384, the samples of an I_PCM macroblock are taken only while they lie inside the payload.  Every loop has the host's cap: 32 on
// ref_idx, 24 on Exp-Golomb prefixes, 120 on mb_qp_delta, mb_w * mb_h macroblocks for the slice: the walk ends on any input.
//
// Neighbour state.  skip, I_PCM, the transform size, cbp, the type class, ref_idx and mv of macroblocks k - 1 and k - mb_w are read
// from the records the walk wrote; "intra_chroma_pred_mode != 0" is read from the record's final chroma_mode (LH264_C_H, _V, _P: the
// three DC forms and the inter macroblocks' 0 all stand for "0").  What no record holds lies in the line, kCabacLineBytes per macroblock
// column for the macroblock parsed last in that column - the four raw intra modes of its bottom row, the eight saturated |mvd| bytes
// of its bottom row, its coded_block_flag word - and, for macroblock k - 1, in the walk itself.
#pragma once
#include "lh264_slice.h"
#include "host/h264_cabac_tables.h"
#include "host/h264_cabac_ctx_tables.h"

namespace lh264slice {

enum { kCabacLineBytes = 16, kCabacContexts = 460 };      // SliceTask::line of a CABAC task: kCabacLineBytes * mb_w bytes

struct alignas (16) CabacTables {
  uint8_t range_lps[64][4], next_lps[64], next_mps[64];
  uint8_t sig8x8[63], last8x8[63], cat_cbf[5], cat_map[5], cat_abs[5];
  uint8_t zigzag4[16], zigzag8[64], chroma_qp[52], norm4[6][3], norm8[6][6], chroma_nzc_idx[2][4];
};
static_assert (sizeof (CabacTables) % 16 == 0 && sizeof (CabacTables) < 2048, "the table record is copied into LDS 16 bytes at a time");

#define LH264S_TAKE(dst, src) static_assert (sizeof (dst) == sizeof (src), #src); memcpy (dst, src, sizeof (dst))
inline void fill_cabac_tables (CabacTables& t) {
  using namespace lh264host;
  memset (&t, 0, sizeof (t));
  LH264S_TAKE (t.range_lps, kCabacRangeLps); LH264S_TAKE (t.next_lps, kCabacNextLps); LH264S_TAKE (t.next_mps, kCabacNextMps);
  LH264S_TAKE (t.sig8x8, kSig8x8); LH264S_TAKE (t.last8x8, kLast8x8); LH264S_TAKE (t.cat_cbf, kCatCbf); LH264S_TAKE (t.cat_map, kCatMap); LH264S_TAKE (t.cat_abs, kCatAbs);
  LH264S_TAKE (t.zigzag4, kZigzag4x4); LH264S_TAKE (t.zigzag8, kZigzag8x8); LH264S_TAKE (t.chroma_qp, kChromaQp);
  LH264S_TAKE (t.norm4, kNormAdjust4x4); LH264S_TAKE (t.norm8, kNormAdjust8x8); LH264S_TAKE (t.chroma_nzc_idx, kChromaNzcIdx);
}
#undef LH264S_TAKE

// one context's initial state (9.3.1.1): pStateIdx << 1 | valMPS from the slice's (m, n) and SliceQPY
LH264S_HD inline uint8_t cabac_init_state (int m, int n, int qp) {
  qp = imin (51, imax (0, qp));
  const int pre = imin (126, imax (1, ((m * qp) >> 4) + n));
  return pre <= 63 ? (uint8_t) ((63 - pre) << 1) : (uint8_t) (((pre - 64) << 1) | 1);
}
// the column of the (m, n) table a slice reads
LH264S_HD inline int cabac_init_column (const SliceTask& t) { return t.slice_type == 2 ? 0 : 1 + (t.reserved & kTaskCabacIdcMask); }

// ---- the arithmetic decoding engine (9.3.1.2, 9.3.3.2): lh264host's Cabac bounded by the task --------------------------------------------
struct CabacEngine {
  const CabacTables* T; const uint8_t* p; uint32_t nbytes, nbits, pos; uint32_t range, offset; bool err;
  uint8_t* state;                   // kCabacContexts bytes, initialised by the caller (LDS on the device)
  uint64_t win; uint32_t wbyte; bool whave;      // the 8 bytes at byte wbyte, big-endian, zero beyond the end
  LH264S_HD void load (uint32_t b) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < 8; i++) v = (v << 8) | (b < nbytes && i < nbytes - b ? p[b + i] : 0);
    win = v; wbyte = b; whave = true;
  }
  LH264S_HD uint32_t bit() {
    if (pos >= nbits) { pos++; if (pos > nbits + 64) err = true; return 0; }
    const uint32_t b = pos >> 3;
    if (!whave || b < wbyte || b - wbyte > 7) load (b);
    const uint32_t v = (uint32_t) (win >> (63 - (pos - wbyte * 8))) & 1u;
    pos++;
    return v;
  }
  LH264S_HD void start (uint32_t bitpos) {
    pos = bitpos; range = 510; offset = 0;
    for (int i = 0; i < 9; i++) offset = (offset << 1) | bit();
  }
  LH264S_HD int decode (int ctx) {
    if ((unsigned)ctx >= (unsigned)kCabacContexts) { err = true; return 0; }      // (cannot happen: every index below is within its range)
    const uint8_t s = state[ctx];
    const int st = s >> 1; int mps = s & 1;
    const uint32_t lps = T->range_lps[st][(range >> 6) & 3];
    range -= lps;
    int b;
    if (offset >= range) {
      b = !mps; offset -= range; range = lps;
      if (st == 0) mps = !mps;
      state[ctx] = (uint8_t) ((T->next_lps[st] << 1) | mps);
    } else { b = mps; state[ctx] = (uint8_t) ((T->next_mps[st] << 1) | mps); }
    while (range < 256) { range <<= 1; offset = (offset << 1) | bit(); }
    return b;
  }
  LH264S_HD int bypass() { offset = (offset << 1) | bit(); if (offset >= range) { offset -= range; return 1; } return 0; }
  LH264S_HD int terminate() {
    range -= 2;
    if (offset >= range) return 1;
    while (range < 256) { range <<= 1; offset = (offset << 1) | bit(); }
    return 0;
  }
};

// ---- the walk over one slice --------------------------------------------------------------------------------------------------------
struct CabacWalk : WalkOps<CabacWalk> {
  const CabacTables* T; const SliceTask* t;
  lh264_mb_t* m;            // the record in hand, copied to t->mbs[k] when the macroblock is done
  int w, n, first, k;
  CabacEngine cb;
  uint8_t* line;            // kCabacLineBytes per column: raw intra modes (0..3), |mvd| of the bottom row (4 + block * 2 + comp), cbf (12..15, little-endian)
  int8_t left[4]; uint8_t left_mvd[4][2]; uint32_t left_cbf;      // the same of macroblock k - 1: its right column
  int8_t ipm[16]; uint8_t mvd[16][2]; uint32_t cbf;               // ... of the macroblock in hand
  int kA, kB;               // macroblocks k - 1 and k - mb_w where they are available, else -1

  LH264S_HD static uint32_t type_class (const lh264_mb_t& r) { return (r.mb_type & (LH264_MB_I4x4 | LH264_MB_I8x8)) ? 1 : (r.mb_type & (LH264_MB_I16x16 | LH264_MB_IPCM)) ? 2 : 3; }
  LH264S_HD static bool is_skip (const lh264_mb_t& r) { return r.mb_type == LH264_MB_SKIP; }
  LH264S_HD static bool is_pcm (const lh264_mb_t& r) { return r.mb_type == LH264_MB_IPCM; }
  LH264S_HD static bool is_t8 (const lh264_mb_t& r) { return (r.flags & LH264_MBF_T8x8) != 0; }
  LH264S_HD static bool chroma_pred_nz (const lh264_mb_t& r) {
    return (r.mb_type & (LH264_MB_I4x4 | LH264_MB_I8x8 | LH264_MB_I16x16)) && (r.chroma_mode == LH264_C_H || r.chroma_mode == LH264_C_V || r.chroma_mode == LH264_C_P);
  }
  LH264S_HD uint32_t line_cbf (int col) const {
    const uint8_t* q = line + (size_t)col * kCabacLineBytes + 12;
    return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
  }
  // the macroblock in hand is done: its record goes out, what the records do not hold becomes the neighbours' context
  LH264S_HD void done() {
    store_record();
    uint8_t* q = line + (size_t) (k % w) * kCabacLineBytes;
    for (int i = 0; i < 4; i++) {
      q[i] = (uint8_t)ipm[12 + i]; left[i] = ipm[i * 4 + 3];
      q[4 + i * 2] = mvd[12 + i][0]; q[5 + i * 2] = mvd[12 + i][1];
      left_mvd[i][0] = mvd[i * 4 + 3][0]; left_mvd[i][1] = mvd[i * 4 + 3][1];
      q[12 + i] = (uint8_t) (cbf >> (8 * i));
    }
    left_cbf = cbf;
  }

  // one residual block (7.3.5.3.3): the number of nonzero coefficients, levels in scan order in lv[0..maxc-1]
  LH264S_HD int residual (int cat, int blk, int plane, bool cur_intra, int* lv, int maxc) {
    for (int i = 0; i < maxc; i++) lv[i] = 0;
    if (cat != 5) {
      // coded_block_flag, ctxIdxInc = condTermFlagA + 2 condTermFlagB (9.3.3.1.1.9)
      int bit, bitA, bitB; bool inA = true, inB = true;       // in: the neighbouring block lies in the macroblock in hand
      if (cat == 0) { bit = bitA = bitB = 16; inA = inB = false; }
      else if (cat == 3) { bit = bitA = bitB = 17 + plane; inA = inB = false; }
      else if (cat == 4) {
        const int cx = blk & 1, cy = blk >> 1;
        bit = 19 + plane * 4 + blk;
        if (cx == 0) { inA = false; bitA = 19 + plane * 4 + cy * 2 + 1; } else bitA = bit - 1;
        if (cy == 0) { inB = false; bitB = 19 + plane * 4 + 2 + cx; } else bitB = bit - 2;
      } else {
        const int bx = blk & 3, by = blk >> 2;
        bit = blk;
        if (bx == 0) { inA = false; bitA = by * 4 + 3; } else bitA = blk - 1;
        if (by == 0) { inB = false; bitB = 12 + bx; } else bitB = blk - 4;
      }
      const int cA = inA ? (int) ((cbf >> bitA) & 1) : kA < 0 ? (cur_intra ? 1 : 0) : (int) ((left_cbf >> bitA) & 1);
      const int cBf = inB ? (int) ((cbf >> bitB) & 1) : kB < 0 ? (cur_intra ? 1 : 0) : (int) ((line_cbf (k % w) >> bitB) & 1);
      if (!cb.decode (85 + T->cat_cbf[cat] + cA + 2 * cBf)) return 0;
      cbf |= 1u << bit;
    }
    const int sig_base = cat == 5 ? 402 : 105 + T->cat_map[cat], last_base = cat == 5 ? 417 : 166 + T->cat_map[cat];
    const int abs_base = cat == 5 ? 426 : 227 + T->cat_abs[cat];
    uint8_t sig[64];
    int n_sig = 0, i;
    for (i = 0; i < maxc - 1; i++) {
      const int inc_s = cat == 5 ? T->sig8x8[i] : cat == 3 ? imin (i, 2) : i;
      const int inc_l = cat == 5 ? T->last8x8[i] : cat == 3 ? imin (i, 2) : i;
      if (cb.decode (sig_base + inc_s)) {
        sig[n_sig++] = (uint8_t)i;
        if (cb.decode (last_base + inc_l)) break;
      }
    }
    if (i == maxc - 1) sig[n_sig++] = (uint8_t) (maxc - 1);      // the last position is significant by inference
    int num_eq1 = 0, num_gt1 = 0;
    for (int j = n_sig - 1; j >= 0; j--) {
      int inc = num_gt1 ? 0 : imin (4, 1 + num_eq1);
      int v = 0;                                                   // coeff_abs_level_minus1: TU prefix (cMax 14) + EG0 suffix
      if (cb.decode (abs_base + inc)) {
        v = 1;
        inc = 5 + imin (4 - (cat == 3 ? 1 : 0), num_gt1);
        while (v < 14 && cb.decode (abs_base + inc)) v++;
        if (v == 14) {
          int kk = 0;
          while (cb.bypass()) { v += 1 << kk; kk++; if (kk > 24) { cb.err = true; break; } }
          while (kk--) v += cb.bypass() << kk;
        }
      }
      const int mag = v + 1;
      lv[sig[j]] = cb.bypass() ? -mag : mag;
      if (mag == 1) num_eq1++; else num_gt1++;
    }
    return n_sig;
  }

  // the mb_type of an I slice, or the suffix of an intra macroblock in a P slice (9.3.2.5, 9.3.3.1.1.3)
  LH264S_HD int i_type (bool islice) {
    int b0;
    if (islice) {
      const int cA = kA >= 0 && type_class (t->mbs[kA]) != 1, cBn = kB >= 0 && type_class (t->mbs[kB]) != 1;       // neighbour is not I_NxN
      b0 = cb.decode (3 + cA + cBn);
    } else b0 = cb.decode (17);
    if (!b0) return 0;
    if (cb.terminate()) return 25;
    const int base = islice ? 3 : 17;
    const int luma = cb.decode (base + (islice ? 3 : 1));
    const int b3 = cb.decode (base + (islice ? 4 : 2));
    int chroma = 0;
    if (b3) chroma = cb.decode (base + (islice ? 5 : 2)) ? 2 : 1;
    const int p0 = cb.decode (base + (islice ? 6 : 3)), p1 = cb.decode (base + (islice ? 7 : 3));
    return 1 + (p0 << 1 | p1) + 4 * chroma + 12 * luma;
  }
  LH264S_HD int chroma_pred() {                          // intra_chroma_pred_mode, 9.3.3.1.1.8
    const int cA = kA >= 0 && chroma_pred_nz (t->mbs[kA]), cBn = kB >= 0 && chroma_pred_nz (t->mbs[kB]);
    if (!cb.decode (64 + cA + cBn)) return 0;
    if (!cb.decode (67)) return 1;
    return cb.decode (67) ? 3 : 2;
  }
  // ref_idx_l0 of the partition whose first 4x4 block is (bx,by): ctxIdxInc from the partitions to the left and above
  LH264S_HD int ref_gt0 (int bx, int by) const {
    const lh264_mb_t* s = m;
    int x = bx, yy = by;
    if (x < 0) { if (kA < 0) return 0; s = &t->mbs[kA]; x = 3; } else if (yy < 0) { if (kB < 0) return 0; s = &t->mbs[kB]; yy = 3; }
    if (type_class (*s) != 3 || is_skip (*s)) return 0;
    return s->ref_idx[(yy >> 1) * 2 + (x >> 1)] > 0;
  }
  LH264S_HD int read_ref (int nref, int bx, int by) {
    if (nref <= 1) return 0;
    int inc = ref_gt0 (bx - 1, by) + 2 * ref_gt0 (bx, by - 1), v = 0;
    while (cb.decode (54 + inc)) { v++; inc = v == 1 ? 4 : 5; if (v > 32) { cb.err = true; break; } }
    return v;
  }
  LH264S_HD int abs_mvd (int bx, int by, int comp) const {
    if (bx < 0) return kA < 0 ? 0 : left_mvd[by][comp];
    if (by < 0) return kB < 0 ? 0 : line[(size_t) (k % w) * kCabacLineBytes + 4 + bx * 2 + comp];
    return mvd[by * 4 + bx][comp];
  }
  LH264S_HD int read_mvd (int bx, int by, int comp) {   // UEG3, signedValFlag 1, uCoff 9 (9.3.2.3, 9.3.3.1.1.7)
    const int base = comp ? 47 : 40;
    const int sum = abs_mvd (bx - 1, by, comp) + abs_mvd (bx, by - 1, comp);
    int inc = sum < 3 ? 0 : sum > 32 ? 2 : 1;
    if (!cb.decode (base + inc)) return 0;
    int v = 1;
    inc = 3;
    while (v < 9 && cb.decode (base + inc)) { v++; if (inc < 6) inc++; }
    if (v == 9) {
      int kk = 3;
      while (cb.bypass()) { v += 1 << kk; kk++; if (kk > 24) { cb.err = true; break; } }
      while (kk--) v += cb.bypass() << kk;
    }
    return cb.bypass() ? -v : v;
  }
  LH264S_HD void fill_part_mvd (int bx, int by, int bw, int bh, int mvx, int mvy, int dx, int dy, uint32_t& filled) {
    const uint8_t ax = (uint8_t)imin (255, dx < 0 ? -dx : dx), ay = (uint8_t)imin (255, dy < 0 ? -dy : dy);
    fill_part (bx, by, bw, bh, mvx, mvy, filled);
    for (int y = by; y < by + bh; y++) for (int x = bx; x < bx + bw; x++) { mvd[y * 4 + x][0] = ax; mvd[y * 4 + x][1] = ay; }
  }
  // condTermFlagN of coded_block_pattern (9.3.3.1.1.4) for a neighbouring macroblock
  LH264S_HD int cbp_luma_bit (int kk, int b8) const {
    if (kk < 0) return 0;
    const lh264_mb_t& s = t->mbs[kk];
    if (is_pcm (s)) return 0;
    if (is_skip (s)) return 1;
    return ((s.cbp >> b8) & 1) ? 0 : 1;
  }
  LH264S_HD int cbp_chroma_nz (int kk, int lvl) const {
    if (kk < 0) return 0;
    const lh264_mb_t& s = t->mbs[kk];
    if (is_pcm (s)) return 1;
    if (is_skip (s)) return 0;
    return (s.cbp >> 4) >= lvl;
  }
  LH264S_HD int t8_inc() const { return (kA >= 0 && is_t8 (t->mbs[kA])) + (kB >= 0 && is_t8 (t->mbs[kB])); }

  // one macroblock (7.3.5); false where the host's parse_mb_cabac returns false
  LH264S_HD bool parse_mb (int& qp_prev, int& last_dqp, bool skip) {
    memset (m, 0, sizeof (*m));
    m->slice_id = (uint16_t)t->slice_index;
    for (int i = 0; i < 16; i++) { ipm[i] = 2; mvd[i][0] = mvd[i][1] = 0; }
    for (int i = 0; i < 4; i++) m->ref_idx[i] = -1;
    cbf = 0;
    int16_t* coef = t->coeffs + (size_t)k * 384;
    kA = ((k % w) && avail (k - 1)) ? k - 1 : -1; kB = (k >= w && avail (k - w)) ? k - w : -1;
    if (skip) {                                           // P_Skip
      m->mb_type = LH264_MB_SKIP;
      for (int i = 0; i < 4; i++) m->ref_idx[i] = 0;
      const Nb A = nb_block (-1, 0, 0), B = nb_block (0, -1, 0);
      int px = 0, py = 0;
      if (A.avail && B.avail && !(A.ref == 0 && A.mvx == 0 && A.mvy == 0) && !(B.ref == 0 && B.mvx == 0 && B.mvy == 0))
        predict_mv (0, 0, 0, 4, 0, 0, px, py);
      uint32_t filled = 0;
      fill_part (0, 0, 4, 4, px, py, filled);
      set_qp (qp_prev);
      last_dqp = 0;
      return true;
    }
    uint32_t mbt;
    bool intra = true;
    if (t->slice_type == 2) mbt = (uint32_t)i_type (true);
    else if (cb.decode (14)) mbt = (uint32_t)i_type (false);
    else {
      intra = false;
      if (!cb.decode (15)) mbt = cb.decode (16) ? 3 : 0;
      else mbt = cb.decode (17) ? 1 : 2;
    }
    if (cb.err) return false;
    int cbp = 0;
    bool t8 = false;
    int raw_modes[16]; bool have_raw = false; int i16mode = -1, chroma_mode = -1;
    if (intra) {
      if (mbt == 25) {                                    // I_PCM: the samples follow byte aligned, then the engine restarts (9.3.1.2)
        m->mb_type = LH264_MB_IPCM; cbf = 0xffffffffu;
        uint32_t bp = (cb.pos + 7) & ~7u;
        for (int i = 0; i < 384; i++, bp += 8) put (coef, i, bp + 8 <= cb.nbits ? cb.p[bp >> 3] : 0);
        if (bp > cb.nbits) cb.err = true;
        cb.start (bp);
        m->flags |= LH264_MBF_PCM_IN_COEFF;
        memset (m->nzc, 16, 24);
        m->qp_y = 0; m->qp_c[0] = m->qp_c[1] = 0;
        finalize_intra_modes (nullptr, false, -1, -1);
        last_dqp = 0;
        return !cb.err;
      }
      if (mbt == 0) {                                     // I_NxN
        if (t->transform_8x8) t8 = cb.decode (399 + t8_inc()) != 0;
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
          else modeB = (int8_t)line[(size_t) (k % w) * kCabacLineBytes + bx];
          const int pred = dcpred ? 2 : imin (modeA, modeB);
          int mode = pred;
          if (!cb.decode (68)) { int rem = cb.decode (69); rem |= cb.decode (69) << 1; rem |= cb.decode (69) << 2; mode = rem < pred ? rem : rem + 1; }
          const int nn = t8 ? 2 : 1;
          for (int yy = 0; yy < nn; yy++) for (int x = 0; x < nn; x++) { ipm[(by + yy) * 4 + bx + x] = (int8_t)mode; raw_modes[(by + yy) * 4 + bx + x] = mode; }
        }
        have_raw = true;
        chroma_mode = chroma_pred();
      } else {                                            // Intra16x16
        m->mb_type = LH264_MB_I16x16;
        i16mode = (int) ((mbt - 1) & 3);
        cbp = (int) ((((mbt - 1) >> 2) % 3) << 4 | ((mbt - 1) >= 12 ? 15 : 0));
        chroma_mode = chroma_pred();
      }
    } else {                                              // P macroblocks
      m->mb_type = (uint16_t) (mbt == 0 ? LH264_MB_P16x16 : mbt == 1 ? LH264_MB_P16x8 : mbt == 2 ? LH264_MB_P8x16 : LH264_MB_P8x8);
      const int nref = t->num_ref_idx_l0;
      uint32_t filled = 0;
      if (mbt <= 2) {
        const int np = mbt == 0 ? 1 : 2;
        int ref[2];
        for (int i = 0; i < np; i++) {
          const int bx = mbt == 2 ? i * 2 : 0, by = mbt == 1 ? i * 2 : 0;
          ref[i] = read_ref (nref, bx, by);
          if (ref[i] < 0 || ref[i] >= nref) return false;
          for (int q = 0; q < 4; q++) {
            const bool in = mbt == 0 || (mbt == 1 ? (q >> 1) == i : (q & 1) == i);
            if (in) m->ref_idx[q] = (int8_t)ref[i];
          }
        }
        for (int i = 0; i < np; i++) {
          int bx = 0, by = 0, bw = 4, bh = 4, shape = 0;
          if (mbt == 1) { bh = 2; by = i * 2; shape = 1 + i; } else if (mbt == 2) { bw = 2; bx = i * 2; shape = 3 + i; }
          int px, py;
          predict_mv (filled, bx, by, bw, ref[i], shape, px, py);
          const int dx = read_mvd (bx, by, 0), dy = read_mvd (bx, by, 1);
          fill_part_mvd (bx, by, bw, bh, px + dx, py + dy, dx, dy, filled);
        }
      } else {
        int sub[4], ref[4] = {0, 0, 0, 0};
        for (int q = 0; q < 4; q++) {                     // sub_mb_type, Table 9-37
          if (cb.decode (21)) sub[q] = 0;
          else if (!cb.decode (22)) sub[q] = 1;
          else sub[q] = cb.decode (23) ? 2 : 3;
          m->sub_type[q] = (uint8_t) (1 << sub[q]);
        }
        for (int q = 0; q < 4; q++) {
          ref[q] = read_ref (nref, (q & 1) * 2, (q >> 1) * 2);
          if (ref[q] < 0 || ref[q] >= nref) return false;
          m->ref_idx[q] = (int8_t)ref[q];
        }
        for (int q = 0; q < 4; q++) {
          const int qx = (q & 1) * 2, qy = (q >> 1) * 2;
          const int nsp = sub[q] == 0 ? 1 : sub[q] == 3 ? 4 : 2;
          for (int j = 0; j < nsp; j++) {
            int bx = qx, by = qy, bw = 2, bh = 2;
            if (sub[q] == 1) { bh = 1; by += j; } else if (sub[q] == 2) { bw = 1; bx += j; } else if (sub[q] == 3) { bw = bh = 1; bx += j & 1; by += j >> 1; }
            int px, py;
            predict_mv (filled, bx, by, bw, ref[q], 0, px, py);
            const int dx = read_mvd (bx, by, 0), dy = read_mvd (bx, by, 1);
            fill_part_mvd (bx, by, bw, bh, px + dx, py + dy, dx, dy, filled);
          }
        }
      }
    }
    if (cb.err) return false;
    const bool i16 = m->mb_type == LH264_MB_I16x16;
    if (!i16) {                                           // coded_block_pattern, 9.3.2.6 / 9.3.3.1.1.4
      int cl = 0;
      for (int b8 = 0; b8 < 4; b8++) {
        const int cA = (b8 & 1) ? (((cl >> (b8 - 1)) & 1) ? 0 : 1) : cbp_luma_bit (kA, b8 + 1);
        const int cBn = (b8 & 2) ? (((cl >> (b8 - 2)) & 1) ? 0 : 1) : cbp_luma_bit (kB, b8 + 2);
        cl |= cb.decode (73 + cA + 2 * cBn) << b8;
      }
      int cc = 0;
      if (cb.decode (77 + cbp_chroma_nz (kA, 1) + 2 * cbp_chroma_nz (kB, 1))) cc = cb.decode (77 + 4 + cbp_chroma_nz (kA, 2) + 2 * cbp_chroma_nz (kB, 2)) ? 2 : 1;
      cbp = cl | (cc << 4);
      if (!intra) {
        bool no_sub_lt8 = true;
        if (mbt == 3) for (int q = 0; q < 4; q++) if (m->sub_type[q] != LH264_SUB_8x8) no_sub_lt8 = false;
        if ((cbp & 15) && t->transform_8x8 && no_sub_lt8) t8 = cb.decode (399 + t8_inc()) != 0;
      }
    }
    if (cb.err) return false;
    m->cbp = (uint8_t)cbp;
    if (t8) m->flags |= LH264_MBF_T8x8;
    if (intra) finalize_intra_modes (have_raw ? raw_modes : nullptr, t8, i16mode, chroma_mode);
    int qp = qp_prev;
    if (cbp || i16) {                                     // mb_qp_delta, 9.3.2.7 / 9.3.3.1.1.5
      int v = 0;
      if (cb.decode (60 + (last_dqp != 0 ? 1 : 0))) {
        v = 1;
        if (cb.decode (62)) { v = 2; while (cb.decode (63)) { v++; if (v > 120) { cb.err = true; break; } } }
      }
      const int dqp = (v & 1) ? (v + 1) >> 1 : - (v >> 1);
      if (dqp < -26 || dqp > 25) return false;
      qp = ((qp_prev + dqp) % 52 + 52) % 52;
      last_dqp = dqp;
    } else last_dqp = 0;
    set_qp (qp);
    qp_prev = qp;
    if (!(cbp || i16)) return !cb.err;

    // ---- residual
    int lv[64];
    const int ylist = intra ? 0 : 3;
    if (i16) {
      residual (0, 0, 0, true, lv, 16);
      for (int i = 0; i < 16; i++) if (lv[i]) {
          const int r = T->zigzag4[i], zb = xy2z (r & 3, r >> 2);
          put (coef, zb * 16, lv[i]);                       // dequantised by the DC transform in the reconstruct kernel
        }
    }
    for (int i8 = 0; i8 < 4; i8++) {
      if (!((cbp >> i8) & 1)) continue;
      if (t8) {
        const int tot = residual (5, i8, 0, intra, lv, 64);
        for (int j = 0; j < 4; j++) { const int z = i8 * 4 + j; m->nzc[z2y (z) * 4 + z2x (z)] = (uint8_t)tot; cbf |= 1u << (z2y (z) * 4 + z2x (z)); }
        for (int i = 0; i < 64; i++) if (lv[i]) { const int pos = T->zigzag8[i]; put (coef, i8 * 64 + pos, dq8 (intra ? 0 : 1, qp, pos, lv[i])); }
        continue;
      }
      for (int j = 0; j < 4; j++) {
        const int z = i8 * 4 + j, bx = z2x (z), by = z2y (z);
        const int maxc = i16 ? 15 : 16;
        const int tot = residual (i16 ? 1 : 2, by * 4 + bx, 0, intra, lv, maxc);
        m->nzc[by * 4 + bx] = (uint8_t)tot;
        for (int i = 0; i < maxc; i++) if (lv[i]) { const int pos = T->zigzag4[i16 ? i + 1 : i]; put (coef, z * 16 + pos, dq4 (ylist, qp, pos, lv[i])); }
      }
    }
    const int cbpc = cbp >> 4;
    if (cbpc) {
      for (int p = 0; p < 2; p++) {
        residual (3, 0, p, intra, lv, 4);
        const int qc = m->qp_c[p];
        const int d0 = T->norm4[qc % 6][0] << (qc / 6);
        for (int i = 0; i < 4; i++) if (lv[i]) put (coef, 256 + p * 64 + i * 16, t->use_sl ? (lv[i] * (t->scaling[(ylist + 1 + p) * 16] * d0)) >> 4 : lv[i] * d0);
      }
      if (cbpc == 2) {
        for (int p = 0; p < 2; p++) for (int j = 0; j < 4; j++) {
            const int tot = residual (4, j, p, intra, lv, 15);
            m->nzc[T->chroma_nzc_idx[p][j]] = (uint8_t)tot;
            for (int i = 0; i < 15; i++) if (lv[i]) { const int pos = T->zigzag4[i + 1]; put (coef, 256 + p * 64 + j * 16 + pos, dq4 (ylist + 1 + p, m->qp_c[p], pos, lv[i])); }
          }
      }
    }
    return !cb.err;
  }
};

// a task this walk takes: SliceTask::reserved names CABAC and a cabac_init_idc that is defined
LH264S_HD inline bool cabac_task_ok (const SliceTask& t) { return task_ok (t, true); }

// The slice of one CABAC task: slice_data() as the host's parse_slice_data_cabac walks it.  scratch: a record for the macroblock in hand
// (16-byte aligned); line: kCabacLineBytes per macroblock column (contents do not matter); state: kCabacContexts bytes, initialised for
// the slice (cabac_init_states, or the kernel's lanes).  Statuses as parse_slice has them; stop_bit is the engine's position (see
// DeferredSlice::stop_bit).
LH264S_HD inline SliceResult parse_slice_cabac (const CabacTables& T, const SliceTask& t, lh264_mb_t* scratch, uint8_t* line, uint8_t* state) {
  SliceResult r = {SLICE_BAD_TASK, 0, 0};
  if (!cabac_task_ok (t) || !scratch || !line || !state) return r;
  CabacWalk W;
  W.T = &T; W.t = &t; W.m = scratch; W.line = line;
  W.w = t.mb_w; W.n = t.mb_w * t.mb_h; W.first = t.first_mb; W.k = t.first_mb;
  for (int i = 0; i < 4; i++) { W.left[i] = 2; W.left_mvd[i][0] = W.left_mvd[i][1] = 0; }
  W.left_cbf = 0; W.cbf = 0; W.kA = W.kB = -1;
  CabacEngine& cb = W.cb;
  cb.T = &T; cb.p = t.rbsp; cb.nbytes = t.rbsp_bytes; cb.nbits = t.rbsp_bytes * 8; cb.err = false; cb.state = state;
  cb.win = 0; cb.wbyte = 0; cb.whave = false;
  cb.start ((t.data_bit + 7) & ~7u);                     // cabac_alignment_one_bit
  const int n = W.n, limit = t.limit_mb;
  int qp_prev = t.slice_qp, last_dqp = 0, count = 0, status = SLICE_OK;
  while (W.k < n) {
    if (W.k >= limit) { status = SLICE_OVERRUN; break; }
    bool skip = false;
    if (t.slice_type != 2) {                              // mb_skip_flag, 9.3.3.1.1.1
      const int k = W.k, w = W.w;
      const int kA = ((k % w) && W.avail (k - 1)) ? k - 1 : -1, kB = (k >= w && W.avail (k - w)) ? k - w : -1;
      skip = cb.decode (11 + (kA >= 0 && !CabacWalk::is_skip (t.mbs[kA])) + (kB >= 0 && !CabacWalk::is_skip (t.mbs[kB]))) != 0;
    }
    if (!W.parse_mb (qp_prev, last_dqp, skip)) { status = SLICE_SYNTAX; break; }
    W.done();
    W.k++; count++;
    if (cb.terminate()) break;                            // end_of_slice_flag
    if (cb.err) { status = SLICE_SYNTAX; break; }
  }
  r.status = status; r.n_mbs = count; r.stop_bit = (int32_t)cb.pos;
  if (status == SLICE_OK && t.slice) t.slice->n_mbs = count;
  return r;
}

// the context bytes of a task's slice from the (m, n) table: what the kernel's lanes do together
inline void cabac_init_states (const SliceTask& t, uint8_t* state) {
  const int col = cabac_init_column (t);
  for (int i = 0; i < kCabacContexts; i++) state[i] = cabac_init_state (lh264host::kCabacInit[i][col][0], lh264host::kCabacInit[i][col][1], t.slice_qp);
}

}  // namespace lh264slice
