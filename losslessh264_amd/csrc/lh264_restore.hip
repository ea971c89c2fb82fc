// lh264_restore.hip - the restore direction on the device (include/lh264.h lh264_pip_restore_batch_device):
// one single-wave workgroup per stream runs the adaptive decode of csrc/host/pip_restore.cpp (Restorer::decode_slice,
// decode_coeffs, the scan primitives, update_frame) and its macroblock writers, slice after slice, in the same decision
// order: the CAVLC writer, and in a kernel instance of its own (restore_cabac_kernel, for batches that ask for it) the CABAC writer
// (CabacEnc, write_mb_cabac, cabac_residual), which feeds nothing back into the model.
// The decode is a serial chain (every prior depends on what was decoded before it): lane 0 runs it; the wave clears
// the work memory and runs update_frame's skip-run scan.  What the host keeps in growing containers lives in fixed regions
// the host sized from pass 1 (lh264_restore.h RestoreJob); running out of one, or input the host would refuse, ends the
// stream with a status and the host restores it instead.  Every loop is bounded.
// The code is __host__ __device__ so that the same chain can be stepped on the CPU against the host Restorer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lh264.h"
#include "lh264_restore.h"

#define LH_HD __host__ __device__

namespace lh264r {
namespace {

enum { TAG_SKIP = 1, TAG_SKIP_END = 2, TAG_CBPL = 4, TAG_QPL = 6, TAG_MB_TYPE = 7, TAG_T8 = 8, TAG_REF = 9, TAG_8x8 = 10, TAG_16x16 = 11,
       TAG_PRED_MODE = 13, TAG_SUB_MB = 14, TAG_MVX = 15, TAG_MVY = 16, TAG_LDC = 17, TAG_CRDC = 18, TAG_LAC_0 = 19, TAG_LAC_N = 24,
       TAG_CRAC = 29, TAG_PADBYTE = 69, N_TAGS = 72 };

// ---- DynProb as one word: c0 bits 0-9, c1 bits 10-19, prob bits 20-27.  c0 + c1 <= 513 before the halving, so the word holds
// the counts after it and the prob computed before it: exactly what the host's struct keeps
#define DP_INIT (128u << 20)
// floor (num / den) for num < 2^18, 2 <= den <= 515: the reciprocal's relative error (< 2^-22) moves the product by less than
// 2^-14, so the truncated quotient is off by at most one either way, and one step each way makes it exact
LH_HD inline uint32_t div_prob (uint32_t num, uint32_t den) {
#ifdef __HIP_DEVICE_COMPILE__
  uint32_t q = (uint32_t) ((float)num * __builtin_amdgcn_rcpf ((float)den));
  if (q * den > num) q--;
  else if ((q + 1u) * den <= num) q++;
  return q;
#else
  return num / den;
#endif
}
LH_HD inline uint32_t dp_update (uint32_t c, int bit) {
  uint32_t c0 = c & 1023u, c1 = (c >> 10) & 1023u;
  if (bit) c1++; else c0++;
  const uint32_t prob = div_prob (256u * (c0 + 1u), c0 + c1 + 2u);
  if (c0 + c1 > 512u) { c0 = (c0 + 1u) >> 1; c1 = (c1 + 1u) >> 1; }
  return c0 | (c1 << 10) | (prob << 20);
}

// ---- the bool decoder (pip_restore.cpp BoolReader)
struct Reader { const uint8_t* p; const uint8_t* end; uint64_t value; int32_t count; uint32_t range; int32_t present, pad; };
LH_HD inline void rd_fill (Reader& r) {
  int shift = 64 - 8 - (r.count + 8);
  while (shift >= 0) {                                  // at most 8 bytes
    if (r.p < r.end) { r.count += 8; r.value |= (uint64_t) (*r.p++) << shift; shift -= 8; }
    else { r.count += 0x40000000; break; }              // past the end: zeros
  }
}
LH_HD inline int rd_read (Reader& r, uint32_t prob) {
  const uint32_t split = 1 + (((r.range - 1) * prob) >> 8);
  if (r.count < 0) rd_fill (r);
  const uint64_t bigsplit = (uint64_t)split << 56;
  int bit = 0;
  uint32_t rr = split;
  if (r.value >= bigsplit) { rr = r.range - split; r.value -= bigsplit; bit = 1; }
  const int shift = rr >= 128 ? 0 : __builtin_clz (rr) - 24;
  rr <<= shift;
  r.range = rr; r.value <<= shift; r.count -= shift;
  return bit;
}

struct Cell {                           // pip_restore.cpp Cell
  uint8_t initialized, zeroed, cbp_c, cbp_l, chroma_mode, luma16_mode;
  uint16_t cached_skips;
  uint32_t mb_type, num_ref;
  uint8_t nnz[24];
};
static_assert (sizeof (Cell) == 40, "Cell layout");
struct WState {                         // the CAVLC part of pip_restore.cpp WState
  int32_t slice; uint32_t mb_type; int8_t ipm[16]; uint8_t nzc[24]; uint8_t type_class, pad[3];
};
static_assert (sizeof (WState) == 52, "WState layout");
struct WStateC {                        // pip_restore.cpp WState whole: the CAVLC part where WState has it, then the CABAC context selection (9.3.3.1.1)
  int32_t slice; uint32_t mb_type; int8_t ipm[16]; uint8_t nzc[24]; uint8_t type_class, skip, t8, cbp;
  uint8_t chroma_pred; int8_t ref[4]; uint8_t mvd[16][2]; uint8_t pad[3]; uint32_t cbf;
};
static_assert (sizeof (WStateC) == 96, "WStateC layout");
template <bool kCabac> struct WSel { typedef WState type; };
template <> struct WSel<true> { typedef WStateC type; };
struct alignas (16) MbDec {
  uint32_t type; int cbp_c, cbp_l, luma_qp, num_ref, chroma_mode, luma16_mode, t8;
  int pred_mode[16]; int sub_type[4]; int ref_idx[4]; int mvd[16][2];
  int16_t lev[384];
};

// what the workgroup keeps in LDS
struct Shared {
  RestoreTables T;
  Reader rd[N_TAGS];
  MbDec m;
  uint8_t zero[24];                     // the nnz of an absent neighbour
  uint32_t test_prob;
  int32_t status;
  EscapeCursor esc[2];                  // where the stream stands in its escape entries: [0] SKIPRUN, [1] NUMREF
};
// and what the instance with the CABAC writer keeps there beside it
struct CabacShared {
  RestoreCabacEnc K;
  uint8_t state[460];                   // pStateIdx << 1 | valMPS by context (CabacEnc::state)
};

inline LH_HD int type_code (uint32_t t) {
  switch (t) {
  case LH264_MB_I4x4: return 0;  case LH264_MB_I16x16: return 1;  case LH264_MB_I8x8: return 2;
  case LH264_MB_P16x16: return 3;  case LH264_MB_P16x8: return 4;  case LH264_MB_P8x16: return 5;
  case LH264_MB_P8x8: return 6;  case LH264_MB_P8x8REF0: return 7;  case LH264_MB_IPCM: return 8;
  default: return 11;
  }
}
LH_HD inline uint32_t code_type (unsigned c) {
  switch (c) {
  case 0: return LH264_MB_I4x4;  case 1: return LH264_MB_I16x16;  case 2: return LH264_MB_I8x8;  case 3: return LH264_MB_P16x16;
  case 4: return LH264_MB_P16x8;  case 5: return LH264_MB_P8x16;  case 6: return LH264_MB_P8x8;  case 7: return LH264_MB_P8x8REF0;
  default: return LH264_MB_IPCM;
  }
}
LH_HD inline int min2 (int v) { return v < 2 ? v : 2; }
LH_HD inline int clamp04 (int v) { return v < 0 ? 0 : (v > 4 ? 4 : v); }
LH_HD inline int imin (int a, int b) { return a < b ? a : b; }
LH_HD inline int z2x (int z) { return (z & 1) | ((z >> 2) & 1) << 1; }
LH_HD inline int z2y (int z) { return ((z >> 1) & 1) | ((z >> 3) & 1) << 1; }

// the state of the CABAC encoder (pip_restore.cpp CabacEnc): its bits go out through the chain's bits / nbits, its context states live
// in C.  A base of the chain, empty without the CABAC writer: that chain is then the one the CAVLC kernel has always had
template <bool kCabac> struct EncState {};
template <> struct EncState<true> { CabacShared* C; uint32_t c_low, c_range; int c_out; bool c_first; };

// the serial chain of one stream: lane 0's part of the kernel.  kCabac: with the CABAC writer (and the longer WState it needs)
template <bool kCabac> struct Chain : EncState<kCabac> {
  typedef typename WSel<kCabac>::type W;
  const RestoreJob& J;
  Shared& S;
  const RestoreTables& T;
  Cell* img[2];
  W* ws;
  const uint8_t* pcm; const uint8_t* pcm_end;
  uint32_t used, pool_used;
  int sid;
  // the writer: bytes of the current slice go to J.out[pos...]
  uint32_t pos, bits; int nbits;

  LH_HD Chain (const RestoreJob& j, Shared& s) : J (j), S (s), T (s.T) {}
  LH_HD bool failed() const { return S.status != RS_OK; }
  LH_HD void fail (int st) { if (S.status == RS_OK) S.status = st; }

  // ---- the writer (MainStreamWriter without the escaping, which the host applies when it splices the slice in)
  LH_HD void put_byte (uint32_t b) {
    if (pos < J.out_cap) J.out[pos] = (uint8_t)b;
    else fail (RS_OUT_FULL);
    pos++;
  }
  LH_HD void emit_bits (uint32_t v, int n) {           // n <= 32, MSB first
    const uint64_t acc = ((uint64_t)bits << n) | (n >= 32 ? (uint64_t)v : ((uint64_t)v & ((1ull << n) - 1)));
    int k = nbits + n;
    while (k >= 8) { put_byte ((uint32_t) (acc >> (k - 8)) & 255u); k -= 8; }
    bits = (uint32_t) (acc & ((1ull << k) - 1ull)); nbits = k;
  }
  LH_HD void emit_bit (uint32_t b) { emit_bits (b & 1u, 1); }
  LH_HD void put_ue (uint32_t v) { int n = 0; while (((v + 1) >> n) > 1) n++; emit_bits (0, n); emit_bits (v + 1, n + 1); }
  LH_HD void put_se (int v) { put_ue (v > 0 ? (uint32_t) (2 * v - 1) : (uint32_t) (-2 * v)); }

  // ---- the prior store: open addressing over J.hash, kCell[table] words of J.pool per key.  The first 512 words of the pool are
  // a sink for the decisions after an overflow (the chain stops at its next check, as the host's does after fail())
  LH_HD uint32_t* get (int table, uint32_t index) {
    const uint32_t key = LH264_PRIOR (table, index) + 1u;
    const uint32_t mask = J.slots - 1u;
    uint32_t h = (uint32_t) (((uint64_t)key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++) {
      const uint32_t k = J.hash[2 * h];
      if (k == key) return J.pool + J.hash[2 * h + 1];
      if (k == 0) {
        const uint32_t nc = (uint32_t)T.cell[table];
        if (2u * (used + 1u) > J.slots || pool_used + nc > J.pool_cap) break;
        J.hash[2 * h] = key; J.hash[2 * h + 1] = pool_used;
        uint32_t* c = J.pool + pool_used;
        for (uint32_t i = 0; i < nc; i++) c[i] = DP_INIT;
        pool_used += nc; used++;
        return c;
      }
      h = (h + 1u) & mask;
    }
    fail (RS_STORE_FULL);
    return J.pool;
  }

  // ---- scan primitives
  LH_HD int scan_bit (int tag, uint32_t* p) {
    Reader& r = S.rd[tag];
    if (!r.present) { fail (RS_CORRUPT); return 0; }
    const uint32_t c = *p;
    const int bit = rd_read (r, c >> 20);
    *p = dp_update (c, bit);
    return bit;
  }
  LH_HD int scan_fresh (int tag) {                      // a fresh DynProb (prob 128) whose update nobody keeps
    Reader& r = S.rd[tag];
    if (!r.present) { fail (RS_CORRUPT); return 0; }
    return rd_read (r, 128);
  }
  LH_HD int scan_raw (int tag) { return scan_bit (tag, &S.test_prob); }
  LH_HD unsigned scan_raw_bits (int tag, int n) { unsigned v = 0; for (int i = 0; i < n; i++) v = (v << 1) | (unsigned)scan_raw (tag); return v; }
  LH_HD unsigned scan_tree (int tag, int nbits, uint32_t* arr) {
    unsigned off = 0, v = 0;
    for (int n = nbits; n >= 1; n--) {
      const int bit = scan_bit (tag, arr + off);
      v = (v << 1) | (unsigned)bit;
      off += bit ? 1u + ((1u << (n - 1)) - 1u) : 1u;
    }
    return v;
  }
  LH_HD unsigned scan_pow2 (int tag, int nbits, uint32_t* priors, unsigned preferred) {
    if (!scan_bit (tag, priors)) return preferred;
    const unsigned d = scan_tree (tag, nbits, priors + 1);
    return d >= preferred ? d + 1 : d;
  }
  LH_HD int scan_unary (int tag, uint32_t* pri, int n, int early_termination) {
    int i = 0;
    for (;;) {                                          // at most 70,002 steps
      int bit;
      if (n == 0) bit = scan_fresh (tag);
      else bit = scan_bit (tag, pri + (i < n - 1 ? i : n - 1));
      if (!bit) return i;
      i++;
      if (i == early_termination) return i;
      if (i > 70000 || failed()) { fail (RS_CORRUPT); return 0; }
    }
  }
  struct IntPrior { uint32_t* zero; uint32_t* sign; uint32_t* exponent; int E; uint32_t* mantissa; int M; int order; };
  LH_HD int scan_int (const IntPrior& p, int tag_exp, int tag_man, int tag_zero, int tag_sign) {
    if (p.zero && scan_bit (tag_zero, p.zero)) return 0;
    bool positive = true;
    if (p.sign) positive = scan_bit (tag_sign, p.sign) != 0;
    const int log2 = scan_unary (tag_exp, p.exponent, p.E, -1);
    if (log2 > 30) { fail (RS_CORRUPT); return 0; }
    int lo = 0, hi = p.M;
    uint32_t data_high = 1, low = 0;
    for (int i = 0; i < log2 + p.order; i++) {
      int bit;
      if (hi > lo) {
        const int mid = (hi + lo) / 2;
        bit = scan_bit (tag_man, p.mantissa + mid);
        if (bit) lo = mid + 1; else hi = mid;
      } else bit = scan_raw (tag_man);
      if (i < log2) data_high = (data_high << 1) | (uint32_t)bit; else low = (low << 1) | (uint32_t)bit;
    }
    const int data = (int) (((data_high - 1) << p.order) | low) + 1;
    return positive ? data : -data;
  }
  LH_HD int scan_uegk (uint32_t* cell, int N, int M, int E, int Mant, int order, int tag_exp, int tag_man, int tag_zero, int tag_sign) {
    if (scan_bit (tag_zero, cell + 0)) return 0;
    const int neg = scan_bit (tag_sign, cell + 1);
    int v = scan_unary (tag_man, cell + 2, M, N);
    if (v >= N) {
      IntPrior p; p.zero = cell + 2 + M; p.sign = nullptr; p.exponent = cell + 2 + M + 1; p.E = E; p.mantissa = p.exponent + E; p.M = Mant; p.order = order;
      v = N + scan_int (p, tag_exp, tag_man, tag_zero, tag_sign);
    }
    v += 1;
    return neg ? -v : v;
  }
  LH_HD unsigned tree (int tag, int table, uint32_t index) { return scan_tree (tag, T.tree_bits[table], get (table, index)); }
  // the part of the SKIPRUN (esc 0) / NUMREF (esc 1) symbol just read that its tree drops; 0 for a stream without tag LH264_TAG_ESC
  LH_HD uint32_t escape (int esc) { EscapeCursor& c = S.esc[esc]; return c.rep ? escape_next (c, J.esc[esc], J.n_esc[esc]) : 0u; }

  LH_HD void decode_coeffs (MbDec& m, int st, int mbc, const Cell* nl, const Cell* na, const Cell* np, Cell& e);
  LH_HD int pred_intra_mode (int k, int bx, int by, int w, int sid, bool cip) const;
  LH_HD void write_residual_block (const int* lv, int maxc, int nC, int& total_out);
  LH_HD void write_mb (const RestoreSlice& H, int k, const MbDec& m, int& qp_prev);
  LH_HD void decode_slice (const RestoreSlice& H, int cur_, bool prior_valid, int8_t* ipm, uint8_t* nxn);

  // ---- CABAC arithmetic encoding engine, 9.3.4.2 (this->: the members of EncState, a dependent base)
  LH_HD void ce_reset() { this->c_low = 0; this->c_range = 510; this->c_out = 0; this->c_first = true; }
  LH_HD void ce_write_bit (uint32_t b) { bits = (bits << 1) | (b & 1u); if (++nbits == 8) { put_byte (bits); bits = 0; nbits = 0; } }
  LH_HD void ce_put (uint32_t b) {                      // PutBit, figure 9-9
    if (this->c_first) this->c_first = false; else ce_write_bit (b);
    while (this->c_out > 0) { ce_write_bit (1u - b); this->c_out--; }
  }
  LH_HD void ce_renorm() {
    while (this->c_range < 256) {                             // at most 7 steps
      if (this->c_low < 256) ce_put (0);
      else if (this->c_low >= 512) { this->c_low -= 512; ce_put (1); }
      else { this->c_low -= 256; this->c_out++; }
      this->c_range <<= 1; this->c_low <<= 1;
    }
  }
  LH_HD void ce_encode (int ctx, int bin) {
    const uint32_t s = this->C->state[ctx];
    const uint32_t st = s >> 1; uint32_t mps = s & 1u;
    const uint32_t lps = this->C->K.range_lps[st][(this->c_range >> 6) & 3];
    this->c_range -= lps;
    if ((uint32_t) (bin & 1) != mps) {
      this->c_low += this->c_range; this->c_range = lps;
      if (st == 0) mps ^= 1u;
      this->C->state[ctx] = (uint8_t) ((this->C->K.next_lps[st] << 1) | mps);
    } else this->C->state[ctx] = (uint8_t) ((this->C->K.next_mps[st] << 1) | mps);
    ce_renorm();
  }
  LH_HD void ce_bypass (int bin) {
    this->c_low <<= 1;
    if (bin & 1) this->c_low += this->c_range;
    if (this->c_low >= 1024) { ce_put (1); this->c_low -= 1024; }
    else if (this->c_low < 512) ce_put (0);
    else { this->c_low -= 512; this->c_out++; }
  }
  LH_HD void ce_terminate (int bin) {
    this->c_range -= 2;
    if (bin) {
      this->c_low += this->c_range;
      this->c_range = 2; ce_renorm();                         // EncodeFlush
      ce_put ((this->c_low >> 9) & 1);
      ce_write_bit ((this->c_low >> 8) & 1); ce_write_bit (1);   // the last bit is the rbsp stop bit
      while (nbits) ce_write_bit (0);
    } else ce_renorm();
  }
  LH_HD void ce_ueg_suffix (int rem, int kk) {          // the Exp-Golomb suffix of UEGk, bypass coded; rem < 2^28
    while (kk < 30 && rem >= (1 << kk)) { ce_bypass (1); rem -= 1 << kk; kk++; }
    ce_bypass (0);
    while (kk--) ce_bypass ((rem >> kk) & 1);
  }
  LH_HD void cabac_residual (int w, int k, int cat, int blk, int plane, bool cur_intra, const int* lv, int maxc);
  LH_HD void write_mb_cabac (const RestoreSlice& H, int k, const MbDec* m /* null: P_Skip */, int& qp_prev, int& last_dqp);
};

// pip_restore.cpp Restorer::decode_coeffs
template <bool kCabac> LH_HD void Chain<kCabac>::decode_coeffs (MbDec& m, int st, int mbc, const Cell* nl, const Cell* na, const Cell* np, Cell& e) {
  const uint8_t* Lf = nl ? nl->nnz : S.zero; const uint8_t* Ab = na ? na->nnz : S.zero; const uint8_t* Pa = np ? np->nnz : S.zero;
  uint8_t* C = e.nnz;
  int16_t* lev = m.lev;
  const bool i16 = m.type == LH264_MB_I16x16;
  const bool cdc = m.cbp_c == 1 || m.cbp_c == 2;
  if (i16) for (int i = 0; i < 16; i++) {
      uint32_t* cell = get (LH264_TB_LDC, (uint32_t) ((i * 5 + st) * 16 + mbc));
      IntPrior p; p.exponent = cell; p.E = 3; p.mantissa = cell + 3; p.M = 4; p.zero = cell + 7; p.sign = cell + 8; p.order = 0;
      lev[i * 16] = (int16_t)scan_int (p, TAG_LDC, TAG_LDC, TAG_LDC, TAG_LDC);
    }
  if (cdc) for (int i = 0; i < 8; i++) {
      uint32_t* cell = get (LH264_TB_CDC, (uint32_t) ((i * 5 + st) * 16 + mbc));
      IntPrior p; p.exponent = cell; p.E = 3; p.mantissa = cell + 3; p.M = 4; p.zero = cell + 7; p.sign = cell + 8; p.order = 0;
      lev[256 + i * 16] = (int16_t)scan_int (p, TAG_CRDC, TAG_CRDC, TAG_CRDC, TAG_CRDC);
    }
  for (int b = 0; b < 24; b++) C[b] = (uint8_t) (lev[b * 16] != 0);
  for (int b = 0; b < 24; b++) {
    const bool luma = b < 16;
    const bool big = luma && m.t8;
    bool coded = luma ? ((m.cbp_l >> (b >> 2)) & 1) != 0 : m.cbp_c == 2;
    if (big && (b & 3)) coded = false;
    if (coded && !failed()) {
      const bool emit_dc = luma ? !i16 : !cdc;
      const int start = emit_dc ? 0 : 1, color = luma ? 0 : (b < 20 ? 1 : 2), nco = big ? 64 : 16;
      int past, left, above;
      if (big) {
        const int s = b >> 2;
        past = Pa[b] + Pa[b + 1] + Pa[b + 2] + Pa[b + 3];
        const uint8_t* lp = (s & 1) == 0 ? Lf + (s + 1) * 4 : C + (s - 1) * 4;
        const uint8_t* ap = (s & 2) == 0 ? Ab + (s + 2) * 4 : C + (s - 2) * 4;
        left = lp[0] + lp[1] + lp[2] + lp[3];
        above = ap[0] + ap[1] + ap[2] + ap[3];
      } else if (luma) {
        past = Pa[b];
        left = (b & 3) == 0 ? Lf[b + 3] : C[b - 1];
        above = b < 4 ? Ab[b + 12] : C[b - 4];
      } else {
        const int i = b - 16;
        past = Pa[b];
        left = (i & 1) == 0 ? Lf[b + 1] : C[b - 1];
        above = (i & 2) == 0 ? Ab[b + 2] : C[b - 2];
      }
      int nonzeros;
      {
        uint32_t* cell = get (big ? LH264_TB_NZ8 : LH264_TB_NZ4,
                              (uint32_t) ((((((st * 16 + mbc) * 3 + color) * 3 + min2 (past)) * 3 + min2 (left)) * 3) + min2 (above)));
        IntPrior p; p.exponent = cell; p.E = 3; p.mantissa = cell + 3; p.M = 4; p.zero = cell + 7; p.sign = nullptr; p.order = 0;
        const int t = color ? TAG_CRAC : TAG_LAC_0;
        nonzeros = scan_int (p, t, t, t, t);
      }
      if (nonzeros < 0 || nonzeros > nco - start) { fail (RS_CORRUPT); return; }
      const uint32_t outer0 = (uint32_t) (((st * 16 + mbc) * 3 + color) * nco);
      int left_nz = nonzeros, prev = 0, prev2 = 0, emitted = 0;
      for (int pos = start; pos < nco && left_nz > 0 && !failed(); pos++) {
        const uint32_t inner = (uint32_t) ((((imin (4, left_nz) * 5 + clamp04 (prev + 2)) * 5 + clamp04 (prev2 + 2)) * 5 + 2) * 5 + 2);
        const bool first = color == 0 && emitted == 0 && mbc != 1;
        const int base = color ? TAG_CRAC : (first ? TAG_LAC_0 : TAG_LAC_N);
        const int v = scan_uegk (get (big ? LH264_TB_AC8 : LH264_TB_AC4, (outer0 + (uint32_t)emitted) * 3125u + inner), 14, 4, 2, 4, 0,
                                 base + 2, base + 3, base + 1, base + 4);
        if (v < -32768 || v > 32767) { fail (RS_CORRUPT); return; }
        const int at = big ? T.zz64[pos] : T.zz16[pos];
        lev[b * 16 + at] = (int16_t)v;
        prev2 = prev; prev = v; emitted++;
        if (v) { left_nz--; C[b + (at >> 4)]++; }
      }
    }
  }
}

template <bool kCabac> LH_HD int Chain<kCabac>::pred_intra_mode (int k, int bx, int by, int w, int sid_, bool cip) const {
  int modeA = 2, modeB = 2; bool dcpred = false;
  auto avail = [&] (int kk) { return kk >= 0 && ws[kk].slice == sid_ && (!cip || ws[kk].type_class == 1 || ws[kk].type_class == 2); };
  {
    int kk = k, x = bx - 1, y = by;
    if (x < 0) { kk = (k % w) ? k - 1 : -1; x = 3; }
    if (kk != k && !avail (kk)) dcpred = true;
    else modeA = (kk == k || ws[kk].type_class == 1) ? ws[kk].ipm[y * 4 + x] : 2;
  }
  {
    int kk = k, x = bx, y = by - 1;
    if (y < 0) { kk = k >= w ? k - w : -1; y = 3; }
    if (kk != k && !avail (kk)) dcpred = true;
    else modeB = (kk == k || ws[kk].type_class == 1) ? ws[kk].ipm[y * 4 + x] : 2;
  }
  return dcpred ? 2 : imin (modeA, modeB);
}

// residual_block_cavlc, 7.3.5.3.2 / 9.2 (pip_restore.cpp Restorer::write_residual_block)
template <bool kCabac> LH_HD void Chain<kCabac>::write_residual_block (const int* lv, int maxc, int nC, int& total_out) {
  int coef[16], pos_of[16], total = 0;
  for (int i = maxc - 1; i >= 0; i--) if (lv[i]) { coef[total] = lv[i]; pos_of[total] = i; total++; }
  total_out = total;
  int t1 = 0;
  while (t1 < total && t1 < 3 && (coef[t1] == 1 || coef[t1] == -1)) t1++;
  const int tab = nC < 0 ? 4 : nC < 2 ? 0 : nC < 4 ? 1 : nC < 8 ? 2 : 3;
  if (tab == 3) emit_bits (total == 0 ? 3u : (uint32_t) (((total - 1) << 2) | t1), 6);
  else emit_bits (T.tok_code[tab][total][t1], T.tok_len[tab][total][t1]);
  if (total == 0) return;
  for (int i = 0; i < t1; i++) emit_bit (coef[i] < 0);
  int suffix_len = (total > 10 && t1 < 3) ? 1 : 0;
  for (int i = t1; i < total; i++) {
    const int level = coef[i];
    int code = level > 0 ? 2 * level - 2 : -2 * level - 1;
    if (i == t1 && t1 < 3) code -= 2;
    const int base15 = (15 << suffix_len) + (suffix_len == 0 ? 15 : 0);
    if (suffix_len == 0 && code < 14) { emit_bits (1, code + 1); }
    else if (suffix_len == 0 && code < 30) { emit_bits (1, 15); emit_bits ((uint32_t) (code - 14), 4); }
    else if (suffix_len > 0 && (code >> suffix_len) < 15) { emit_bits (1, (code >> suffix_len) + 1); emit_bits ((uint32_t)code & ((1u << suffix_len) - 1), suffix_len); }
    else {
      const int v = code - base15;
      if (v < 4096) { emit_bits (1, 16); emit_bits ((uint32_t)v, 12); }
      else {                                            // level_prefix >= 16; |level| < 2^15 keeps p below 31
        int p = 16;
        while (p < 31 && v - ((1 << (p - 3)) - 4096) >= (1 << (p - 3))) p++;
        emit_bits (0, p - 16); emit_bits (1, 17);
        emit_bits ((uint32_t) (v - ((1 << (p - 3)) - 4096)), p - 3);
      }
    }
    if (suffix_len == 0) suffix_len = 1;
    const int mag = level < 0 ? -level : level;
    if (mag > (3 << (suffix_len - 1)) && suffix_len < 6) suffix_len++;
  }
  int zeros_left = 0;
  if (total < maxc) {
    zeros_left = pos_of[0] + 1 - total;
    if (nC < 0) { if (total < 4 && zeros_left < 4) emit_bits (T.tzc_code[total][zeros_left], T.tzc_len[total][zeros_left]); }
    else if (zeros_left < 16) emit_bits (T.tz_code[total][zeros_left], T.tz_len[total][zeros_left]);
  }
  for (int i = 0; i < total - 1 && zeros_left > 0; i++) {
    const int run = pos_of[i] - pos_of[i + 1] - 1;
    const int zl = imin (zeros_left, 7);
    if (run < 16) emit_bits (T.rb_code[zl][run], T.rb_len[zl][run]);
    zeros_left -= run;
  }
}

// macroblock_layer, 7.3.5 (pip_restore.cpp Restorer::write_mb)
template <bool kCabac> LH_HD void Chain<kCabac>::write_mb (const RestoreSlice& H, int k, const MbDec& m, int& qp_prev) {
  const int w = H.mb_w;
  const bool is_p = H.slice_type == 0;
  W& s = ws[k];
  s.slice = sid; for (int i = 0; i < 24; i++) s.nzc[i] = 0; for (int i = 0; i < 16; i++) s.ipm[i] = 2;
  const uint32_t type = m.type;
  s.mb_type = type;
  const bool intra = (type & LH264_MB_INTRA) != 0;
  const bool i16 = type == LH264_MB_I16x16;
  const int cbp = m.cbp_l | (m.cbp_c << 4);
  if (type == LH264_MB_IPCM) {
    put_ue (25u + (is_p ? 5u : 0u));
    while (nbits & 7) emit_bit (0);
    for (int i = 0; i < 384; i++) put_byte (pcm[i]);
    pcm += 384;
    s.type_class = 2;
    for (int i = 0; i < 24; i++) s.nzc[i] = 16;
    return;
  }
  if (intra) {
    uint32_t mbt;
    if (i16) {
      const int kRaw16[7] = {0, 1, 2, 3, 2, 2, 2};
      mbt = 1u + (uint32_t)kRaw16[imin (m.luma16_mode, 6)] + 4u * (uint32_t)m.cbp_c + (m.cbp_l ? 12u : 0u);
      s.type_class = 2;
    } else { mbt = 0; s.type_class = 1; }
    put_ue (mbt + (is_p ? 5u : 0u));
    if (!i16) {
      const bool t8 = type == LH264_MB_I8x8;
      if (H.transform_8x8) emit_bit (t8);
      const int nblk = t8 ? 4 : 16;
      for (int i = 0; i < nblk; i++) {
        const int bx = t8 ? (i & 1) * 2 : z2x (i), by = t8 ? (i >> 1) * 2 : z2y (i);
        const int pred = pred_intra_mode (k, bx, by, w, sid, H.constrained_intra_pred);
        const int mode = m.pred_mode[i];
        if (mode == pred) emit_bit (1);
        else { emit_bit (0); emit_bits ((uint32_t) (mode < pred ? mode : mode - 1), 3); }
        const int n = t8 ? 2 : 1;
        for (int yy = 0; yy < n; yy++) for (int x = 0; x < n; x++) s.ipm[(by + yy) * 4 + bx + x] = (int8_t)mode;
      }
    }
    const int kRawChroma[7] = {0, 1, 2, 3, 0, 0, 0};
    put_ue ((uint32_t)kRawChroma[imin (m.chroma_mode, 6)]);
    if (!i16) put_ue (T.cbp_code[0][cbp]);
  } else {
    s.type_class = 3;
    const int nref = H.num_ref_idx_l0;
    auto put_ref = [&] (int r) { if (nref <= 1) return; if (nref == 2) emit_bit (r ? 0 : 1); else put_ue ((uint32_t)r); };
    auto put_mvd = [&] (int blk) { put_se (m.mvd[blk][0]); put_se (m.mvd[blk][1]); };
    if (type == LH264_MB_P16x16) { put_ue (0); put_ref (m.ref_idx[0]); put_mvd (0); }
    else if (type == LH264_MB_P16x8) { put_ue (1); put_ref (m.ref_idx[0]); put_ref (m.ref_idx[1]); put_mvd (0); put_mvd (8); }
    else if (type == LH264_MB_P8x16) { put_ue (2); put_ref (m.ref_idx[0]); put_ref (m.ref_idx[1]); put_mvd (0); put_mvd (2); }
    else {
      put_ue (type == LH264_MB_P8x8 ? 3 : 4);
      for (int q = 0; q < 4; q++) put_ue (m.sub_type[q] == LH264_SUB_8x8 ? 0u : m.sub_type[q] == LH264_SUB_8x4 ? 1u : m.sub_type[q] == LH264_SUB_4x8 ? 2u : 3u);
      if (type == LH264_MB_P8x8) for (int q = 0; q < 4; q++) put_ref (m.ref_idx[q]);
      for (int q = 0; q < 4; q++) {
        switch (m.sub_type[q]) {
        case LH264_SUB_8x8: put_mvd (T.z2raster[q << 2]); break;
        case LH264_SUB_8x4: for (int j = 0; j < 2; j++) put_mvd (T.z2raster[(q << 2) + (j << 1)]); break;
        case LH264_SUB_4x8: for (int j = 0; j < 2; j++) put_mvd (T.z2raster[(q << 2) + j]); break;
        default: for (int j = 0; j < 4; j++) put_mvd (T.z2raster[(q << 2) + j]); break;
        }
      }
    }
    put_ue (T.cbp_code[1][cbp]);
    bool no_sub_lt8 = true;
    if (type == LH264_MB_P8x8 || type == LH264_MB_P8x8REF0) for (int q = 0; q < 4; q++) if (m.sub_type[q] != LH264_SUB_8x8) no_sub_lt8 = false;
    if (m.cbp_l && H.transform_8x8 && no_sub_lt8) emit_bit (m.t8);
  }
  if (!(cbp || i16)) return;
  {
    const int d = (((m.luma_qp - qp_prev) + 26 + 104) % 52) - 26;
    put_se (d);
    qp_prev = m.luma_qp;
  }
  int lv[16], tot;
  auto luma_nC = [&] (int bx, int by) {
    int nA = 0, nB = 0; bool aA = true, aB = true;
    if (bx == 0) { const int kk = (k % w) ? k - 1 : -1; aA = kk >= 0 && ws[kk].slice == sid; if (aA) nA = ws[kk].nzc[by * 4 + 3]; } else nA = s.nzc[by * 4 + bx - 1];
    if (by == 0) { const int kk = k >= w ? k - w : -1; aB = kk >= 0 && ws[kk].slice == sid; if (aB) nB = ws[kk].nzc[12 + bx]; } else nB = s.nzc[(by - 1) * 4 + bx];
    return (aA && aB) ? (nA + nB + 1) >> 1 : aA ? nA : aB ? nB : 0;
  };
  if (i16) {
    for (int i = 0; i < 16; i++) { const int r = T.zz4[i]; lv[i] = m.lev[(((r & 3) & 1) | (((r >> 2) & 1) << 1) | (((r & 3) >> 1) << 2) | (((r >> 2) >> 1) << 3)) * 16]; }
    write_residual_block (lv, 16, luma_nC (0, 0), tot);
  }
  for (int i8 = 0; i8 < 4; i8++) {
    if (!((m.cbp_l >> i8) & 1)) continue;
    for (int j = 0; j < 4; j++) {
      const int z = i8 * 4 + j, bx = z2x (z), by = z2y (z);
      const int maxc = i16 ? 15 : 16;
      for (int i = 0; i < maxc; i++) lv[i] = m.t8 ? m.lev[i8 * 64 + T.zz8[4 * i + j]] : m.lev[z * 16 + T.zz4[i16 ? i + 1 : i]];
      write_residual_block (lv, maxc, luma_nC (bx, by), tot);
      s.nzc[by * 4 + bx] = (uint8_t)tot;
    }
  }
  if (m.cbp_c) {
    for (int p = 0; p < 2; p++) {
      for (int i = 0; i < 4; i++) lv[i] = m.lev[256 + p * 64 + i * 16];
      write_residual_block (lv, 4, -1, tot);
    }
    if (m.cbp_c == 2) {
      for (int p = 0; p < 2; p++) for (int j = 0; j < 4; j++) {
          const int bx = j & 1, by = j >> 1;
          int nA = 0, nB = 0; bool aA = true, aB = true;
          if (bx == 0) { const int kk = (k % w) ? k - 1 : -1; aA = kk >= 0 && ws[kk].slice == sid; if (aA) nA = ws[kk].nzc[T.chroma_nzc[p][by * 2 + 1]]; } else nA = s.nzc[T.chroma_nzc[p][by * 2]];
          if (by == 0) { const int kk = k >= w ? k - w : -1; aB = kk >= 0 && ws[kk].slice == sid; if (aB) nB = ws[kk].nzc[T.chroma_nzc[p][2 + bx]]; } else nB = s.nzc[T.chroma_nzc[p][bx]];
          const int nC = (aA && aB) ? (nA + nB + 1) >> 1 : aA ? nA : aB ? nB : 0;
          for (int i = 0; i < 15; i++) lv[i] = m.lev[256 + p * 64 + j * 16 + T.zz4[i + 1]];
          write_residual_block (lv, 15, nC, tot);
          s.nzc[T.chroma_nzc[p][j]] = (uint8_t)tot;
        }
    }
  }
}

// ---- the CABAC macroblock layer writer: 7.3.5 with the binarisations and context selection of 9.3.2 / 9.3.3 (pip_restore.cpp
// Restorer::cabac_residual, Restorer::write_mb_cabac), instantiated in the kCabac chain only
template <bool kCabac> LH_HD void Chain<kCabac>::cabac_residual (int w, int k, int cat, int blk, int plane, bool cur_intra, const int* lv, int maxc) {
  const RestoreCabacEnc& K = this->C->K;
  W& s = ws[k];
  int last_nz = -1, n_sig = 0;
  for (int i = 0; i < maxc; i++) if (lv[i]) { last_nz = i; n_sig++; }
  if (cat != 5) {                                          // coded_block_flag, 9.3.3.1.1.9
    int bit, bitA, bitB; int kA = k, kB = k;
    if (cat == 0) { bit = bitA = bitB = 16; kA = -2; kB = -2; }
    else if (cat == 3) { bit = bitA = bitB = 17 + plane; kA = -2; kB = -2; }
    else if (cat == 4) {
      const int cx = blk & 1, cy = blk >> 1;
      bit = 19 + plane * 4 + blk;
      if (cx == 0) { kA = -2; bitA = 19 + plane * 4 + cy * 2 + 1; } else bitA = bit - 1;
      if (cy == 0) { kB = -2; bitB = 19 + plane * 4 + 2 + cx; } else bitB = bit - 2;
    } else {
      const int bx = blk & 3, by = blk >> 2;
      bit = blk;
      if (bx == 0) { kA = -2; bitA = by * 4 + 3; } else bitA = blk - 1;
      if (by == 0) { kB = -2; bitB = 12 + bx; } else bitB = blk - 4;
    }
    if (kA == -2) kA = ((k % w) && ws[k - 1].slice == sid) ? k - 1 : -1;
    if (kB == -2) kB = (k >= w && ws[k - w].slice == sid) ? k - w : -1;
    const int cA = kA < 0 ? (cur_intra ? 1 : 0) : (int) ((ws[kA].cbf >> bitA) & 1);
    const int cBf = kB < 0 ? (cur_intra ? 1 : 0) : (int) ((ws[kB].cbf >> bitB) & 1);
    ce_encode (85 + K.cat_cbf[cat] + cA + 2 * cBf, n_sig != 0);
    if (!n_sig) return;
    s.cbf |= 1u << bit;
  }
  const int sig_base = cat == 5 ? 402 : 105 + K.cat_map[cat], last_base = cat == 5 ? 417 : 166 + K.cat_map[cat];
  const int abs_base = cat == 5 ? 426 : 227 + K.cat_abs[cat];
  for (int i = 0; i < maxc - 1; i++) {
    const int inc_s = cat == 5 ? K.sig8x8[i] : cat == 3 ? imin (i, 2) : i;
    const int inc_l = cat == 5 ? K.last8x8[i] : cat == 3 ? imin (i, 2) : i;
    const int sig = lv[i] != 0;
    ce_encode (sig_base + inc_s, sig);
    if (sig) {
      ce_encode (last_base + inc_l, i == last_nz);
      if (i == last_nz) break;
    }
  }
  int num_eq1 = 0, num_gt1 = 0;
  for (int i = maxc - 1; i >= 0; i--) {
    if (!lv[i]) continue;
    const int mag = lv[i] < 0 ? -lv[i] : lv[i], v = mag - 1;
    int inc = num_gt1 ? 0 : imin (4, 1 + num_eq1);
    ce_encode (abs_base + inc, v > 0);
    if (v > 0) {
      inc = 5 + imin (4 - (cat == 3 ? 1 : 0), num_gt1);
      int cnt = 1;
      while (cnt < 14) { const int bin = v > cnt; ce_encode (abs_base + inc, bin); if (!bin) break; cnt++; }
      if (v >= 14) ce_ueg_suffix (v - 14, 0);               // Exp-Golomb order 0 suffix
    }
    ce_bypass (lv[i] < 0);
    if (mag == 1) num_eq1++; else num_gt1++;
  }
}

template <bool kCabac> LH_HD void Chain<kCabac>::write_mb_cabac (const RestoreSlice& H, int k, const MbDec* mp, int& qp_prev, int& last_dqp) {
  const int w = H.mb_w;
  const bool is_p = H.slice_type == 0;
  W& s = ws[k];
  const int kA = ((k % w) && ws[k - 1].slice == sid) ? k - 1 : -1, kB = (k >= w && ws[k - w].slice == sid) ? k - w : -1;
  if (is_p) ce_encode (11 + (kA >= 0 && !ws[kA].skip) + (kB >= 0 && !ws[kB].skip), mp == nullptr);     // mb_skip_flag
  s.slice = sid; for (int i = 0; i < 24; i++) s.nzc[i] = 0; for (int i = 0; i < 16; i++) { s.ipm[i] = 2; s.mvd[i][0] = s.mvd[i][1] = 0; }
  s.skip = 0; s.t8 = 0; s.cbp = 0; s.chroma_pred = 0; s.cbf = 0;
  for (int i = 0; i < 4; i++) s.ref[i] = -1;
  if (!mp) {
    s.mb_type = LH264_MB_SKIP; s.type_class = 3; s.skip = 1;
    for (int i = 0; i < 4; i++) s.ref[i] = 0;
    last_dqp = 0;
    return;
  }
  const MbDec& m = *mp;
  const uint32_t type = m.type;
  s.mb_type = type;
  const bool intra = (type & LH264_MB_INTRA) != 0;
  const bool i16 = type == LH264_MB_I16x16;
  const int cbp = m.cbp_l | (m.cbp_c << 4);
  auto i_type = [&] (bool islice, int mbt) {               // 9.3.2.5, Table 9-36
    const int ctx0 = islice ? 3 + (kA >= 0 && ws[kA].type_class != 1) + (kB >= 0 && ws[kB].type_class != 1) : 17;
    if (mbt == 0) { ce_encode (ctx0, 0); return; }
    ce_encode (ctx0, 1);
    ce_terminate (0);
    const int v = mbt - 1, pm = v & 3, chroma = (v >> 2) % 3, luma = v >= 12;
    const int base = islice ? 3 : 17;
    ce_encode (base + (islice ? 3 : 1), luma);
    ce_encode (base + (islice ? 4 : 2), chroma != 0);
    if (chroma) ce_encode (base + (islice ? 5 : 2), chroma == 2);
    ce_encode (base + (islice ? 6 : 3), pm >> 1);
    ce_encode (base + (islice ? 7 : 3), pm & 1);
  };
  auto t8_flag = [&] (int v) { ce_encode (399 + (kA >= 0 && ws[kA].t8) + (kB >= 0 && ws[kB].t8), v); };
  bool t8 = false;
  if (type == LH264_MB_IPCM) {
    // mb_type 25: the prefix bin, then the terminating bin set, which flushes the engine (9.3.4.5) and leaves the stream byte aligned;
    // the samples follow as they are and the engine starts afresh behind them, the context states kept (9.3.1.2)
    if (is_p) ce_encode (14, 1);
    ce_encode (is_p ? 17 : 3 + (kA >= 0 && ws[kA].type_class != 1) + (kB >= 0 && ws[kB].type_class != 1), 1);
    ce_terminate (1);
    for (int i = 0; i < 384; i++) put_byte (pcm[i]);
    pcm += 384;
    ce_reset();
    s.type_class = 2; s.cbf = 0xffffffffu; s.cbp = 0x2f;
    for (int i = 0; i < 24; i++) s.nzc[i] = 16;
    last_dqp = 0;
    return;
  }
  if (intra) {
    int mbt = 0;
    if (i16) {
      const int kRaw16[7] = {0, 1, 2, 3, 2, 2, 2};
      mbt = 1 + kRaw16[imin (m.luma16_mode, 6)] + 4 * m.cbp_c + (m.cbp_l ? 12 : 0);
      s.type_class = 2;
    } else s.type_class = 1;
    if (is_p) ce_encode (14, 1);
    i_type (!is_p, mbt);
    if (!i16) {
      t8 = type == LH264_MB_I8x8;
      if (H.transform_8x8) t8_flag (t8);
      s.t8 = t8;
      const int nblk = t8 ? 4 : 16;
      for (int i = 0; i < nblk; i++) {
        const int bx = t8 ? (i & 1) * 2 : z2x (i), by = t8 ? (i >> 1) * 2 : z2y (i);
        const int pred = pred_intra_mode (k, bx, by, w, sid, H.constrained_intra_pred);
        const int mode = m.pred_mode[i];
        ce_encode (68, mode == pred);
        if (mode != pred) { const int rem = mode < pred ? mode : mode - 1; ce_encode (69, rem & 1); ce_encode (69, (rem >> 1) & 1); ce_encode (69, (rem >> 2) & 1); }
        const int n = t8 ? 2 : 1;
        for (int yy = 0; yy < n; yy++) for (int x = 0; x < n; x++) s.ipm[(by + yy) * 4 + bx + x] = (int8_t)mode;
      }
    }
    const int kRawChroma[7] = {0, 1, 2, 3, 0, 0, 0};
    const int cm = kRawChroma[imin (m.chroma_mode, 6)];
    {                                                        // intra_chroma_pred_mode, 9.3.3.1.1.8
      const int cA = kA >= 0 && ws[kA].type_class != 3 && ws[kA].chroma_pred != 0;
      const int cBn = kB >= 0 && ws[kB].type_class != 3 && ws[kB].chroma_pred != 0;
      ce_encode (64 + cA + cBn, cm != 0);
      if (cm) { ce_encode (67, cm != 1); if (cm != 1) ce_encode (67, cm == 3); }
    }
    s.chroma_pred = (uint8_t)cm;
  } else {
    s.type_class = 3;
    const int nref = H.num_ref_idx_l0;
    ce_encode (14, 0);
    if (type == LH264_MB_P16x16) { ce_encode (15, 0); ce_encode (16, 0); }
    else if (type == LH264_MB_P8x8 || type == LH264_MB_P8x8REF0) { ce_encode (15, 0); ce_encode (16, 1); }
    else if (type == LH264_MB_P16x8) { ce_encode (15, 1); ce_encode (17, 1); }
    else { ce_encode (15, 1); ce_encode (17, 0); }
    auto ref_gt0 = [&] (int bx, int by) -> int {
      int kk = k, x = bx, yy = by;
      if (x < 0) { kk = kA; x = 3; } else if (yy < 0) { kk = kB; yy = 3; }
      if (kk < 0) return 0;
      const W& t = ws[kk];
      if (t.type_class != 3 || t.skip) return 0;
      return t.ref[(yy >> 1) * 2 + (x >> 1)] > 0;
    };
    auto put_ref = [&] (int bx, int by, int v) {
      if (nref <= 1) return;
      int inc = ref_gt0 (bx - 1, by) + 2 * ref_gt0 (bx, by - 1);
      for (int i = 0; i < v; i++) { ce_encode (54 + inc, 1); inc = i == 0 ? 4 : 5; }
      ce_encode (54 + inc, 0);
    };
    auto abs_mvd = [&] (int bx, int by, int comp) -> int {
      int kk = k, x = bx, yy = by;
      if (x < 0) { kk = kA; x = 3; } else if (yy < 0) { kk = kB; yy = 3; }
      if (kk < 0) return 0;
      return ws[kk].mvd[yy * 4 + x][comp];
    };
    auto put_mvd1 = [&] (int bx, int by, int comp, int d) {     // UEG3, uCoff 9, signed (9.3.2.3, 9.3.3.1.1.7)
      const int base = comp ? 47 : 40;
      const int sum = abs_mvd (bx - 1, by, comp) + abs_mvd (bx, by - 1, comp);
      int inc = sum < 3 ? 0 : sum > 32 ? 2 : 1;
      const int a = d < 0 ? -d : d;
      if (a < 0 || a >= (1 << 28)) { fail (RS_CORRUPT); return; }     // no stream codes one; the suffix loop stays in range
      ce_encode (base + inc, a != 0);
      if (!a) return;
      int v = 1;
      inc = 3;
      while (v < 9) { const int bin = a > v; ce_encode (base + inc, bin); if (!bin) break; v++; if (inc < 6) inc++; }
      if (a >= 9) ce_ueg_suffix (a - 9, 3);
      ce_bypass (d < 0);
    };
    auto part = [&] (int bx, int by, int bw, int bh) {          // the partition whose motion vector difference sits at (bx,by)
      const int dx = m.mvd[by * 4 + bx][0], dy = m.mvd[by * 4 + bx][1];
      put_mvd1 (bx, by, 0, dx); put_mvd1 (bx, by, 1, dy);
      const uint8_t ax = (uint8_t)imin (255, dx < 0 ? -dx : dx), ay = (uint8_t)imin (255, dy < 0 ? -dy : dy);
      for (int yy = by; yy < by + bh; yy++) for (int x = bx; x < bx + bw; x++) { s.mvd[yy * 4 + x][0] = ax; s.mvd[yy * 4 + x][1] = ay; }
    };
    if (type == LH264_MB_P16x16 || type == LH264_MB_P16x8 || type == LH264_MB_P8x16) {
      const int mbt = type == LH264_MB_P16x16 ? 0 : type == LH264_MB_P16x8 ? 1 : 2;
      const int np = mbt == 0 ? 1 : 2;
      for (int i = 0; i < np; i++) {
        const int bx = mbt == 2 ? i * 2 : 0, by = mbt == 1 ? i * 2 : 0;
        put_ref (bx, by, m.ref_idx[i]);
        for (int q = 0; q < 4; q++) {
          const bool in = mbt == 0 || (mbt == 1 ? (q >> 1) == i : (q & 1) == i);
          if (in) s.ref[q] = (int8_t)m.ref_idx[i];
        }
      }
      for (int i = 0; i < np; i++) {
        int bx = 0, by = 0, bw = 4, bh = 4;
        if (mbt == 1) { bh = 2; by = i * 2; } else if (mbt == 2) { bw = 2; bx = i * 2; }
        part (bx, by, bw, bh);
      }
    } else {
      int sub[4];
      for (int q = 0; q < 4; q++) {                           // sub_mb_type, Table 9-37
        sub[q] = m.sub_type[q] == LH264_SUB_8x8 ? 0 : m.sub_type[q] == LH264_SUB_8x4 ? 1 : m.sub_type[q] == LH264_SUB_4x8 ? 2 : 3;
        if (sub[q] == 0) ce_encode (21, 1);
        else { ce_encode (21, 0); if (sub[q] == 1) ce_encode (22, 0); else { ce_encode (22, 1); ce_encode (23, sub[q] == 2); } }
      }
      for (int q = 0; q < 4; q++) { put_ref ((q & 1) * 2, (q >> 1) * 2, m.ref_idx[q]); s.ref[q] = (int8_t)m.ref_idx[q]; }
      for (int q = 0; q < 4; q++) {
        const int qx = (q & 1) * 2, qy = (q >> 1) * 2;
        const int nsp = sub[q] == 0 ? 1 : sub[q] == 3 ? 4 : 2;
        for (int j = 0; j < nsp; j++) {
          int bx = qx, by = qy, bw = 2, bh = 2;
          if (sub[q] == 1) { bh = 1; by += j; } else if (sub[q] == 2) { bw = 1; bx += j; } else if (sub[q] == 3) { bw = bh = 1; bx += j & 1; by += j >> 1; }
          part (bx, by, bw, bh);
        }
      }
    }
  }
  if (!i16) {                                                // coded_block_pattern, 9.3.2.6 / 9.3.3.1.1.4
    auto luma_bit = [&] (int kk, int b8) -> int {
      if (kk < 0) return 0;
      if (ws[kk].skip) return 1;
      return ((ws[kk].cbp >> b8) & 1) ? 0 : 1;
    };
    int cl = 0;
    for (int b8 = 0; b8 < 4; b8++) {
      const int cA = (b8 & 1) ? (((cl >> (b8 - 1)) & 1) ? 0 : 1) : luma_bit (kA, b8 + 1);
      const int cBn = (b8 & 2) ? (((cl >> (b8 - 2)) & 1) ? 0 : 1) : luma_bit (kB, b8 + 2);
      const int bit = (m.cbp_l >> b8) & 1;
      ce_encode (73 + cA + 2 * cBn, bit);
      cl |= bit << b8;
    }
    auto chroma_nz = [&] (int kk, int lvl) -> int {
      if (kk < 0) return 0;
      if (ws[kk].skip) return 0;
      return (ws[kk].cbp >> 4) >= lvl;
    };
    ce_encode (77 + chroma_nz (kA, 1) + 2 * chroma_nz (kB, 1), m.cbp_c != 0);
    if (m.cbp_c) ce_encode (77 + 4 + chroma_nz (kA, 2) + 2 * chroma_nz (kB, 2), m.cbp_c == 2);
    if (!intra) {
      bool no_sub_lt8 = true;
      if (type == LH264_MB_P8x8 || type == LH264_MB_P8x8REF0) for (int q = 0; q < 4; q++) if (m.sub_type[q] != LH264_SUB_8x8) no_sub_lt8 = false;
      if (m.cbp_l && H.transform_8x8 && no_sub_lt8) { t8 = m.t8 != 0; t8_flag (t8); }
    }
  }
  s.cbp = (uint8_t)cbp;
  if (t8) s.t8 = 1;
  if (!(cbp || i16)) { last_dqp = 0; return; }
  {                                                          // mb_qp_delta, 9.3.2.7 / 9.3.3.1.1.5
    const int d = (((m.luma_qp - qp_prev) + 26 + 104) % 52) - 26;
    const int v = d > 0 ? 2 * d - 1 : -2 * d;
    ce_encode (60 + (last_dqp != 0 ? 1 : 0), v != 0);
    if (v) {
      ce_encode (62, v >= 2);
      if (v >= 2) { for (int j = 2; j < v; j++) ce_encode (63, 1); ce_encode (63, 0); }
    }
    last_dqp = d;
    qp_prev = m.luma_qp;
  }
  int lv[64];
  if (i16) {
    for (int i = 0; i < 16; i++) { const int r = T.zz4[i]; lv[i] = m.lev[(((r & 3) & 1) | (((r >> 2) & 1) << 1) | (((r & 3) >> 1) << 2) | (((r >> 2) >> 1) << 3)) * 16]; }
    cabac_residual (w, k, 0, 0, 0, true, lv, 16);
  }
  for (int i8 = 0; i8 < 4; i8++) {
    if (!((m.cbp_l >> i8) & 1)) continue;
    if (t8) {
      for (int i = 0; i < 64; i++) lv[i] = m.lev[i8 * 64 + T.zz8[i]];
      cabac_residual (w, k, 5, i8, 0, intra, lv, 64);
      for (int j = 0; j < 4; j++) { const int z = i8 * 4 + j; s.cbf |= 1u << (z2y (z) * 4 + z2x (z)); }
      continue;
    }
    for (int j = 0; j < 4; j++) {
      const int z = i8 * 4 + j, bx = z2x (z), by = z2y (z);
      const int maxc = i16 ? 15 : 16;
      for (int i = 0; i < maxc; i++) lv[i] = m.lev[z * 16 + T.zz4[i16 ? i + 1 : i]];
      cabac_residual (w, k, i16 ? 1 : 2, by * 4 + bx, 0, intra, lv, maxc);
    }
  }
  if (m.cbp_c) {
    for (int p = 0; p < 2; p++) {
      for (int i = 0; i < 4; i++) lv[i] = m.lev[256 + p * 64 + i * 16];
      cabac_residual (w, k, 3, 0, p, intra, lv, 4);
    }
    if (m.cbp_c == 2) {
      for (int p = 0; p < 2; p++) for (int j = 0; j < 4; j++) {
          for (int i = 0; i < 15; i++) lv[i] = m.lev[256 + p * 64 + j * 16 + T.zz4[i + 1]];
          cabac_residual (w, k, 4, j, p, intra, lv, 15);
        }
    }
  }
}

// one slice (pip_restore.cpp Restorer::decode_slice after its bookkeeping, which the whole wave did)
template <bool kCabac> LH_HD void Chain<kCabac>::decode_slice (const RestoreSlice& H, int cur_, bool prior_valid, int8_t* ipm_, uint8_t* nxn_) {
  const int w = H.mb_w, n = H.mb_w * H.mb_h;
  Cell* cur = img[cur_];
  Cell* last = img[1 - cur_];
  const bool is_p = H.slice_type == 0;
  const int st = H.slice_type;
  const bool cabac = kCabac && H.cabac;
  const uint32_t pos0 = pos;
  int skip_state = -1, mb_in_slice = 0, cached_qp = 0, last_nonzero_dqp = 0, qp_prev = H.slice_qp, last_dqp = 0;
  uint32_t pending_skips = 0;
  MbDec& m = S.m;
  for (int k = H.first_mb; ; k++, mb_in_slice++) {      // ends at the stop flag; k < n bounds it
    if (k >= n) { fail (RS_CORRUPT); return; }
    if (failed()) return;
    const int x = k % w;
    const Cell* nl = (x > 0 && cur[k - 1].initialized) ? &cur[k - 1] : nullptr;
    const Cell* na = (k >= w && cur[k - w].initialized) ? &cur[k - w] : nullptr;
    const Cell* np = (prior_valid && last[k].initialized) ? &last[k] : nullptr;
    int mb_skip_run = 0;
    const uint32_t stop_idx = (uint32_t) (mb_in_slice < 2048 ? mb_in_slice : 2047);
    if (skip_state == -1 || cabac) {                    // CABAC: a run of 0 or 1 for every macroblock
      const int pr = np ? np->cached_skips / 8 + (np->cached_skips % 8 ? 1 : 0) : 0;
      int run = (int)tree (TAG_SKIP, LH264_TB_SKIPRUN, (uint32_t) (pr * 16 + 11));
      if (const uint32_t high = escape (0)) {
        if (high > kEscapeHighMax) { fail (RS_CORRUPT); return; }
        run |= (int) (high << T.tree_bits[LH264_TB_SKIPRUN]);
      }
      if (is_p && !cabac) skip_state = run; else mb_skip_run = run;
      if (cabac && run > 1) { fail (RS_CORRUPT); return; }
    }
    if (is_p && !cabac) { mb_skip_run = skip_state; skip_state--; }
    bool has_stop = false;
    if (mb_skip_run == 1) has_stop = scan_bit (TAG_SKIP_END, get (LH264_TB_STOP, stop_idx)) != 0;
    if (mb_skip_run != 0) {
      if (!is_p) { fail (RS_CORRUPT); return; }
      cur[k] = last[k];
      nxn_[k] = 0;
      W& s = ws[k];
      s.slice = sid; s.mb_type = LH264_MB_SKIP; s.type_class = 3; for (int i = 0; i < 24; i++) s.nzc[i] = 0; for (int i = 0; i < 16; i++) s.ipm[i] = 2;
      if constexpr (kCabac) {
        if (cabac) { write_mb_cabac (H, k, nullptr, qp_prev, last_dqp); ce_terminate (has_stop); }
        else pending_skips++;
      } else pending_skips++;
      if (has_stop) break;
      continue;
    }
    has_stop = scan_bit (TAG_SKIP_END, get (LH264_TB_STOP, stop_idx)) != 0;
    {
      uint4* z = (uint4*)&m;                            // memset (&m, 0, sizeof (m))
      for (unsigned i = 0; i < sizeof (MbDec) / 16; i++) z[i] = uint4{0, 0, 0, 0};
    }
    {
      int prior = 15, prev = 15;
      if (na) prior = type_code (na->mb_type);
      if (nl) prior = type_code (nl->mb_type);
      if (np) prev = type_code (np->mb_type);
      const unsigned code = tree (TAG_MB_TYPE, LH264_TB_MBTYPE, (uint32_t) ((prior + prev) * 2 + (is_p ? 1 : 0)));
      if (code > 8) { fail (RS_CORRUPT); return; }
      if (code == 8 && pcm_end - pcm < 384) { fail (RS_CORRUPT); return; }
      m.type = code_type (code);
    }
    const uint32_t type = m.type;
    const int mbc = type_code (type);
    if (!is_p && !(type & LH264_MB_INTRA)) { fail (RS_CORRUPT); return; }
    m.cbp_c = (int)tree (TAG_CBPL, LH264_TB_CBPC, (uint32_t) ((np ? np->cbp_c : 0) * 16 + mbc));
    m.cbp_l = (int)tree (TAG_CBPL, LH264_TB_CBPL, (uint32_t) ((np ? np->cbp_l : 0) * 16 + mbc));
    if (m.cbp_c > 2) { fail (RS_CORRUPT); return; }
    {
      const int sidx = last_nonzero_dqp < 0 ? 0 : (last_nonzero_dqp == 0 ? 1 : 2);
      const unsigned sw = scan_pow2 (TAG_QPL, 7, get (LH264_TB_QPL, (uint32_t) ((mb_in_slice == 0 ? 1 : 0) * 3 + sidx)), 0);
      const int dqp = (sw & 1) ? - (int) (sw >> 1) - 1 : (int) (sw >> 1);
      m.luma_qp = (cached_qp + dqp) & 0xff;
      cached_qp = m.luma_qp;
      if (dqp) last_nonzero_dqp = dqp;
      if (m.luma_qp > 51) { fail (RS_CORRUPT); return; }
    }
    m.num_ref = (int)tree (TAG_REF, LH264_TB_NUMREF, (uint32_t) ((np ? np->num_ref : 0) * 16 + mbc));
    if (const uint32_t high = escape (1)) {
      if (high > 1 || m.num_ref) { fail (RS_CORRUPT); return; }
      m.num_ref = 16;
    }
    int ref_bits = 0;
    while (ref_bits < 31 && (1 << ref_bits) < m.num_ref) ref_bits++;
    {
      int pr = 7;
      if (np) { pr = np->chroma_mode; if (pr >= 6) pr = 6; }
      m.chroma_mode = (int)scan_pow2 (TAG_8x8, 3, get (LH264_TB_MODE8, (uint32_t)pr), (unsigned)pr);
      pr = 7;
      if (np) { pr = np->luma16_mode; if (pr >= 6) pr = 6; }
      m.luma16_mode = (int)scan_pow2 (TAG_16x16, 3, get (LH264_TB_MODE8, (uint32_t)pr), (unsigned)pr);
    }
    int8_t* my_ipm = &ipm_[(size_t)k * 8];
    if (type == LH264_MB_I4x4 || type == LH264_MB_I8x8) {
      int8_t cache[48];
      for (int i = 0; i < 48; i++) cache[i] = 0;
      const bool cip = H.constrained_intra_pred;
      bool left_av = x > 0 && k - 1 >= H.first_mb, top_av = k - w >= H.first_mb, topleft_av = x > 0 && k - w - 1 >= H.first_mb;
      const uint32_t lt = left_av ? ws[k - 1].mb_type : 0, tt = top_av ? ws[k - w].mb_type : 0, tlt = topleft_av ? ws[k - w - 1].mb_type : 0;
      if (!cip) {
        if (top_av && nxn_[k - w]) for (int i = 0; i < 4; i++) cache[1 + i] = ipm_[(size_t) (k - w) * 8 + i];
        else for (int i = 0; i < 4; i++) cache[1 + i] = (int8_t) (top_av ? 2 : -1);
        if (left_av && nxn_[k - 1]) {
          const int8_t* li = &ipm_[(size_t) (k - 1) * 8];
          cache[8] = li[4]; cache[16] = li[5]; cache[24] = li[6]; cache[32] = li[3];
        } else cache[8] = cache[16] = cache[24] = cache[32] = (int8_t) (left_av ? 2 : -1);
      } else {
        if (top_av && tt == LH264_MB_I4x4) for (int i = 0; i < 4; i++) cache[1 + i] = ipm_[(size_t) (k - w) * 8 + i];
        else for (int i = 0; i < 4; i++) cache[1 + i] = (int8_t) ((tt == LH264_MB_I16x16 || tt == LH264_MB_IPCM) ? 2 : -1);
        if (left_av && lt == LH264_MB_I4x4) {
          const int8_t* li = &ipm_[(size_t) (k - 1) * 8];
          cache[8] = li[4]; cache[16] = li[5]; cache[24] = li[6]; cache[32] = li[3];
        } else cache[8] = cache[16] = cache[24] = cache[32] = (int8_t) ((lt == LH264_MB_I16x16 || lt == LH264_MB_IPCM) ? 2 : -1);
        left_av = left_av && (lt & LH264_MB_INTRA); top_av = top_av && (tt & LH264_MB_INTRA); topleft_av = topleft_av && (tlt & LH264_MB_INTRA);
      }
      if (type == LH264_MB_I4x4) {
        uint8_t sample_av[30];
        for (int i = 0; i < 30; i++) sample_av[i] = 0;
        sample_av[0] = topleft_av;
        for (int i = 1; i <= 4; i++) { sample_av[i] = top_av; sample_av[6 * i] = left_av; }
        for (int i = 0; i < 16; i++) {
          const int top_mode = cache[T.scan8[i] - 8], left_mode = cache[T.scan8[i] - 1];
          const int pred = (left_mode == -1 || top_mode == -1) ? 2 : (left_mode < top_mode ? left_mode : top_mode);
          const int idx = T.cache30[i];
          sample_av[idx] = 1;
          const int avail_idx = (sample_av[idx - 1] ? 4 : 0) | (sample_av[idx - 6] ? 2 : 0) | (sample_av[idx - 7] ? 1 : 0);
          m.pred_mode[i] = (int)tree (TAG_PRED_MODE, LH264_TB_PREDMODE, (uint32_t) ((mbc * 8 + avail_idx) * 9 + pred));
          if (m.pred_mode[i] > 8) { fail (RS_CORRUPT); return; }
          cache[T.scan8[i]] = (int8_t)m.pred_mode[i];
        }
      } else {
        for (int i = 0; i < 4; i++) {
          m.pred_mode[i] = (int)tree (TAG_PRED_MODE, LH264_TB_PREDMODE, (uint32_t) ((mbc * 8 + 6) * 9 + 1));
          if (m.pred_mode[i] > 8) { fail (RS_CORRUPT); return; }
        }
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) cache[T.scan8[(i << 2) + j]] = (int8_t)m.pred_mode[i];
      }
      for (int i = 0; i < 4; i++) my_ipm[i] = cache[1 + 8 * 4 + i];
      my_ipm[4] = cache[4 + 8 * 1]; my_ipm[5] = cache[4 + 8 * 2]; my_ipm[6] = cache[4 + 8 * 3];
      nxn_[k] = 1;
    } else nxn_[k] = 0;
    auto mvd = [&] (int blk) {
      m.mvd[blk][0] = scan_uegk (get (LH264_TB_MVD, type * 16 + (uint32_t)blk), 9, 4, 3, 4, 3, TAG_MVX, TAG_MVX, TAG_MVX, TAG_MVX);
      m.mvd[blk][1] = scan_uegk (get (LH264_TB_MVD, type * 16 + (uint32_t)blk), 9, 4, 3, 4, 3, TAG_MVY, TAG_MVY, TAG_MVY, TAG_MVY);
    };
    auto sub = [&] (int i) { m.sub_type[i] = (int)tree (TAG_SUB_MB, LH264_TB_SUBMB, (uint32_t)mbc); };
    auto ref = [&] (int i) { m.ref_idx[i] = (int)scan_raw_bits (TAG_REF, ref_bits); };
    if (type == LH264_MB_I8x8) {
      for (int i = 0; i < 4; i++) sub (i);
      for (int i = 0; i < 4; i++) ref (i);
    } else if (type == LH264_MB_P8x8 || type == LH264_MB_P8x8REF0) {
      for (int i = 0; i < 4; i++) sub (i);
      if (type == LH264_MB_P8x8) for (int i = 0; i < 4; i++) ref (i);
      for (int i = 0; i < 4; i++) {
        switch (m.sub_type[i]) {
        case LH264_SUB_8x8: mvd (T.z2raster[i << 2]); break;
        case LH264_SUB_8x4: for (int j = 0; j < 2; j++) mvd (T.z2raster[(i << 2) + (j << 1)]); break;
        case LH264_SUB_4x8: for (int j = 0; j < 2; j++) mvd (T.z2raster[(i << 2) + j]); break;
        case LH264_SUB_4x4: for (int j = 0; j < 4; j++) mvd (T.z2raster[(i << 2) + j]); break;
        default: fail (RS_CORRUPT); return;
        }
      }
    } else if (type == LH264_MB_P8x16 || type == LH264_MB_P16x8) {
      for (int i = 0; i < 2; i++) ref (i);
      for (int i = 0; i < 2; i++) mvd (type == LH264_MB_P16x8 ? i * 8 : i * 2);
    } else if (type == LH264_MB_P16x16) {
      ref (0);
      mvd (0);
    }
    {
      bool no_sub_lt8 = true;
      if (type == LH264_MB_P8x8 || type == LH264_MB_P8x8REF0) for (int i = 0; i < 4; i++) no_sub_lt8 = no_sub_lt8 && m.sub_type[i] == LH264_SUB_8x8;
      const bool is_inter = (type & LH264_MB_INTER) != 0;
      if (((type >= LH264_MB_P16x16 && type <= LH264_MB_P8x16) || no_sub_lt8) && is_inter && m.cbp_l > 0 && H.transform_8x8)
        m.t8 = scan_bit (TAG_T8, get (LH264_TB_T8, (uint32_t) (mbc * 128 + m.luma_qp)));
      else m.t8 = type == LH264_MB_I8x8;
    }
    Cell e;
    e.initialized = 1; e.zeroed = 0; e.cbp_c = (uint8_t)m.cbp_c; e.cbp_l = (uint8_t)m.cbp_l; e.chroma_mode = (uint8_t)m.chroma_mode; e.luma16_mode = (uint8_t)m.luma16_mode;
    e.mb_type = type; e.num_ref = (uint32_t)m.num_ref; e.cached_skips = 0;
    decode_coeffs (m, st, mbc, x > 0 ? &cur[k - 1] : nullptr, k >= w ? &cur[k - w] : nullptr, np, e);
    if (failed()) return;
    e.zeroed = 1;
    for (int i = 0; i < 384; i++) if (m.lev[i]) { e.zeroed = 0; break; }
    cur[k] = e;
    if constexpr (kCabac) if (cabac) {
        write_mb_cabac (H, k, &m, qp_prev, last_dqp); ce_terminate (has_stop);
        if (has_stop) break;
        continue;
      }
    if (is_p) { put_ue (pending_skips); pending_skips = 0; }
    write_mb (H, k, m, qp_prev);
    if (has_stop) break;
  }
  if constexpr (kCabac) if (cabac) {
      // the codeword ends with the rbsp stop bit on a byte; the low 7 bits of its last byte are what the compressor saw there
      const unsigned pad_value = scan_raw_bits (TAG_PADBYTE, 7);
      if (failed()) return;
      if (pos == pos0) { fail (RS_CORRUPT); return; }
      J.out[pos - 1] = (uint8_t) ((J.out[pos - 1] & 0x80u) | pad_value);     // (not failed: pos <= out_cap)
      return;
    }
  if (pending_skips) put_ue (pending_skips);
  // rbsp_slice_trailing_bits: the stop bit, then the alignment bits as the compressor saw them
  const int pad_bits = 7 - (nbits & 7);
  const unsigned pad_value = pad_bits ? scan_raw_bits (TAG_PADBYTE, pad_bits) : 0;
  emit_bit (1);
  emit_bits (pad_value, pad_bits);
}

#ifdef __HIP_DEVICE_COMPILE__
#define RBAR() __syncthreads()
#else
#define RBAR() ((void)0)
#endif

// one stream on `nl` lanes (the kernel: a wave; the CPU check: one); the bookkeeping of decode_slice on every lane, the chain on lane 0
template <bool kCabac>
LH_HD void restore_stream (const RestoreJob& J, const RestoreTables& Tg, Shared& S, int lane, int nl, const RestoreCabacTables* CT, CabacShared* CS) {
  typedef typename Chain<kCabac>::W W;
  {
    const uint32_t* src = (const uint32_t*)&Tg;
    uint32_t* dst = (uint32_t*)&S.T;
    for (unsigned i = (unsigned)lane; i < sizeof (RestoreTables) / 4; i += (unsigned)nl) dst[i] = src[i];
  }
  if constexpr (kCabac) {
    const uint32_t* src = (const uint32_t*)&CT->enc;
    uint32_t* dst = (uint32_t*)&CS->K;
    for (unsigned i = (unsigned)lane; i < sizeof (RestoreCabacEnc) / 4; i += (unsigned)nl) dst[i] = src[i];
  }
  if (lane == 0) {
    S.status = RS_OK;
    S.test_prob = DP_INIT;
    for (int i = 0; i < 24; i++) S.zero[i] = 0;
    for (int t = 0; t < 2; t++) { S.esc[t] = EscapeCursor{0, 0, 0, 0}; escape_load (S.esc[t], J.esc[t], J.n_esc[t]); }
    if (J.esc_bad) S.status = RS_CORRUPT;
  }
  if (lane < N_TAGS) {
    for (int t = lane; t < N_TAGS; t += nl) {
      Reader& r = S.rd[t];
      r.p = J.tags + J.tag_off[t]; r.end = r.p + J.tag_len[t];
      r.value = 0; r.count = -8; r.range = 255; r.pad = 0;
      r.present = t != LH264_TAG_PCM && t != LH264_TAG_ESC && ((J.tag_present[t >> 5] >> (t & 31)) & 1u);
      if (r.present) rd_fill (r);
    }
  }
  RBAR();
  Chain<kCabac> c (J, S);
  if constexpr (kCabac) c.C = CS;
  c.img[0] = (Cell*)J.cells; c.img[1] = (Cell*)J.cells + J.n_max;
  c.ws = (W*)J.ws;
  const bool have_pcm = (J.tag_present[LH264_TAG_PCM >> 5] >> (LH264_TAG_PCM & 31)) & 1u;
  c.pcm = have_pcm ? J.tags + J.tag_off[LH264_TAG_PCM] : nullptr;
  c.pcm_end = have_pcm ? c.pcm + J.tag_len[LH264_TAG_PCM] : nullptr;
  c.used = 0; c.pool_used = 512; c.sid = 0; c.pos = 0; c.bits = 0; c.nbits = 0;
  if (J.pool_cap < 512 || J.slots < 2) { if (lane == 0) c.fail (RS_STORE_FULL); }
  // Restorer's bookkeeping (uniform across the wave)
  int img_w = 0, img_h = 0, cur = 0, last_frame_id = 0, ipm_n = 0, ws_n = 0;
  RBAR();
  for (uint32_t si = 0; si < J.n_slices; si++) {
    if (S.status != RS_OK) break;
    const RestoreSlice H = J.slices[si];
    const int n = H.mb_w * H.mb_h;
    if (n <= 0 || H.first_mb < 0 || H.first_mb >= n || (!kCabac && H.cabac)) { if (lane == 0) c.fail (RS_CORRUPT); break; }
    if ((uint32_t)n > J.n_max) { if (lane == 0) c.fail (RS_STORE_FULL); break; }
    if (ipm_n != n * 8) {
      for (int i = lane; i < n * 2; i += nl) ((uint32_t*)J.ipm)[i] = 0;
      for (int i = lane; i < n; i += nl) J.nxn[i] = 0;
      ipm_n = n * 8;
    }
    if (ws_n != n) {
      const int ww = (int) (sizeof (W) / 4);
      for (int i = lane; i < n * ww; i += nl) ((uint32_t*)J.ws)[i] = (i % ww) == 0 ? 0xffffffffu : 0u;
      ws_n = n;
    }
    c.sid++;
    bool prior_valid = true;
    // update_frame: the cached_skips of each run of zeroed cells of the frame before, one non-zeroed cell per lane
    if (H.frame_num != last_frame_id) { cur = cur ? 0 : 1; last_frame_id = H.frame_num; }
    {
      Cell* f = c.img[1 - cur];
      const int fn = img_w * img_h;
      for (int i = lane; i < fn; i += nl) {
        if (f[i].zeroed) continue;
        int run = 0;
        while (run < i && f[i - 1 - run].zeroed) run++;
        for (int j = 0; j < run; j++) f[i - j].cached_skips = (uint16_t)run;
      }
    }
    RBAR();
    if (img_w != H.mb_w || img_h != H.mb_h) {
      prior_valid = false;
      img_w = H.mb_w; img_h = H.mb_h;
      for (int i = lane; i < n * 10; i += nl) { ((uint32_t*)c.img[0])[i] = 0; ((uint32_t*)c.img[1])[i] = 0; }
    }
    if constexpr (kCabac) if (H.cabac) {                  // CabacEnc::init, a lane per context (9.3.1.1)
        const int col = H.slice_type == 0 ? imin (3, 1 + (H.cabac >> 1)) : 0;
        const int qp = H.slice_qp < 0 ? 0 : imin (51, H.slice_qp);
        for (int i = lane; i < 460; i += nl) {
          const int pre0 = ((CT->init[i][col][0] * qp) >> 4) + CT->init[i][col][1];
          const int pre = pre0 < 1 ? 1 : imin (126, pre0);
          CS->state[i] = pre <= 63 ? (uint8_t) ((63 - pre) << 1) : (uint8_t) (((pre - 64) << 1) | 1);
        }
      }
    RBAR();
    if (lane == 0) {
      c.nbits = H.phase; c.bits = 0;
      if constexpr (kCabac) c.ce_reset();
      c.decode_slice (H, cur, prior_valid, J.ipm, J.nxn);
      J.slice_end[si] = c.pos;
    }
    RBAR();
  }
  // entries beyond the last symbol: the tag belongs to another stream
  if (lane == 0 && (S.esc[0].rep | S.esc[1].rep)) c.fail (RS_CORRUPT);
  if (lane == 0) { J.status[0] = S.status; J.status[1] = (int32_t)c.used; J.status[2] = (int32_t)c.pool_used; J.status[3] = (int32_t)c.pos; }
}

}  // namespace

// one workgroup (one wave) per stream, the longest first (order).  Uncapped the compiler gives the chain 256 VGPRs and 50 AGPRs: one
// wave per SIMD.  Four waves per SIMD (128 VGPRs, the rest in scratch) keep four times as many chains in flight
#ifndef LH264_RESTORE_WAVES
#define LH264_RESTORE_WAVES 4
#endif
__global__ __launch_bounds__ (64) __attribute__ ((amdgpu_waves_per_eu (LH264_RESTORE_WAVES))) void restore_kernel (const RestoreJob* jobs, const int32_t* order, int n, const RestoreTables* tables) {
  __shared__ Shared S;
  if ((int)blockIdx.x >= n) return;
  restore_stream<false> (jobs[order[blockIdx.x]], *tables, S, (int)threadIdx.x, (int)blockDim.x, nullptr, nullptr);
}
// the same with the CABAC writer beside the CAVLC one, for batches in which a stream has a CABAC slice; an instance of its own, so
// that the CAVLC batches run the kernel above with its registers and LDS
__global__ __launch_bounds__ (64) __attribute__ ((amdgpu_waves_per_eu (LH264_RESTORE_WAVES))) void restore_cabac_kernel (const RestoreJob* jobs, const int32_t* order, int n, const RestoreTables* tables,
                                                                                                                   const RestoreCabacTables* ctables) {
  __shared__ Shared S;
  __shared__ CabacShared CS;
  if ((int)blockIdx.x >= n) return;
  restore_stream<true> (jobs[order[blockIdx.x]], *tables, S, (int)threadIdx.x, (int)blockDim.x, ctables, &CS);
}

// dp_update alone, one pair of counts per thread (lh264_debug_dp_update)
__global__ __launch_bounds__ (256) void dp_update_kernel (const uint32_t* words, const uint8_t* bits, uint32_t* out, int n) {
  const int i = (int) (blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) out[i] = dp_update (words[i], bits[i] & 1);
}

// the same chain on the host, one stream at a time (no device: the CPU check of the transliteration)
void restore_stream_host (const RestoreJob& J, const RestoreTables& T, const RestoreCabacTables* CT) {
  static thread_local Shared S;
  static thread_local CabacShared CS;
  if (CT) restore_stream<true> (J, T, S, 0, 1, CT, &CS);
  else restore_stream<false> (J, T, S, 0, 1, nullptr, nullptr);
}

}  // namespace lh264r

// ---- host side: lh264_pip_restore_batch_device -----------------------------------------------------------------------------------
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "host/capi_internal.h"
#include "host/device_mem.h"
#include "host/pip_restore.h"

namespace {
using namespace lh264r;

double now_ms() { return 1e3 * lh264host::now_s(); }
bool trace_on() { static const bool t = lh264host::trace_on ("LH264_TRACE_RESTORE"); return t; }
// test-only capacity overrides (0 / unset: the host's estimate)
uint32_t env_u32 (const char* name) { const char* e = getenv (name); return e ? (uint32_t)strtoul (e, nullptr, 10) : 0u; }
inline size_t al256 (size_t v) { return (v + 255) & ~(size_t)255; }

struct Plan {
  int path = LH264_RESTORE_PATH_FALLBACK;
  bool cabac = false;                                   // a slice of the stream is a CABAC slice
  std::vector<RestoreSlice> slices;
  std::vector<RestoreEscape> esc[2];                    // tag LH264_TAG_ESC by table; esc_bad: it is malformed
  bool esc_bad = false;
  size_t off_esc = 0;
  size_t tag_bytes = 0;
  uint32_t n_max = 0, slots = 0, pool_cap = 0, out_cap = 0;
  size_t off_slices = 0, off_tags = 0, off_hash = 0, off_work = 0, off_status = 0, off_end = 0, off_out = 0;
};

// device and page-locked buffers kept between calls, one set per device; one call at a time per device
struct RestoreArena {
  lh264host::DevBuf dev; lh264host::PinBuf pin_in, pin_out;
  hipStream_t stream = nullptr; hipEvent_t ev[2] = {nullptr, nullptr};
  bool init() {
    if (stream) return true;
    if (hipStreamCreateWithFlags (&stream, hipStreamNonBlocking) == hipSuccess && hipEventCreate (&ev[0]) == hipSuccess && hipEventCreate (&ev[1]) == hipSuccess) return true;
    drop_stream();
    return false;
  }
  void drop_stream() {
    if (ev[0]) hipEventDestroy (ev[0]);
    if (ev[1]) hipEventDestroy (ev[1]);
    if (stream) hipStreamDestroy (stream);
    stream = nullptr; ev[0] = ev[1] = nullptr;
  }
  ~RestoreArena() { drop_stream(); }
};
lh264host::PerDevice<RestoreArena> g_arena;      // (the CPU check takes device 0's lock and no arena)
std::mutex g_timing_mutex;
double g_timing[4] = {0, 0, 0, 0};

// the per-stream capacities (measured on the reference-written files: DESIGN.md 4.5)
void size_plan (Plan& P, const lh264_restore_item_t& it) {
  uint32_t n_max = 0;
  for (const RestoreSlice& s : P.slices) n_max = std::max (n_max, (uint32_t) (s.mb_w * s.mb_h));
  P.n_max = n_max;
  size_t coded = 0;                                     // the model's tags (the pad bits and the I_PCM samples excepted)
  for (int t = 0; t < it.n_tags && t < 72; t++) if (it.tags[t] && t != LH264_TAG_PCM && t != 69) coded += it.tag_len[t];
  // prior keys: at most 0.38 per tag byte on the reference's files (Static.264; 0.1 on the 1080p ones), 13 pool words per key at most
  const size_t keys = std::min<size_t> ((size_t)1 << 22, 4096 + coded / 2);
  uint32_t slots = 1024;
  while (slots < 2 * keys) slots <<= 1;
  if (uint32_t e = env_u32 ("LH264_RESTORE_SLOTS")) { slots = 2; while (slots < e) slots <<= 1; }
  P.slots = slots;
  P.pool_cap = 512 + 16 * (slots / 2);
  if (uint32_t e = env_u32 ("LH264_RESTORE_POOL")) P.pool_cap = e;
  const size_t pcm = (it.n_tags > LH264_TAG_PCM && it.tags[LH264_TAG_PCM]) ? it.tag_len[LH264_TAG_PCM] : 0;
  // the slice data is at most 1.27 x the tags that code it on the reference's files; twice that, the I_PCM samples and a few bytes per
  // slice and macroblock.  CABAC slices, counted on their own (status[3] of the reference-written CABAC files): 1.055 x at most
  // (test_cif_P_CABAC_slice.264, 4,200 slices), so 2 x the tags is 1.9 x the largest seen and serves them too
  P.out_cap = (uint32_t)std::min<size_t> (0xfffff000u, 2 * coded + 2 * pcm + 64 * P.slices.size() + 2 * (size_t)n_max + 4096);
  if (uint32_t e = env_u32 ("LH264_RESTORE_OUT_CAP")) P.out_cap = e;
}

void item_from_bytes (lh264_restore_item_t& it, const std::vector<uint8_t>& o) {       // as lh264_pip_restore hands out a result
  it.out_len = o.size();
  if (o.size() > it.out_cap || (!it.out && o.size())) { it.status = LH264_E_ARG; return; }
  if (o.size()) memcpy (it.out, o.data(), o.size());
  it.status = LH264_OK;
}
void host_restore (lh264_restore_item_t& it) {
  it.status = lh264_pip_restore (it.main_stream, it.main_len, it.tags, it.tag_len, it.n_tags, it.out, it.out_cap, &it.out_len);
}

// device == false: the kernel's code stepped on the host threads over host memory (lh264_debug_restore_cpu)
int restore_batch (lh264_restore_item_t* items, int n, const lh264_restore_opts_t* opts, int32_t* path_out, bool device) {
  if (!items || n < 0) return LH264_E_ARG;
  if (opts && (opts->struct_bytes != sizeof (lh264_restore_opts_t) || (opts->flags & ~LH264_RESTORE_CABAC_DEVICE))) return LH264_E_ARG;
  const int threads = opts ? opts->threads : 0;
  const bool cabac_device = opts && (opts->flags & LH264_RESTORE_CABAC_DEVICE);
  int dev = 0;
  if (device) {
    if (lh264_device_count() <= 0 || hipGetDevice (&dev) != hipSuccess) return LH264_E_NODEVICE;
    if (dev < 0 || dev >= lh264host::kMaxDevices) return LH264_E_ARG;
  }
  auto lock = g_arena.lock (device ? dev : 0);
  double t[5]; t[0] = now_ms();
  // pass 1
  std::vector<Plan> plans (n);
  run_parallel (n, threads, [&] (int i) {
    const lh264_restore_item_t& it = items[i];
    Plan& P = plans[i];
    P.path = LH264_RESTORE_PATH_FALLBACK;
    if (!it.main_stream || !it.tags || !it.tag_len || it.n_tags < 0) return;      // lh264_pip_restore reports it
    std::string err;
    if (lh264host::pip_restore_describe (it.main_stream, it.main_len, P.slices, P.cabac, err, cabac_device) < 0) return;
    if (P.cabac && !cabac_device) { P.path = LH264_RESTORE_PATH_HOST; return; }
    if (it.n_tags > LH264_TAG_ESC && it.tags[LH264_TAG_ESC])
      P.esc_bad = lh264host::pip_restore_describe_escapes (it.tags[LH264_TAG_ESC], it.tag_len[LH264_TAG_ESC], P.esc, err) < 0;
    for (int q = 0; q < it.n_tags && q < 72; q++) if (it.tags[q]) P.tag_bytes += it.tag_len[q];
    if (P.tag_bytes >= 0xfffff000u) return;
    size_plan (P, it);
    P.path = LH264_RESTORE_PATH_DEVICE;
  });
  std::vector<int> dev_items, host_items;
  for (int i = 0; i < n; i++) (plans[i].path == LH264_RESTORE_PATH_DEVICE ? dev_items : host_items).push_back (i);
  // the longest chains first: tag bytes stand for decisions
  std::stable_sort (dev_items.begin(), dev_items.end(), [&] (int a, int b) { return plans[a].tag_bytes > plans[b].tag_bytes; });
  const int nd = (int)dev_items.size();
  // the kernel instance with the CABAC writer only where a stream of the batch needs it: its WState is the longer one
  bool any_cabac = false;
  for (int i : dev_items) any_cabac = any_cabac || plans[i].cabac;
  const size_t ws_bytes = any_cabac ? sizeof (WStateC) : sizeof (WState);
  // layout: [inputs: tables, jobs, order, per stream slices + tags] [hash tables: zeroed] [work memory] [outputs: status, slice ends, bits]
  size_t off = 0;
  const size_t off_tables = off; off += al256 (sizeof (RestoreTables));
  const size_t off_ctables = off; if (any_cabac) off += al256 (sizeof (RestoreCabacTables));
  const size_t off_jobs = off; off += al256 (sizeof (RestoreJob) * (size_t)nd);
  const size_t off_order = off; off += al256 (sizeof (int32_t) * (size_t)nd);
  for (int i : dev_items) {
    Plan& P = plans[i];
    P.off_slices = off; off += al256 (sizeof (RestoreSlice) * P.slices.size());
    P.off_tags = off; off += al256 (P.tag_bytes);
    P.off_esc = off; off += al256 (sizeof (RestoreEscape) * (P.esc[0].size() + P.esc[1].size()));
  }
  const size_t in_bytes = off;
  const size_t off_zero = off;
  for (int i : dev_items) { plans[i].off_hash = off; off += al256 ((size_t)plans[i].slots * 8); }
  const size_t zero_bytes = off - off_zero;
  for (int i : dev_items) {
    Plan& P = plans[i];
    P.off_work = off;
    off += al256 ((size_t)P.n_max * (2 * 40 + ws_bytes + 8 + 4)) + al256 ((size_t)P.pool_cap * 4);
  }
  const size_t off_outr = off;
  for (int i : dev_items) {
    Plan& P = plans[i];
    P.off_status = off; off += 256;
    P.off_end = off; off += al256 (4 * P.slices.size());
    P.off_out = off; off += al256 (P.out_cap);
  }
  const size_t total = off, out_bytes = total - off_outr;
  // memory: the arena on the device, or host memory for the CPU check
  std::vector<uint8_t> host_mem;
  uint8_t* base = nullptr;       // addresses the kernel sees
  uint8_t* in_stage = nullptr;   // where the host assembles the inputs
  uint8_t* out_stage = nullptr;  // where the outputs arrive
  RestoreArena* A = nullptr;
  if (device) {
    A = &lock.get();
    if (!A->init() || !A->dev.alloc (total) || !A->pin_in.alloc (in_bytes) || !A->pin_out.alloc (out_bytes)) return LH264_E_HIP;
    base = A->dev.as<uint8_t>(); in_stage = A->pin_in.as<uint8_t>(); out_stage = A->pin_out.as<uint8_t>() - off_outr;
  } else {
    host_mem.assign (total, 0);
    base = host_mem.data(); in_stage = host_mem.data(); out_stage = host_mem.data();
  }
  lh264host::restore_tables (*(RestoreTables*) (in_stage + off_tables));
  if (any_cabac) lh264host::restore_cabac_tables (*(RestoreCabacTables*) (in_stage + off_ctables));
  RestoreJob* jobs = (RestoreJob*) (in_stage + off_jobs);
  int32_t* order = (int32_t*) (in_stage + off_order);
  run_parallel (nd, threads, [&] (int j) {
    const int i = dev_items[j];
    const lh264_restore_item_t& it = items[i];
    const Plan& P = plans[i];
    RestoreJob& J = jobs[j];
    memset (&J, 0, sizeof (J));
    memcpy (in_stage + P.off_slices, P.slices.data(), sizeof (RestoreSlice) * P.slices.size());
    uint32_t to = 0;
    for (int q = 0; q < it.n_tags && q < 72; q++) {
      if (!it.tags[q]) continue;
      J.tag_present[q >> 5] |= 1u << (q & 31);
      J.tag_off[q] = to; J.tag_len[q] = (uint32_t)it.tag_len[q];
      if (it.tag_len[q]) memcpy (in_stage + P.off_tags + to, it.tags[q], it.tag_len[q]);
      to += (uint32_t)it.tag_len[q];
    }
    J.tags = base + P.off_tags;
    for (int t = 0, at = 0; t < 2; t++) {
      if (!P.esc[t].empty()) memcpy (in_stage + P.off_esc + sizeof (RestoreEscape) * at, P.esc[t].data(), sizeof (RestoreEscape) * P.esc[t].size());
      J.esc[t] = (const RestoreEscape*) (base + P.off_esc) + at; J.n_esc[t] = (uint32_t)P.esc[t].size();
      at += (int)P.esc[t].size();
    }
    J.esc_bad = P.esc_bad ? 1u : 0u;
    J.n_slices = (uint32_t)P.slices.size(); J.n_max = P.n_max;
    J.slices = (const RestoreSlice*) (base + P.off_slices);
    uint8_t* w = base + P.off_work;
    J.cells = w; w += (size_t)P.n_max * 80;
    J.ws = w; w += (size_t)P.n_max * ws_bytes;
    J.ipm = (int8_t*)w; w += (size_t)P.n_max * 8;
    J.nxn = w;
    J.pool = (uint32_t*) (base + P.off_work + al256 ((size_t)P.n_max * (2 * 40 + ws_bytes + 8 + 4)));
    J.hash = (uint32_t*) (base + P.off_hash);
    J.slots = P.slots; J.pool_cap = P.pool_cap;
    J.out = base + P.off_out; J.out_cap = P.out_cap;
    J.slice_end = (uint32_t*) (base + P.off_end);
    J.status = (int32_t*) (base + P.off_status);
    order[j] = j;
  });
  t[1] = now_ms();
  double kernel_ms = 0;
  if (device) {
    hipStream_t s = A->stream;
    bool ok = hipMemcpyAsync (base, in_stage, in_bytes, hipMemcpyHostToDevice, s) == hipSuccess;
    ok = ok && (zero_bytes == 0 || hipMemsetAsync (base + off_zero, 0, zero_bytes, s) == hipSuccess);
    if (ok && nd) {
      ok = ok && hipEventRecord (A->ev[0], s) == hipSuccess;
      if (any_cabac) hipLaunchKernelGGL (restore_cabac_kernel, dim3 ((unsigned)nd), dim3 (64), 0, s, (const RestoreJob*) (base + off_jobs), (const int32_t*) (base + off_order), nd,
                                         (const RestoreTables*) (base + off_tables), (const RestoreCabacTables*) (base + off_ctables));
      else hipLaunchKernelGGL (restore_kernel, dim3 ((unsigned)nd), dim3 (64), 0, s, (const RestoreJob*) (base + off_jobs), (const int32_t*) (base + off_order), nd,
                               (const RestoreTables*) (base + off_tables));
      ok = ok && hipGetLastError() == hipSuccess;
      ok = ok && hipEventRecord (A->ev[1], s) == hipSuccess;
      ok = ok && hipMemcpyAsync (A->pin_out.p, base + off_outr, out_bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    if (!ok) { hipStreamSynchronize (s); return LH264_E_HIP; }
    // the streams the host restores go while the device works
    run_parallel ((int)host_items.size(), threads, [&] (int j) { if (plans[host_items[j]].path == LH264_RESTORE_PATH_HOST) host_restore (items[host_items[j]]); });
    if (hipStreamSynchronize (s) != hipSuccess) return LH264_E_HIP;
    float ms = 0;
    if (nd && hipEventElapsedTime (&ms, A->ev[0], A->ev[1]) == hipSuccess) kernel_ms = ms;
  } else {
    if (zero_bytes) memset (host_mem.data() + off_zero, 0, zero_bytes);
    run_parallel ((int)host_items.size(), threads, [&] (int j) { if (plans[host_items[j]].path == LH264_RESTORE_PATH_HOST) host_restore (items[host_items[j]]); });
    run_parallel (nd, threads, [&] (int j) {
      restore_stream_host (jobs[j], *(const RestoreTables*) (host_mem.data() + off_tables), any_cabac ? (const RestoreCabacTables*) (host_mem.data() + off_ctables) : nullptr);
    });
  }
  t[2] = now_ms();
  // pass 2
  run_parallel (nd, threads, [&] (int j) {
    const int i = dev_items[j];
    lh264_restore_item_t& it = items[i];
    Plan& P = plans[i];
    const int32_t st = *(const int32_t*) (out_stage + P.off_status);
    if (trace_on()) {
      const int32_t* q = (const int32_t*) (out_stage + P.off_status);
      fprintf (stderr, "[lh264 restore] stream %d: status %d, %d of %u prior keys, %d of %u pool words, %d of %u bytes (%zu tag bytes, %zu slices, %u MBs)\n",
               i, st, q[1], P.slots / 2, q[2], P.pool_cap, q[3], P.out_cap, P.tag_bytes, P.slices.size(), P.n_max);
    }
    if (st == RS_OK) {
      std::vector<uint8_t> o;
      std::string err;
      if (lh264host::pip_restore_splice (it.main_stream, it.main_len, P.slices.data(), P.slices.size(), out_stage + P.off_out,
                                         (const uint32_t*) (out_stage + P.off_end), o, err) == 0) { item_from_bytes (it, o); return; }
    }
    P.path = LH264_RESTORE_PATH_FALLBACK;
  });
  // what the device path could not do, the host restore does
  std::vector<int> fb;
  for (int i = 0; i < n; i++) if (plans[i].path == LH264_RESTORE_PATH_FALLBACK) fb.push_back (i);
  run_parallel ((int)fb.size(), threads, [&] (int j) { host_restore (items[fb[j]]); });
  if (path_out) for (int i = 0; i < n; i++) path_out[i] = plans[i].path;
  t[3] = now_ms();
  {
    std::lock_guard<std::mutex> tl (g_timing_mutex);
    g_timing[0] = t[1] - t[0]; g_timing[1] = t[2] - t[1]; g_timing[2] = kernel_ms; g_timing[3] = t[3] - t[2];
  }
  if (trace_on()) fprintf (stderr, "[lh264 restore] %d streams (%d on the device, %zu elsewhere): pass 1 %.2f ms, device %.2f ms (kernel %.2f), pass 2 %.2f ms; %.1f MB of device memory\n",
                           n, nd, fb.size() + host_items.size() - fb.size(), t[1] - t[0], t[2] - t[1], kernel_ms, t[3] - t[2], total / 1e6);
  return LH264_OK;
}

}  // namespace

extern "C" {
int lh264_pip_restore_batch_device (lh264_restore_item_t* items, int n, int threads, int32_t* path_out) {
  const lh264_restore_opts_t o = {(uint32_t)sizeof (lh264_restore_opts_t), threads, 0u};
  return restore_batch (items, n, &o, path_out, true);
}
int lh264_pip_restore_batch_device_opts (lh264_restore_item_t* items, int n, const lh264_restore_opts_t* opts, int32_t* path_out) {
  return restore_batch (items, n, opts, path_out, true);
}
int lh264_debug_restore_cpu (lh264_restore_item_t* items, int n, int threads, int32_t* path_out) {
  const lh264_restore_opts_t o = {(uint32_t)sizeof (lh264_restore_opts_t), threads, 0u};
  return restore_batch (items, n, &o, path_out, false);
}
int lh264_debug_restore_cpu_opts (lh264_restore_item_t* items, int n, const lh264_restore_opts_t* opts, int32_t* path_out) {
  return restore_batch (items, n, opts, path_out, false);
}
int lh264_debug_dp_update (const uint32_t* words, const uint8_t* bits, uint32_t* out, int n) {
  if (!words || !bits || !out || n < 0) return LH264_E_ARG;
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  if (n == 0) return LH264_OK;
  uint8_t* d = nullptr;                                  // [words] [out] [bits]
  const size_t nw = 4 * (size_t)n;
  if (hipMalloc ((void**)&d, 2 * nw + (size_t)n) != hipSuccess) return LH264_E_HIP;
  bool ok = hipMemcpy (d, words, nw, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy (d + 2 * nw, bits, (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL (lh264r::dp_update_kernel, dim3 ((unsigned) ((n + 255) / 256)), dim3 (256), 0, 0, (const uint32_t*)d, (const uint8_t*) (d + 2 * nw),
                        (uint32_t*) (d + nw), n);
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy (out, d + nw, nw, hipMemcpyDeviceToHost) == hipSuccess;
  }
  hipFree (d);
  return ok ? LH264_OK : LH264_E_HIP;
}
int lh264_restore_last_timing (double* ms) {
  if (!ms) return LH264_E_ARG;
  std::lock_guard<std::mutex> tl (g_timing_mutex);
  for (int i = 0; i < 4; i++) ms[i] = g_timing[i];
  return LH264_OK;
}
void lh264_restore_release (void) { g_arena.release_all(); }
}
