// lh264_kernels.hip - gfx950 (MI355X, wave64) kernels of the decode-reconstruct hot path.
//
// One workgroup per chain of frames (the frames of one stream, in decode order), one wavefront
// per macroblock row (row r is served by wave r % NW), row r running at least two macroblocks
// behind row r-1 -- the raster dependency of intra prediction and of the in-loop filter
// (reference loop order: WelsTargetSliceConstruction decode_slice.cpp:110-206, WelsDeblockingFilterSlice
// deblocking.cpp:872-934).  ALL hand-offs between rows go through LDS:
//   * `line`  : the unfiltered bottom sample row of each macroblock row  (intra prediction neighbours)
//   * `fline` : the filtered bottom 4 (chroma 2) sample rows              (deblocking neighbours)
//   * progress counters
// so no wave ever waits for its HBM stores inside a frame.  Per macroblock a wave
//   0. stages the prefetched record (and the record of the MB above) into LDS and prefetches the next one,
//   1. copies the unfiltered neighbours into its private LDS tile,
//   2. inverse-transforms the 384 coefficients (coalesced 768-byte read, prefetched one MB ahead; 4x4
//      butterflies across lane quads with DPP; 8x8 / DC transforms through LDS),
//   3. predicts (intra from the tile, inter = quarter-pel MC straight from the padded reference planes)
//      and adds the residual                                       [RecI*/GetInterPred rec_mb.cpp],
//   4. publishes the unfiltered bottom row / right column,
//   5. deblocks the macroblock's edges inside the tile              [WelsDeblockingMb deblocking.cpp:815],
//   6. writes a 16x16 window displaced by (-4,-3) -- the samples that became final in this step: every
//      output byte is written exactly once -- and publishes the filtered bottom rows.
// Frames of a chain are PIPELINED through the same wavefront: the rows of all frames of the chain form one sequence
// (global row g is served by wave g % NW), there is no barrier between frames.  A wave that finishes a row also pads
// the band of picture rows that just became final (ExpandReferencingPicture, row by row) and publishes a per-wave
// "stored" counter once those HBM stores have completed; a macroblock of the next frame whose motion vectors reach
// into the frame still in flight waits for exactly the rows it reads.  At most two frames are in flight.
//
// Integer work on u8/int16: no MFMA.  Bounds: HBM traffic (1,280 B / intra MB algorithmic) and VALU
// issue; see DESIGN.md.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lh264.h"
#include "lh264_coder_dev.h"

namespace lh264 {

// Explicit address spaces.  HIP pointers are generic by default and hipcc only recovers LDS/global for accesses
// it can trace to a __shared__ variable or a kernel argument; pointers that pass through structs, noinline
// calls or memory become FLAT accesses (slower, and every wait becomes vmcnt(0)&lgkmcnt(0)).
#ifndef LH264_PHASE
#define LH264_PHASE __noinline__
#endif
#ifndef LH264_MIN_WAVES
#define LH264_MIN_WAVES 1
#endif
// diagnostic build (-DLH264_STAMP): cycle stamps per phase, summed over all waves into g_stamps (never in product builds)
#ifdef LH264_STAMP
__device__ unsigned long long g_stamps[16];
#define STAMP_DECL unsigned long long st_t0 = __builtin_amdgcn_s_memtime(); unsigned long long st_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define STAMP(i) do { unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[i] += t_ - st_t0; st_t0 = t_; } while (0)
#define STAMP_FLUSH do { if (lane == 0) for (int i_ = 0; i_ < 12; i_++) atomicAdd (&g_stamps[i_], st_acc[i_]); } while (0)
#else
#define STAMP_DECL
#define STAMP(i) do {} while (0)
#define STAMP_FLUSH do {} while (0)
#endif
using lh264dev::glb;
typedef int v2i __attribute__ ((ext_vector_type (2)));
__device__ __forceinline__ v2i mk2 (int a, int b) { v2i r; r.x = a; r.y = b; return r; }

// ---- tables (H.264 Tables 8-16/8-17; reference copies: deblocking.cpp:89-125) ----------------
__constant__ uint8_t kTables[52 + 52 + 52 * 4] = {
  // alpha
  0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 5, 6, 7, 8, 9, 10, 12, 13,
  15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255,
  // beta
  0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7,
  8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18,
  // tc0[indexA][bS] (bS 0 unused)
  0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
  0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1,
  0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 2, 0, 1, 1, 2, 0, 1, 1, 2,
  0, 1, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3, 0, 2, 2, 3, 0, 2, 2, 4, 0, 2, 3, 4, 0, 2, 3, 4, 0, 3, 3, 5, 0, 3, 4, 6, 0, 3, 4, 6,
  0, 4, 5, 7, 0, 4, 5, 8, 0, 4, 6, 9, 0, 5, 7, 10, 0, 6, 8, 11, 0, 6, 8, 13, 0, 7, 10, 14, 0, 8, 11, 16, 0, 9, 12, 18, 0, 10, 13, 20,
  0, 11, 15, 23, 0, 13, 17, 25
};
#define TAB_ALPHA 0
#define TAB_BETA 52
#define TAB_TC0 104

// ---- workgroup-shared LDS ----------------------------------------------------------------------
// What is fixed for a frame and read by the phases that are not inlined: they take it from here (a broadcast LDS read, made scalar)
// instead of by value in a dozen argument registers.  At most two frames of a chain are in flight, so two blocks do, frame j using
// block j & 1: a wave writes the block on entering frame j, behind its wait for every row of frame j - 2 and older to be stored, and
// the last read of the block by frame j - 2 (inter_phase of its last macroblock) precedes that row's `stored`.  Every wave entering
// a frame writes the same values.
struct FrameLds {
  uint64_t prev_dy;          // luma plane of the previous job of the chain (0: none): the only other frame that can be in flight
  int32_t  sy, sc, mb_w, mb_h;
  int32_t  prev_base;        // global index of the previous job's row 0
  int32_t  prev_h_nw;        // its height in macroblock rows (low half) and the waves of the workgroup (high half)
};
struct WgLds {
  int      progress[8];    // per wave: (rows it has started - 1) << 12 | macroblocks finished in its current row
  int      stored[8];      // per wave: index (among its own rows) of the last row whose HBM stores, including the
                           // padding that row is responsible for, have completed; -1 = none
  FrameLds frame[2];       // (in the 64 bytes that progress and stored had for waves 8..15, which no launch has)
  uint8_t  tab[52 + 52 + 208];
};
static_assert (sizeof (FrameLds) == 32 && sizeof (WgLds) == 128 + 312, "WgLds keeps its size");

// ---- per-wave LDS ------------------------------------------------------------------------------
struct WaveLds {
  uint8_t  T[20 * 32];       // luma tile: rows -4..15, cols -4..27      idx (r+4)*32 + (c+4)
  uint8_t  C[2][10 * 16];    // chroma tiles: rows -2..7, cols -4..11    idx (r+2)*16 + (c+4)
  int16_t  R[384];           // residual, layout [block b (z-order)][row][col] ; chroma blocks 16..23
  uint32_t rec[2][32];       // current / previous (= left) macroblock record, ping-pong
  uint32_t trec[32];         // record of the macroblock above
  uint32_t slc[58];          // cached slice record (lh264_slice_t)
  uint8_t  leftY[16];        // unfiltered right column of the previous MB (intra neighbours)
  uint8_t  leftC[2][8];
  uint32_t lfY[20];          // filtered right 4 columns of the previous MB, rows -4..15
  uint32_t lfC[2][10];       //                                            rows -2..7
  int32_t  mvi[16][4];       // per 4x4 block motion info
  uint8_t  bs[32];           // boundary strengths [dir][edge][segment]
  uint8_t  E[32];            // filtered I8x8 edge
  int32_t  S[64];            // DC transform scratch
  uint64_t refp[LH264_MAX_REFS][3];   // reference plane pointers of this wave's current job
  int32_t  known_prefix;     // every global row <= known_prefix is known to be stored (cache of wait_prefix)
};
// the glue of process_mb addresses the tiles and the carry as one array each: lane l moves dword l
static_assert (offsetof (WaveLds, T) == 0 && offsetof (WaveLds, C) == 640 && sizeof (WaveLds::C) == 320, "tile layout");
static_assert (offsetof (WaveLds, lfC) == offsetof (WaveLds, lfY) + 80, "carry layout");
#define TILE_C(p) ((p) ? 800 : 640)      // byte offset of chroma tile p from the luma tile (a select, not a multiply)

__device__ __forceinline__ int tY (int r, int c) { return (r + 4) * 32 + (c + 4); }
__device__ __forceinline__ int tC (int r, int c) { return (r + 2) * 16 + (c + 4); }
__device__ __forceinline__ int clip_u8 (int v) { return min (max (v, 0), 255); }
__device__ __forceinline__ int clip3 (int v, int lo, int hi) { return min (max (v, lo), hi); }
__device__ __forceinline__ int zidx (int bx, int by) { return (bx & 1) | ((by & 1) << 1) | ((bx >> 1) << 2) | ((by >> 1) << 3); }
__device__ __forceinline__ int tab_idx (int v) { return clip3 (v, 0, 51); }
__device__ __forceinline__ int uni (int v) { return __builtin_amdgcn_readfirstlane (v); }
// a * b + c for a < 2^24 and a wave-uniform b < 2^24 (rows times a stride): one full-rate instruction where the 32-bit multiply
// takes four issue slots
__device__ __forceinline__ uint32_t mad24 (uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm ("v_mad_u32_u24 %0, %1, %2, %3" : "=v" (r) : "v" (a), "s" (b), "v" (c));
  return r;
}

// order LDS traffic between the lanes of one wave.  The DS instructions of a wave execute in issue order, so
// a later ds_read observes an earlier ds_write of any lane; all that is needed is to stop the COMPILER from
// moving memory operations across this point.  (A wavefront-scope fence would do that too, but hipcc lowers
// it to "s_waitcnt vmcnt(0) lgkmcnt(0)", which drains the prefetches and the output stores at every phase.)
__device__ __forceinline__ void wsync() {
  asm volatile ("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

template <int K> __device__ __forceinline__ int quad_bcast (int v) {
  return __builtin_amdgcn_mov_dpp (v, K * 0x55, 0xf, 0xf, true);
}
__device__ __forceinline__ int sext16 (int v) { return (int) (short)v; }

// 4x4 inverse transform over a lane quad: lane r of the quad holds row r (4 coefficients) of the block and
// receives row r of the residual ((x+32)>>6).  Rows first with int16 intermediates, then columns
// (IdctResAddPred_c, decode_mb_aux.cpp:42-77).
__device__ __forceinline__ void idct4x4_quad (int a, int b, int c, int d, int r, int out[4]) {
  const int e0 = a + c, e1 = a - c, e2 = (b >> 1) - d, e3 = b + (d >> 1);
  int t[4] = {sext16 (e0 + e3), sext16 (e1 + e2), sext16 (e1 - e2), sext16 (e0 - e3)};
  const bool outer = (r == 0) || (r == 3);
  const bool plus = r < 2;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int s0 = quad_bcast<0> (t[i]), s1 = quad_bcast<1> (t[i]), s2 = quad_bcast<2> (t[i]), s3 = quad_bcast<3> (t[i]);
    const int f0 = s0 + s2, f1 = s0 - s2, f2 = (s1 >> 1) - s3, f3 = s1 + (s3 >> 1);
    const int A = outer ? f0 : f1, B = outer ? f3 : f2;
    out[i] = (32 + (plus ? A + B : A - B)) >> 6;
  }
}

// one 8-point butterfly of IdctResAddPred8x8_c (decode_mb_aux.cpp:79-167), int16 temporaries
__device__ __forceinline__ void idct8_1d (const int p[8], int o[8]) {
  int a0 = sext16 (p[0] + p[4]), a1 = sext16 (p[0] - p[4]);
  int a2 = sext16 (p[6] - (p[2] >> 1)), a3 = sext16 (p[2] + (p[6] >> 1));
  const int b0 = sext16 (a0 + a3), b2 = sext16 (a1 - a2), b4 = sext16 (a1 + a2), b6 = sext16 (a0 - a3);
  a0 = sext16 (-p[3] + p[5] - p[7] - (p[7] >> 1));
  a1 = sext16 (p[1] + p[7] - p[3] - (p[3] >> 1));
  a2 = sext16 (-p[1] + p[7] + p[5] + (p[5] >> 1));
  a3 = sext16 (p[3] + p[5] + p[1] + (p[1] >> 1));
  const int b1 = sext16 (a0 + (a3 >> 2)), b3 = sext16 (a1 + (a2 >> 2));
  const int b5 = sext16 (a2 - (a1 >> 2)), b7 = sext16 (a3 - (a0 >> 2));
  o[0] = sext16 (b0 + b7); o[1] = sext16 (b2 - b5); o[2] = sext16 (b4 + b3); o[3] = sext16 (b6 + b1);
  o[4] = sext16 (b6 - b1); o[5] = sext16 (b4 - b3); o[6] = sext16 (b2 + b5); o[7] = sext16 (b0 - b7);
}

__device__ __forceinline__ int tap6 (int a, int b, int c, int d, int e, int f) { return a - 5 * b + 20 * c + 20 * d - 5 * e + f; }

__device__ __forceinline__ int sum_xor (int v, int width) {   // butterfly sum inside aligned groups of `width` lanes
  for (int m = 1; m < width; m <<= 1) v += __shfl_xor (v, m);
  return v;
}

// typed views of a macroblock record staged in LDS (offsets == lh264_mb_t)
struct RecView {
  const LDS uint8_t* p;
  __device__ __forceinline__ int mb_type() const { return * (const LDS uint16_t*)p; }
  __device__ __forceinline__ int cbp() const { return p[2]; }
  __device__ __forceinline__ int qp_y() const { return p[3]; }
  __device__ __forceinline__ int qp_c (int i) const { return p[4 + i]; }
  __device__ __forceinline__ int flags() const { return p[6]; }
  __device__ __forceinline__ int intra_avail() const { return p[7]; }
  __device__ __forceinline__ int intra_mode (int i) const { return (int8_t)p[8 + i]; }
  __device__ __forceinline__ int chroma_mode() const { return (int8_t)p[24]; }
  __device__ __forceinline__ int slice_id() const { return * (const LDS uint16_t*) (p + 26); }
  __device__ __forceinline__ int sub_type (int i) const { return p[28 + i]; }
  __device__ __forceinline__ int ref_idx (int i) const { return (int8_t)p[32 + i]; }
  __device__ __forceinline__ int nzc (int i) const { return p[36 + i]; }
  __device__ __forceinline__ int mvx (int i) const { return * (const LDS int16_t*) (p + 60 + 4 * i); }
  __device__ __forceinline__ int mvy (int i) const { return * (const LDS int16_t*) (p + 62 + 4 * i); }
  __device__ __forceinline__ int ref4 (int b) const { return ref_idx (((b >> 3) << 1) + ((b & 3) >> 1)); }
  __device__ __forceinline__ int nz8 (int o) const { return nzc (o) | nzc (o + 1) | nzc (o + 4) | nzc (o + 5); }
};
// cached slice record (offsets == lh264_slice_t)
struct SliceView {
  const LDS uint8_t* p;
  __device__ __forceinline__ int slice_type() const { return p[8]; }
  __device__ __forceinline__ int deblock_idc() const { return p[9]; }
  __device__ __forceinline__ int alpha_off() const { return (int8_t)p[10]; }
  __device__ __forceinline__ int beta_off() const { return (int8_t)p[11]; }
  __device__ __forceinline__ int weighted() const { return p[12]; }
  __device__ __forceinline__ int luma_denom() const { return p[13]; }
  __device__ __forceinline__ int chroma_denom() const { return p[14]; }
  __device__ __forceinline__ int luma_weight (int i) const { return * (const LDS int16_t*) (p + 16 + 2 * i); }
  __device__ __forceinline__ int luma_offset (int i) const { return * (const LDS int16_t*) (p + 48 + 2 * i); }
  __device__ __forceinline__ int chroma_weight (int i, int c) const { return * (const LDS int16_t*) (p + 80 + 4 * i + 2 * c); }
  __device__ __forceinline__ int chroma_offset (int i, int c) const { return * (const LDS int16_t*) (p + 144 + 4 * i + 2 * c); }
  __device__ __forceinline__ int ref_slot (int i) const { return (int8_t)p[208 + i]; }
  __device__ __forceinline__ int luma_dc_weight() const { return p[224]; }
};

struct FrameCtx {
  const GLB lh264_mb_t* mbs; const GLB int16_t* coeffs; const GLB lh264_slice_t* slices;
  GLB uint8_t* dy; GLB uint8_t* du; GLB uint8_t* dv;
  int mb_w, mb_h, sy, sc, flags;
  int prev_base;             // global index of row 0 of the previous job of the chain (the only other frame that can still be in flight)
};

// Block until every global row <= g_need has been stored (rows are owned round-robin: the next unfinished row of wave
// w is w + nw * (stored[w] + 1)).
__device__ __forceinline__ void wait_prefix (const LDS WgLds& G, LDS WaveLds& L, int g_need, int nw) {
  if (__builtin_amdgcn_readfirstlane (L.known_prefix) >= g_need) return;
  volatile const LDS int* st = G.stored;
  for (;;) {
    int pre = 0x7fffffff;
    for (int w = 0; w < nw; w++) pre = min (pre, w + nw * (st[w] + 1));
    pre = __builtin_amdgcn_readfirstlane (pre) - 1;
    if (pre >= g_need) { L.known_prefix = pre; break; }
    __builtin_amdgcn_s_sleep (2);
  }
  __builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "workgroup");
}


struct Pref { v2i l, c; uint32_t rec; };   // what is fetched one macroblock ahead (per lane)

// a wave-uniform pointer, pinned to a scalar register pair: what is added to it stays a 32-bit lane offset of the load or store
// (scalar base + vector offset addressing) instead of being folded with the lane's part into a 64-bit vector address that is
// kept, or rebuilt, per macroblock
template <typename T> __device__ __forceinline__ T* sbase (T* p) { asm ("" : "+s" (p)); return p; }

__device__ __forceinline__ Pref prefetch_mb (const FrameCtx& F, int k, bool has_top, int lane) {
  Pref p;
  const GLB int16_t* cf = sbase (F.coeffs + (size_t)k * 384);
  p.l = * (const GLB v2i*) (cf + 4 * lane);
  p.c = mk2 (0, 0);
  p.rec = 0;
  if (lane < 32) {
    p.c = * (const GLB v2i*) (sbase (cf + 256) + 4 * lane);
    p.rec = ((const GLB uint32_t*)sbase (F.mbs + k))[lane];
  } else if (has_top) p.rec = ((const GLB uint32_t*)sbase (F.mbs + k - F.mb_w))[lane - 32];
  return p;
}

// ------------------------------------------------------------------------------------------------
// residual: coefficients (registers) -> R[] in LDS as int16, layout [block][row][col]
// ------------------------------------------------------------------------------------------------
__device__ LH264_PHASE void residual_phase (LDS WaveLds& L, v2i v, v2i cv, int mb_type, int cbp, bool t8, int qp, int dcw, int lane) {
  const int b = lane >> 2, r = lane & 3;
  int res[4] = {0, 0, 0, 0}, cres[4] = {0, 0, 0, 0};
  const bool i16 = mb_type == LH264_MB_I16x16;
  int c0 = sext16 (v.x), c1 = v.x >> 16, c2 = sext16 (v.y), c3 = v.y >> 16;
  int d0 = sext16 (cv.x), d1 = cv.x >> 16, d2 = sext16 (cv.y), d3 = cv.y >> 16;
  const bool have_c = (cbp >> 4) != 0;
  if (i16 || have_c) {
    // DC transforms through LDS (WelsLumaDcDequantIdct decode_slice.cpp:271-311, WelsChromaDcIdct :375-396)
    if (r == 0) { L.S[b] = c0; if (lane < 32) L.S[16 + (lane >> 2)] = d0; }
    wsync();
    if (i16 && lane < 16) {
      const int ox = (lane & 1) | ((lane >> 2) & 1) << 1, oy = ((lane >> 1) & 1) | ((lane >> 3) & 1) << 1;  // z-order -> (x,y)
      int f = 0;
#pragma unroll
      for (int jj = 0; jj < 4; jj++) {
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          // Hadamard sign patterns: row 0 ++++, 1 ++--, 2 +--+, 3 +-+-
          const int sy_ = (0xA6C0 >> (oy * 4 + jj)) & 1, sx_ = (0xA6C0 >> (ox * 4 + kk)) & 1;
          const int mv = L.S[zidx (kk, jj)];
          f += (sy_ ^ sx_) ? -mv : mv;
        }
      }
      const int na = (int) ((0x12100E0D0B0Aull >> (8 * (qp % 6))) & 0xff);      // 10 11 13 14 16 18
      const int dq = na << (qp / 6);
      const int qmul = dcw == 16 ? dq : ((dcw * dq) >> 4);
      L.S[32 + lane] = sext16 ((f * qmul + 2) >> 2);
    }
    if (have_c && lane >= 16 && lane < 24) {
      const int p = (lane - 16) >> 2, i = lane & 3;
      const int a = L.S[16 + p * 4], bb = L.S[16 + p * 4 + 1], c = L.S[16 + p * 4 + 2], d = L.S[16 + p * 4 + 3];
      const int s0 = a + bb, dd0 = a - bb, s1 = c + d, dd1 = c - d;
      const int o = i == 0 ? s0 + s1 : i == 1 ? dd0 + dd1 : i == 2 ? s0 - s1 : dd0 - dd1;
      L.S[48 + (lane - 16)] = sext16 (o >> 1);
    }
    wsync();
    if (r == 0) { if (i16) c0 = L.S[32 + b]; if (have_c && lane < 32) d0 = L.S[48 + (lane >> 2)]; }
    wsync();
  }
  if (!t8) idct4x4_quad (c0, c1, c2, c3, r, res);
  else {
    // 8x8 transform through LDS: the MB's luma coefficients already sit row-major per 8x8 block
    * (LDS v2i*) (L.R + 4 * lane) = v;
    wsync();
    if (lane < 32) {              // rows
      int p[8], o[8];
#pragma unroll
      for (int i = 0; i < 8; i++) p[i] = L.R[lane * 8 + i];
      idct8_1d (p, o);
#pragma unroll
      for (int i = 0; i < 8; i++) L.R[lane * 8 + i] = (int16_t)o[i];
    }
    wsync();
    if (lane < 32) {              // columns
      const int blk = lane >> 3, col = lane & 7;
      int p[8], o[8];
#pragma unroll
      for (int i = 0; i < 8; i++) p[i] = L.R[blk * 64 + i * 8 + col];
      idct8_1d (p, o);
#pragma unroll
      for (int i = 0; i < 8; i++) L.R[blk * 64 + i * 8 + col] = (int16_t)o[i];
    }
    wsync();
    const int bx = (b & 1) | ((b >> 2) & 1) << 1, by = ((b >> 1) & 1) | ((b >> 3) & 1) << 1;
    const int ly = 4 * by + r, lx0 = 4 * bx;
    const int i8 = (ly >> 3) * 2 + (lx0 >> 3);
#pragma unroll
    for (int i = 0; i < 4; i++) res[i] = (32 + L.R[i8 * 64 + (ly & 7) * 8 + (lx0 & 7) + i]) >> 6;
    wsync();
  }
  if (have_c) idct4x4_quad (d0, d1, d2, d3, r, cres);
  * (LDS v2i*) (L.R + 4 * lane) = mk2 ((res[0] & 0xffff) | (res[1] << 16), (res[2] & 0xffff) | (res[3] << 16));
  if (lane < 32) * (LDS v2i*) (L.R + 256 + 4 * lane) = mk2 ((cres[0] & 0xffff) | (cres[1] << 16), (cres[2] & 0xffff) | (cres[3] << 16));
  wsync();
}

__device__ __forceinline__ void zero_residual (LDS WaveLds& L, int lane) {
  * (LDS v2i*) (L.R + 4 * lane) = mk2 (0, 0);
  if (lane < 32) * (LDS v2i*) (L.R + 256 + 4 * lane) = mk2 (0, 0);
  wsync();
}

// residual of this lane's 4-sample strip (luma layout: lane = 4*b + r ; chroma layout lanes 0..31)
__device__ __forceinline__ void load_res4 (const LDS int16_t* R, int lane, int out[4]) {
  const v2i v = * (const LDS v2i*) (R + 4 * lane);
  out[0] = sext16 (v.x); out[1] = v.x >> 16; out[2] = sext16 (v.y); out[3] = v.y >> 16;
}
__device__ __forceinline__ uint32_t pack_add4 (const int pr[4], const int rs[4]) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) o |= (uint32_t)clip_u8 (pr[i] + rs[i]) << (8 * i);
  return o;
}

// ------------------------------------------------------------------------------------------------
// intra prediction
// ------------------------------------------------------------------------------------------------
// I4x4 directional prediction of one sample from the edge e[0..12] = L3 L2 L1 L0 TL T0..T7
// (get_intra_predictor.cpp:54-380).  hi = 12, or 8 for the *_TOP variants (p[3,-1] replicated).
__device__ __forceinline__ int edge4_load (const LDS uint8_t* T, int bx, int by, int j, int hi) {
  j = clip3 (j, 0, hi);
  const int r = (j < 4) ? (4 * by + 3 - j) : (4 * by - 1);
  const int c = (j < 4) ? (4 * bx - 1) : (4 * bx + j - 5);
  return T[tY (r, c)];
}

__device__ __forceinline__ int pred4_dir (const LDS uint8_t* T, int bx, int by, int mode, int x, int y) {
  int k, three = 1, hi = 12;
  switch (mode) {
  case LH264_I4_DDL_TOP: hi = 8;    // fall through
  case LH264_I4_DDL: k = x + y + 6; break;
  case LH264_I4_DDR: k = 4 + x - y; break;
  case LH264_I4_VR: {
    const int z = 2 * x - y;
    if (z >= 0) { k = 4 + x - (y >> 1); three = z & 1; }
    else if (z == -1) k = 4;
    else k = 5 - y;
    break;
  }
  case LH264_I4_HD: {
    const int z = 2 * y - x;
    if (z >= 0) { k = 4 - (y - (x >> 1)); three = z & 1; if (!three) k -= 1; }
    else if (z == -1) k = 4;
    else k = 3 + x;
    break;
  }
  case LH264_I4_VL_TOP: hi = 8;     // fall through
  case LH264_I4_VL: { const int kk = x + (y >> 1); three = y & 1; k = three ? kk + 6 : kk + 5; break; }
  default: /* HU */ { const int z = x + 2 * y; const int a = z >> 1; three = z & 1; k = 2 - a; break; }
  }
  if (three) {
    const int e0 = edge4_load (T, bx, by, k - 1, hi), e1 = edge4_load (T, bx, by, k, hi), e2 = edge4_load (T, bx, by, k + 1, hi);
    return (e0 + 2 * e1 + e2 + 2) >> 2;
  }
  const int e0 = edge4_load (T, bx, by, k, hi), e1 = edge4_load (T, bx, by, k + 1, hi);
  return (e0 + e1 + 1) >> 1;
}

// RecI4x4Luma rec_mb.cpp:124-157, one lane per sample.  The reference walks the 16 blocks in z-order; a block reads its left, top,
// top-left and - where H.264 calls it available, i.e. where it comes earlier in z-order - top-right neighbour block.  All of those have a
// smaller bx + 2 by, so the blocks of one anti-diagonal bx + 2 by = t are independent of each other: 10 steps of one or two blocks (lanes
// 0..15 and 16..31) instead of 16 steps of one.  (A block whose top-right neighbour is NOT available was given a *_TOP mode by the
// parser, parse_mb_syn_cavlc.cpp:519-611, and does not look at it - that it may already be there in this order does not matter.)
__device__ LH264_PHASE void intra4x4_phase (LDS WaveLds& L, RecView m, int lane) {
  LDS uint8_t* T = L.T;
  const int half = (lane >> 4) & 1, x = lane & 3, y = (lane >> 2) & 3;
  for (int t = 0; t < 10; t++) {
    // blocks on this anti-diagonal: by from max (0, ceil ((t - 3) / 2)) to min (3, t / 2); at most two
    const int by0 = t <= 3 ? 0 : (t - 2) >> 1;
    const int by1 = min (3, t >> 1);
    const int qy = by0 + half, qx = t - 2 * qy;
    const bool act = lane < 32 && qy <= by1 && qx >= 0 && qx <= 3;
    if (act) {
      const int mode = m.intra_mode (qy * 4 + qx);
      int v;
      if (mode == LH264_I4_V) v = T[tY (4 * qy - 1, 4 * qx + x)];
      else if (mode == LH264_I4_H) v = T[tY (4 * qy + y, 4 * qx - 1)];
      else if (mode == LH264_I4_DC || mode == LH264_I4_DC_L || mode == LH264_I4_DC_T) {
        int s = 0;
        if (mode != LH264_I4_DC_L) {
          const uint32_t tw = * (const LDS uint32_t*)&T[tY (4 * qy - 1, 4 * qx)];
          s += (tw & 0xff) + ((tw >> 8) & 0xff) + ((tw >> 16) & 0xff) + (tw >> 24);
        }
        if (mode != LH264_I4_DC_T)
          s += (int)T[tY (4 * qy, 4 * qx - 1)] + (int)T[tY (4 * qy + 1, 4 * qx - 1)] + (int)T[tY (4 * qy + 2, 4 * qx - 1)] + (int)T[tY (4 * qy + 3, 4 * qx - 1)];
        v = (mode == LH264_I4_DC) ? (s + 4) >> 3 : (s + 2) >> 2;
      } else if (mode == LH264_I4_DC_128) v = 128;
      else v = pred4_dir (T, qx, qy, mode, x, y);
      const int rr = L.R[zidx (qx, qy) * 16 + y * 4 + x];
      T[tY (4 * qy + y, 4 * qx + x)] = (uint8_t)clip_u8 (v + rr);
    }
    wsync();
  }
}

// RecI8x8Luma rec_mb.cpp:70-115 (reference-sample low-pass 8.3.2.2.1; get_intra_predictor.cpp:382-880)
__device__ LH264_PHASE void intra8x8_phase (LDS WaveLds& L, RecView m, int lane) {
  LDS uint8_t* T = L.T;
  const int av = uni (m.intra_avail());
  for (int i8 = 0; i8 < 4; i8++) {
    const int ox = (i8 & 1) * 8, oy = (i8 >> 1) * 8;
    const int mode = uni (m.intra_mode (((i8 >> 1) << 3) + ((i8 & 1) << 1)));
    int tl = i8 == 0 ? !! (av & LH264_AVAIL_TL) : i8 == 1 ? !! (av & LH264_AVAIL_T) : i8 == 2 ? !! (av & LH264_AVAIL_L) : 1;
    const int tr = i8 == 0 ? !! (av & LH264_AVAIL_T) : i8 == 1 ? !! (av & LH264_AVAIL_TR) : i8 == 2 ? 1 : 0;
    const bool need_top = !(mode == LH264_I4_H || mode == LH264_I4_DC_L || mode == LH264_I4_DC_128 || mode == LH264_I4_HU);
    const bool need_left = !(mode == LH264_I4_V || mode == LH264_I4_DC_T || mode == LH264_I4_DC_128 || mode == LH264_I4_DDL ||
                             mode == LH264_I4_DDL_TOP || mode == LH264_I4_VL || mode == LH264_I4_VL_TOP);
    const bool full_tr = (mode == LH264_I4_DDL || mode == LH264_I4_VL);
    const bool corner = (mode == LH264_I4_DDR || mode == LH264_I4_VR || mode == LH264_I4_HD);
    const bool top_var = (mode == LH264_I4_DDL_TOP || mode == LH264_I4_VL_TOP);
    if (corner) tl = 1;
    // filtered edge E[0..24] = L'7..L'0, TL', T'0..T'15
    if (lane < 25) {
      int val = 0;
      const int TLv = tl ? T[tY (oy - 1, ox - 1)] : 0;
      if (lane < 8) {                 // L'[7-lane]
        const int i = 7 - lane;
        if (need_left) {
          const int l0 = T[tY (oy + i, ox - 1)];
          const int lm = i > 0 ? T[tY (oy + i - 1, ox - 1)] : TLv;
          const int lp = i < 7 ? T[tY (oy + i + 1, ox - 1)] : l0;
          if (i == 0) val = tl ? (TLv + 2 * l0 + lp + 2) >> 2 : (3 * l0 + lp + 2) >> 2;
          else val = (lm + 2 * l0 + lp + 2) >> 2;      // i == 7: lp == l0 -> (L6 + 3 L7 + 2) >> 2
        }
      } else if (lane == 8) {
        if (corner) val = ((int)T[tY (oy, ox - 1)] + 2 * TLv + (int)T[tY (oy - 1, ox)] + 2) >> 2;
      } else if (need_top) {
        const int i = lane - 9;       // T'[i]
        const bool t8real = tr && !top_var;
        // raw top samples with the reference's substitution rules
        auto rawT = [&] (int q) -> int {
          if (q < 8) return T[tY (oy - 1, ox + q)];
          if (full_tr) return T[tY (oy - 1, ox + q)];
          if (t8real && q == 8) return T[tY (oy - 1, ox + 8)];
          return T[tY (oy - 1, ox + 7)];
        };
        if (full_tr) {
          if (i == 0) val = tl ? (TLv + 2 * rawT (0) + rawT (1) + 2) >> 2 : (3 * rawT (0) + rawT (1) + 2) >> 2;
          else if (i == 15) val = (rawT (14) + 3 * rawT (15) + 2) >> 2;
          else val = (rawT (i - 1) + 2 * rawT (i) + rawT (i + 1) + 2) >> 2;
        } else {
          if (i == 0) val = tl ? (TLv + 2 * rawT (0) + rawT (1) + 2) >> 2 : (3 * rawT (0) + rawT (1) + 2) >> 2;
          else if (i < 7) val = (rawT (i - 1) + 2 * rawT (i) + rawT (i + 1) + 2) >> 2;
          else if (i == 7) val = t8real ? (rawT (6) + 2 * rawT (7) + rawT (8) + 2) >> 2 : (rawT (6) + 3 * rawT (7) + 2) >> 2;
          else val = rawT (7);
        }
      }
      L.E[lane] = (uint8_t)val;
    }
    wsync();
    {
      const int x = lane & 7, y = lane >> 3;
      const LDS uint8_t* E = L.E;
      int v;
      auto f3 = [&] (int kk) -> int { const int lo = clip3 (kk - 1, 0, 24), mid = clip3 (kk, 0, 24), hi = clip3 (kk + 1, 0, 24); return (E[lo] + 2 * E[mid] + E[hi] + 2) >> 2; };
      auto f2 = [&] (int kk) -> int { return (E[clip3 (kk, 0, 24)] + E[clip3 (kk + 1, 0, 24)] + 1) >> 1; };
      switch (mode) {
      case LH264_I4_V: v = E[9 + x]; break;
      case LH264_I4_H: v = E[7 - y]; break;
      case LH264_I4_DC: case LH264_I4_DC_L: case LH264_I4_DC_T: {
        int term = 0;
        if (lane < 8) term = (mode == LH264_I4_DC_T) ? 0 : E[lane];
        else if (lane < 16) term = (mode == LH264_I4_DC_L) ? 0 : E[9 + lane - 8];
        term = sum_xor (term, 16);
        const int s = __builtin_amdgcn_readlane (term, 0);
        v = (mode == LH264_I4_DC) ? (s + 8) >> 4 : (s + 4) >> 3;
        break;
      }
      case LH264_I4_DC_128: v = 128; break;
      case LH264_I4_DDL: case LH264_I4_DDL_TOP: v = f3 (9 + x + y + 1); break;
      case LH264_I4_DDR: v = f3 (8 + x - y); break;
      case LH264_I4_VR: {
        const int z = 2 * x - y;
        if (z >= 0) { const int kk = 8 + x - (y >> 1); v = (z & 1) ? f3 (kk) : f2 (kk); }
        else if (z == -1) v = f3 (8);
        else v = f3 (9 - y + 2 * x);
        break;
      }
      case LH264_I4_HD: {
        const int z = 2 * y - x;
        if (z >= 0) { const int kk = 8 - (y - (x >> 1)); v = (z & 1) ? f3 (kk) : f2 (kk - 1); }
        else if (z == -1) v = f3 (8);
        else v = f3 (7 + x - 2 * y);
        break;
      }
      case LH264_I4_VL: case LH264_I4_VL_TOP: { const int kk = 9 + x + (y >> 1); v = (y & 1) ? f3 (kk + 1) : f2 (kk); break; }
      default: { const int z = x + 2 * y, a = z >> 1; v = (z & 1) ? f3 (6 - a) : f2 (6 - a); break; }   // HU
      }
      const int X = ox + x, Y = oy + y;
      const int rr = L.R[zidx (X >> 2, Y >> 2) * 16 + (Y & 3) * 4 + (X & 3)];
      wsync();
      T[tY (Y, X)] = (uint8_t)clip_u8 (v + rr);
    }
    wsync();
  }
}

// RecI16x16Mb rec_mb.cpp:179-230 (luma part), lane = 4*b + r strip layout
__device__ LH264_PHASE void intra16_phase (LDS WaveLds& L, int mode, int lane) {
  LDS uint8_t* T = L.T;
  const int b = lane >> 2, r = lane & 3;
  const int bx = (b & 1) | ((b >> 2) & 1) << 1, by = ((b >> 1) & 1) | ((b >> 3) & 1) << 1;
  const int ly = 4 * by + r, lx0 = 4 * bx;
  int pr[4], res[4];
  load_res4 (L.R, lane, res);
  if (mode == LH264_I16_V) {
    const uint32_t t = * (const LDS uint32_t*)&T[tY (-1, lx0)];
#pragma unroll
    for (int i = 0; i < 4; i++) pr[i] = (t >> (8 * i)) & 0xff;
  } else if (mode == LH264_I16_H) {
    const int l = T[tY (ly, -1)];
#pragma unroll
    for (int i = 0; i < 4; i++) pr[i] = l;
  } else if (mode == LH264_I16_P) {
    int term = 0;
    if (lane < 8) term = (lane + 1) * ((int)T[tY (-1, 8 + lane)] - (int)T[tY (-1, 6 - lane)]);
    else if (lane < 16) { const int i = lane - 8; term = (i + 1) * ((int)T[tY (8 + i, -1)] - (int)T[tY (6 - i, -1)]); }
    term = sum_xor (term, 8);
    const int H = __builtin_amdgcn_readlane (term, 0), V = __builtin_amdgcn_readlane (term, 8);
    const int a = ((int)T[tY (15, -1)] + (int)T[tY (-1, 15)]) << 4;
    const int bb = (5 * H + 32) >> 6, c = (5 * V + 32) >> 6;
#pragma unroll
    for (int i = 0; i < 4; i++) pr[i] = clip_u8 ((a + bb * (lx0 + i - 7) + c * (ly - 7) + 16) >> 5);
  } else {
    int v = 128;
    if (mode != LH264_I16_DC_128) {
      int term = 0;
      if (lane < 16) term = (mode == LH264_I16_DC_L) ? 0 : T[tY (-1, lane)];
      else if (lane < 32) term = (mode == LH264_I16_DC_T) ? 0 : T[tY (lane - 16, -1)];
      term = sum_xor (term, 32);
      const int s = __builtin_amdgcn_readlane (term, 0);
      v = (mode == LH264_I16_DC) ? (s + 16) >> 5 : (s + 8) >> 4;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) pr[i] = v;
  }
  const uint32_t o = pack_add4 (pr, res);
  wsync();
  * (LDS uint32_t*)&T[tY (ly, lx0)] = o;
}

// RecI4x4Chroma rec_mb.cpp:160-177 (prediction) + RecChroma :547-575 (residual): lanes 0..31
__device__ LH264_PHASE void intra_chroma_phase (LDS WaveLds& L, int mode, int lane) {
  const int r = lane & 3;
  const int cp = (lane >> 4) & 1, cj = (lane >> 2) & 3;
  const int cy = 4 * (cj >> 1) + r, cx0 = 4 * (cj & 1);
  const LDS uint8_t* Cc = L.C[cp];
  int pr[4] = {128, 128, 128, 128}, cres[4];
  load_res4 (L.R + 256, lane & 31, cres);
  const int q = lane & 15;
  if (mode == LH264_C_V) {
    const uint32_t t = * (const LDS uint32_t*)&Cc[tC (-1, cx0)];
#pragma unroll
    for (int i = 0; i < 4; i++) pr[i] = (t >> (8 * i)) & 0xff;
  } else if (mode == LH264_C_H) {
    const int l = Cc[tC (cy, -1)];
#pragma unroll
    for (int i = 0; i < 4; i++) pr[i] = l;
  } else if (mode == LH264_C_P) {
    int term = 0;
    if (q < 4) term = (q + 1) * ((int)Cc[tC (-1, 4 + q)] - (int)Cc[tC (-1, 2 - q)]);
    else if (q < 8) { const int i = q - 4; term = (i + 1) * ((int)Cc[tC (4 + i, -1)] - (int)Cc[tC (2 - i, -1)]); }
    term = sum_xor (term, 4);
    const int H = __shfl (term, (lane & 48) + 0), V = __shfl (term, (lane & 48) + 4);
    const int a = ((int)Cc[tC (7, -1)] + (int)Cc[tC (-1, 7)]) << 4;
    const int bb = (17 * H + 16) >> 5, c = (17 * V + 16) >> 5;
#pragma unroll
    for (int i = 0; i < 4; i++) pr[i] = clip_u8 ((a + bb * (cx0 + i - 3) + c * (cy - 3) + 16) >> 5);
  } else if (mode != LH264_C_DC_128) {
    int term = (q < 8) ? (int)Cc[tC (-1, q)] : (int)Cc[tC (q - 8, -1)];
    term = sum_xor (term, 4);
    const int base = lane & 48;
    const int t0 = __shfl (term, base + 0), t1 = __shfl (term, base + 4), l0 = __shfl (term, base + 8), l1 = __shfl (term, base + 12);
    int v;
    const bool rightq = cx0 >= 4, lowq = cy >= 4;
    if (mode == LH264_C_DC) v = !rightq && !lowq ? (t0 + l0 + 4) >> 3 : rightq && !lowq ? (t1 + 2) >> 2 : !rightq ? (l1 + 2) >> 2 : (t1 + l1 + 4) >> 3;
    else if (mode == LH264_C_DC_L) v = lowq ? (l1 + 2) >> 2 : (l0 + 2) >> 2;
    else v = rightq ? (t1 + 2) >> 2 : (t0 + 2) >> 2;
#pragma unroll
    for (int i = 0; i < 4; i++) pr[i] = v;
  }
  const uint32_t o = pack_add4 (pr, cres);
  wsync();
  if (lane < 32) * (LDS uint32_t*)&L.C[cp][tC (cy, cx0)] = o;
}

// ------------------------------------------------------------------------------------------------
// motion compensation straight from the padded reference planes (mc.cpp:142-380)
// ------------------------------------------------------------------------------------------------
// Reference fetches are issued as whole 16-byte (luma) / 8-byte (chroma) aligned rows up front, for every row the
// macroblock can need, and the interpolation works on registers afterwards: one exposed memory latency per macroblock
// instead of one per filter stage.  Row12 = 12 consecutive bytes starting at an unaligned address.
typedef uint32_t v4u __attribute__ ((ext_vector_type (4)));
typedef uint32_t v2u __attribute__ ((ext_vector_type (2)));
struct Row12 { uint32_t w0, w1, w2; };
__device__ __forceinline__ Row12 align12 (v4u d, int sh) {
  Row12 o;
  o.w0 = __builtin_amdgcn_alignbyte (d.y, d.x, sh);
  o.w1 = __builtin_amdgcn_alignbyte (d.z, d.y, sh);
  o.w2 = __builtin_amdgcn_alignbyte (d.w, d.z, sh);
  return o;
}
#define BYTE(w, i) (int) (((w) >> (8 * (i))) & 0xff)
// byte i (0..11, compile-time) of a Row12
#define RB(R, i) ((i) < 4 ? BYTE ((R).w0, (i)) : (i) < 8 ? BYTE ((R).w1, (i) - 4) : BYTE ((R).w2, (i) - 8))

// The 6-tap filter (1,-5,20,20,-5,1) on bytes without unpacking them one by one.
// Horizontal: the six samples of an output are consecutive bytes - two signed 4x8-bit dot products (v_dot4c_i32_i8) on the row
// with 128 subtracted from every sample (the taps sum to 32, so 4096 goes back in).  Vertical: the same byte position of six
// rows - two adjacent columns of a row are picked into one 2x16-bit word (v_perm_b32) and the filter runs on 16-bit pairs
// (v_pk_*); the sums stay within int16 (|sum| <= 10,710).
typedef short s16x2 __attribute__ ((ext_vector_type (2)));
__device__ __forceinline__ s16x2 as_s2 (uint32_t v) { return __builtin_bit_cast (s16x2, v); }
__device__ __forceinline__ uint32_t as_u (s16x2 v) { return __builtin_bit_cast (uint32_t, v); }
// horizontal taps at outputs 0..3 of a row (output i = samples i..i+5), each with `bias` added
__device__ __forceinline__ void htap4 (const Row12 R, int bias, int out[4]) {
  const uint32_t s0 = R.w0 ^ 0x80808080u, s1 = R.w1 ^ 0x80808080u, s2 = R.w2 ^ 0x80808080u;
  const int ca = 0x1414FB01, cb = 0x000001FB;       // bytes (1, -5, 20, 20) and (-5, 1, 0, 0)
  out[0] = __builtin_amdgcn_sdot4 ((int)s0, ca, __builtin_amdgcn_sdot4 ((int)s1, cb, 4096 + bias, false), false);
#pragma unroll
  for (int i = 1; i < 4; i++)
    out[i] = __builtin_amdgcn_sdot4 ((int)__builtin_amdgcn_alignbyte (s1, s0, i), ca,
                                     __builtin_amdgcn_sdot4 ((int)__builtin_amdgcn_alignbyte (s2, s1, i), cb, 4096 + bias, false), false);
}
// bytes a, a + 1 (compile-time) of the eight bytes hi:lo as a 16-bit pair (v_perm_b32: selector 0x0c gives a zero byte)
#define PAIR16(hi, lo, a) __builtin_amdgcn_perm ((hi), (lo), 0x0c000c00u | (uint32_t) ((a) + 1) << 16 | (uint32_t) (a))
// vertical taps of two adjacent columns of six rows (p_k = the two samples of row k as a 16-bit pair), on 16-bit pairs (v_pk_*)
__device__ __forceinline__ s16x2 vtap_pair (uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t p4, uint32_t p5) {
  const s16x2 k20 = {20, 20}, k5 = {5, 5};
  return (as_s2 (p2) + as_s2 (p3)) * k20 + (as_s2 (p0) + as_s2 (p5)) - (as_s2 (p1) + as_s2 (p4)) * k5;
}
#define VTAP_PAIR(R, hi, lo, a) vtap_pair (PAIR16 (R[0].hi, R[0].lo, a), PAIR16 (R[1].hi, R[1].lo, a), PAIR16 (R[2].hi, R[2].lo, a), \
                                           PAIR16 (R[3].hi, R[3].lo, a), PAIR16 (R[4].hi, R[4].lo, a), PAIR16 (R[5].hi, R[5].lo, a))
// clip_u8 (v >> 5) of both halves of a pair (the rounding 16 already added): bytes 0 and 2 of the result, bytes 1 and 3 zero
__device__ __forceinline__ uint32_t shr5_clip_pair (s16x2 v) {
  const s16x2 z = {0, 0}, m = {255, 255};
  return as_u (__builtin_elementwise_min (__builtin_elementwise_max (v >> 5, z), m));
}
// bytes 0 and 2 of lo, then bytes 0 and 2 of hi: two clipped pairs -> four samples
__device__ __forceinline__ uint32_t pack_pairs (uint32_t hi, uint32_t lo) { return __builtin_amdgcn_perm (hi, lo, 0x06040200u); }

// one 4x1 luma strip from the fetched rows, as four bytes: R[k] holds samples -2..9 of row k-2 relative to the strip's first
// sample (McLuma_c / McHorVer* common/src/mc.cpp:142-380).  With any_fy false (no strip of the wave has a vertical fraction) only
// R[2] is defined.
// By STAGES, not by fraction classes: the strips of a wave differ in their fractions (a macroblock of several partitions), and a
// branch per class makes the wave pay the sum of its classes.  Each stage is computed by all lanes together behind one wave-uniform
// test and skipped when no lane needs it:
//   H  fx != 0            the horizontal half samples of row 2 (row 3 where fy == 3): positions a b c and the b / s term of e g p r f q
//   V  fy != 0            vertical sums (int16, as the reference keeps them) of columns 2..5: d h n, the h / m term of e p i
//   X  both fractions     columns 6, 7: the m term of g r k
//   J  both, one of them 2: columns 0, 1, 8 and the four horizontal taps over the nine sums: j and the j term of f q i k
// Every position is (A + B + 1) >> 1 of two of those four-byte terms (A == B: the term itself), so the stages only select A and B
// per lane and one v_lerp_u8 finishes the strip.
__device__ __forceinline__ uint32_t mc_luma_rows (const Row12 R[6], int fx, int fy, bool any_fy) {
  const uint32_t G = __builtin_amdgcn_alignbyte (R[2].w1, R[2].w0, 2);      // the integer samples
  uint32_t A = G, B = G;
  if (__ballot (fx != 0)) {                         // ---- H
    Row12 H = R[2];
    if (fy == 3) H = R[3];
    int t[4];
    htap4 (H, 16, t);
    const s16x2 t01 = {(short)t[0], (short)t[1]}, t23 = {(short)t[2], (short)t[3]};      // |sum + 16| <= 10,726
    const uint32_t HH = pack_pairs (shr5_clip_pair (t23), shr5_clip_pair (t01));
    A = fx != 0 ? HH : A;
    B = fx == 2 ? HH : fx == 3 ? __builtin_amdgcn_alignbyte (R[2].w1, R[2].w0, 3) : B;
  }
  if (any_fy) {                                     // ---- V
    const s16x2 k16 = {16, 16};
    const s16x2 P = VTAP_PAIR (R, w1, w0, 2), Q = VTAP_PAIR (R, w1, w0, 4);       // columns 2, 3 and 4, 5
    const uint32_t VV0 = pack_pairs (shr5_clip_pair (Q + k16), shr5_clip_pair (P + k16));
    uint32_t VVx = VV0;
    const bool both = fx != 0 && fy != 0;
    if (__ballot (both)) {                          // ---- X
      const s16x2 E = VTAP_PAIR (R, w2, w1, 2);     // columns 6, 7
      VVx = fx == 3 ? __builtin_amdgcn_alignbyte (shr5_clip_pair (E + k16), VV0, 1) : VV0;
      const bool isj = both && (fx == 2 || fy == 2);
      if (__ballot (isj)) {                         // ---- J
        const s16x2 Z = VTAP_PAIR (R, w1, w0, 0);   // columns 0, 1
        const uint32_t M = 0xffu;
        const s16x2 W = vtap_pair (R[0].w2 & M, R[1].w2 & M, R[2].w2 & M, R[3].w2 & M, R[4].w2 & M, R[5].w2 & M);       // column 8
        // the horizontal taps over the nine sums, in int32 as the reference has them
        const int vs[9] = {Z.x, Z.y, P.x, P.y, Q.x, Q.y, E.x, E.y, W.x};
        const int j0 = tap6 (vs[0], vs[1], vs[2], vs[3], vs[4], vs[5]) + 512, j1 = tap6 (vs[1], vs[2], vs[3], vs[4], vs[5], vs[6]) + 512;
        const int j2 = tap6 (vs[2], vs[3], vs[4], vs[5], vs[6], vs[7]) + 512, j3 = tap6 (vs[3], vs[4], vs[5], vs[6], vs[7], vs[8]) + 512;
        // clipped as 16-bit pairs like the other terms (-300 < j >> 10 < 600).  Not as clip_u8 (j0 >> 10) | clip_u8 (j1 >> 10) << 8:
        // hipcc turns that into v_ashr_pk_u8_i32 and ORs bytes 2, 3 into its result register, whose upper half the instruction was seen to
        // leave as it was (stale on an MI355X: wrong samples 2 and 3)
        const s16x2 z = {0, 0}, m = {255, 255};
        const s16x2 j01 = {(short) (j0 >> 10), (short) (j1 >> 10)}, j23 = {(short) (j2 >> 10), (short) (j3 >> 10)};
        const uint32_t J = pack_pairs (as_u (__builtin_elementwise_min (__builtin_elementwise_max (j23, z), m)),
                                       as_u (__builtin_elementwise_min (__builtin_elementwise_max (j01, z), m)));
        A = isj ? J : A;
        B = (fx == 2 && fy == 2) ? J : B;
      }
    }
    // fx == 0: d h n = the vertical half sample with G (row 2), itself, or row 3; both fractions: fx == 2 keeps what H / J chose (the
    // horizontal half sample, or j), odd fx takes the vertical half sample of column fx >> 1
    const uint32_t Bv = fx == 0 ? (fy == 2 ? VV0 : fy == 3 ? __builtin_amdgcn_alignbyte (R[3].w1, R[3].w0, 2) : G) : (fx == 2 ? B : VVx);
    B = fy != 0 ? Bv : B;
    A = (fy != 0 && fx == 0) ? VV0 : A;
  }
  return __builtin_amdgcn_lerp (A, B, 0x01010101u);   // per byte (A + B + 1) >> 1
}

// two horizontally adjacent chroma samples sharing one motion vector (a 4x4 luma block = 2x2 chroma); a / b = the
// 4 bytes starting at the pair's first sample in rows 0 / 1 (McChroma_c mc.cpp)
__device__ __forceinline__ void mc_chroma_rows (uint32_t a, uint32_t b, int dx, int dy, int& o0, int& o1) {
  if ((dx | dy) == 0) { o0 = BYTE (a, 0); o1 = BYTE (a, 1); return; }
  // the four weights (each <= 64) as bytes, the four samples of an output as bytes: one unsigned 4x8-bit dot product each
  const uint32_t wgt = (uint32_t) ((8 - dx) * (8 - dy)) | (uint32_t) (dx * (8 - dy)) << 8 | (uint32_t) ((8 - dx) * dy) << 16 | (uint32_t) (dx * dy) << 24;
  o0 = (int) (__builtin_amdgcn_udot4 ((a & 0xffffu) | (b << 16), wgt, 32u, false) >> 6);
  o1 = (int) (__builtin_amdgcn_udot4 (((a >> 8) & 0xffffu) | ((b >> 8) << 16), wgt, 32u, false) >> 6);
}

// partition geometry of the 4x4 block (bx,by): origin and size of the motion partition that holds it
__device__ __forceinline__ void partition_of (int mb_type, RecView m, int bx, int by, int& ox, int& oy, int& pw, int& ph) {
  ox = oy = 0; pw = ph = 16;
  if (mb_type == LH264_MB_P16x8) { ph = 8; oy = (by >> 1) << 3; }
  else if (mb_type == LH264_MB_P8x16) { pw = 8; ox = (bx >> 1) << 3; }
  else if (mb_type == LH264_MB_P8x8 || mb_type == LH264_MB_P8x8REF0) {
    const int q = ((by >> 1) << 1) | (bx >> 1);
    const int st = m.sub_type (q);
    ox = (bx >> 1) << 3; oy = (by >> 1) << 3; pw = ph = 8;
    if (st == LH264_SUB_8x4) { ph = 4; oy += (by & 1) << 2; }
    else if (st == LH264_SUB_4x8) { pw = 4; ox += (bx & 1) << 2; }
    else if (st == LH264_SUB_4x4) { pw = ph = 4; ox += (bx & 1) << 2; oy += (by & 1) << 2; }
  }
}

// The frame context comes from the frame's LDS block (FrameLds), read here with LDS-qualified loads and made scalar: a reference
// to the caller's FrameCtx would turn every field access in this non-inlined function into a scratch load followed by
// "s_waitcnt vmcnt(0)", which also drains the reference fetches in flight, and passing it by value cost the caller 17 moves into
// argument registers per macroblock.
struct InterCtx { int sy, sc, mb_w, mb_h; };

// GetInterPred rec_mb.cpp:344-545, BaseMC :247-274, WeightPrediction :276-341 (+ residual add)
__device__ LH264_PHASE void inter_phase (LDS WaveLds& L, const LDS WgLds& G, const LDS FrameLds& FR, RecView m, SliceView sl, int mb_type,
                                          int mbx, int mby, bool has_res, int lane) {
  InterCtx F;
  F.sy = uni (FR.sy); F.sc = uni (FR.sc); F.mb_w = uni (FR.mb_w); F.mb_h = uni (FR.mb_h);
  const uint64_t prev_dy = FR.prev_dy;
  const int b = lane >> 2, r = lane & 3;
  const int bx = (b & 1) | ((b >> 2) & 1) << 1, by = ((b >> 1) & 1) | ((b >> 3) & 1) << 1;
  const int ly = 4 * by + r, lx0 = 4 * bx;
  const int cp = (lane >> 4) & 1, cj = (lane >> 2) & 3;
  const int cy = 4 * (cj >> 1) + r, cx0 = 4 * (cj & 1);
  int need = -0x7fffffff;
  if (lane < 16) {
    const int qx = lane & 3, qy = lane >> 2;      // raster 4x4 block
    int ox, oy, pw, ph;
    partition_of (mb_type, m, qx, qy, ox, oy, pw, ph);
    const int pb = (oy >> 2) * 4 + (ox >> 2);     // raster index of the partition's first block (its MV)
    const int W = F.mb_w * 16, Hh = F.mb_h * 16;
    int fx = ((mbx * 16 + ox) << 2) + m.mvx (pb);
    int fy = ((mby * 16 + oy) << 2) + m.mvy (pb);
    fx = clip3 (fx, (-LH264_PAD_LUMA + 2) * 4, (W + LH264_PAD_LUMA - 19) * 4);
    fy = clip3 (fy, (-LH264_PAD_LUMA + 2) * 4, (Hh + LH264_PAD_LUMA - 19) * 4);
    const int ridx = m.ref_idx (((qy >> 1) << 1) + (qx >> 1));
    int slot = (ridx >= 0 && ridx < LH264_MAX_REFS) ? sl.ref_slot (ridx) : -1;
    if (slot < 0) slot = sl.ref_slot (0);          // rec_mb.cpp:238-242: missing picture -> list entry 0
    if (slot < 0) slot = 0;
    // integer sample position of this 4x4 block's first pixel in the reference planes
    const int sx = (fx >> 2) + (qx * 4 - ox), syy = (fy >> 2) + (qy * 4 - oy);
    const int cxs = (fx >> 3) + ((qx * 4 - ox) >> 1), cys = (fy >> 3) + ((qy * 4 - oy) >> 1);
    L.mvi[lane][0] = syy * F.sy + sx;
    L.mvi[lane][1] = cys * F.sc + cxs;
    L.mvi[lane][2] = (fx & 3) | (fy & 3) << 2 | (fx & 7) << 4 | (fy & 7) << 8 | slot << 12 | (ridx < 0 ? 0 : ridx) << 16;
    L.mvi[lane][3] = ox | oy << 8 | pw << 16 | ph << 24;
    // last luma row this block can touch in the frame that may still be in flight: its 4 rows, 3 more under a
    // vertical 6-tap; chroma: 2 rows, 1 more under a vertical fraction (in luma units)
    if (L.refp[slot][0] == prev_dy) need = max (syy + 3 + ((fy & 3) ? 3 : 0), 2 * (cys + 1 + ((fy & 7) ? 1 : 0)) + 1);
  }
  if (__ballot (prev_dy != 0)) {                    // (wave-uniform)
#pragma unroll
    for (int msk = 1; msk < 16; msk <<= 1) need = max (need, __shfl_xor (need, msk));
    need = uni (need);
    if (need != -0x7fffffff) {
      const int hn = uni (FR.prev_h_nw), prev_h = hn & 0xffff;
      const int rneed = clip3 (need >> 4, 0, prev_h - 1);
      wait_prefix (G, L, uni (FR.prev_base) + min (rneed + 1, prev_h - 1), hn >> 16);
    }
  }
  wsync();
  const bool wp = sl.weighted() != 0;
  // ---- issue every reference fetch of the macroblock ------------------------------------------------------------
  const int lrb = by * 4 + bx;                      // raster index of this lane's luma block
  const int linfo = L.mvi[lrb][2];
  const int lfx = linfo & 3, lfy = (linfo >> 2) & 3;
  const bool any_fy = __ballot (lfy != 0) != 0;     // wave-uniform: does any strip need the vertical neighbours?
  v4u lrow[6];
  int lsh;
  {
    const GLB uint8_t* plane = (const GLB uint8_t*)L.refp[(linfo >> 12) & 15][0];
    const uintptr_t a0 = (uintptr_t) (plane + L.mvi[lrb][0] + r * F.sy - 2);
    lsh = (int) (a0 & 3);
    const GLB uint8_t* q = (const GLB uint8_t*) (a0 & ~ (uintptr_t)3);
#ifdef LH264_ABL_NOMC      // timing ablation only (wrong pictures): no reference fetch
#pragma unroll
    for (int k = 0; k < 6; k++) lrow[k] = (v4u) ((uint32_t) (uintptr_t)q);
#else
    lrow[2] = * (const GLB v4u*)q;
    if (any_fy) {
      lrow[0] = * (const GLB v4u*) (q - 2 * F.sy); lrow[1] = * (const GLB v4u*) (q - F.sy);
      lrow[3] = * (const GLB v4u*) (q + F.sy); lrow[4] = * (const GLB v4u*) (q + 2 * F.sy); lrow[5] = * (const GLB v4u*) (q + 3 * F.sy);
    }                                               // else they stay undefined and are never used: every strip has fy == 0, and 20
                                                    // moves of zeros in front of the branch would be paid by every macroblock
#endif
  }
  // chroma: lane l and lane l + 32 share the 4-sample strip of lane l < 32; half h = l >> 5 takes the pair at columns
  // cx0 + 2h, cx0 + 2h + 1 (one motion vector: a 4x4 luma block is a 2x2 chroma block)
  const int ch = lane >> 5, cx = cx0 + 2 * ch;
  const int crb = (cy >> 1) * 4 + (cx >> 1);
  const int cinfo = L.mvi[crb][2];
  v2u crow[2];                                      // [row]
  int csh;
  {
    const GLB uint8_t* plane = (const GLB uint8_t*)L.refp[(cinfo >> 12) & 15][1 + cp];
    const uintptr_t a0 = (uintptr_t) (plane + L.mvi[crb][1] + (cy & 1) * F.sc);
    csh = (int) (a0 & 3);
    const GLB uint8_t* q = (const GLB uint8_t*) (a0 & ~ (uintptr_t)3);
#ifdef LH264_ABL_NOMC
    crow[0] = crow[1] = (v2u) ((uint32_t) (uintptr_t)q);
#else
    crow[0] = * (const GLB v2u*)q;
    crow[1] = * (const GLB v2u*) (q + F.sc);
#endif
  }
  // ---- luma ------------------------------------------------------------------------------------------------------
  int pr[4], res[4];
  uint32_t lpk;
  {
    Row12 R[6];
#pragma unroll
    for (int k = 0; k < 6; k++) R[k] = align12 (lrow[k], lsh);
    lpk = mc_luma_rows (R, lfx, lfy, any_fy);
  }
  if (__ballot (wp || has_res)) {                   // (wave-uniform) otherwise the strip is final as it is
#pragma unroll
    for (int i = 0; i < 4; i++) pr[i] = BYTE (lpk, i);
    if (wp) {
      const int ri = (linfo >> 16) & 15, ld = sl.luma_denom(), wt = sl.luma_weight (ri), of = sl.luma_offset (ri);
#pragma unroll
      for (int i = 0; i < 4; i++) pr[i] = clip_u8 (ld >= 1 ? ((pr[i] * wt + (1 << (ld - 1))) >> ld) + of : pr[i] * wt + of);
    }
    res[0] = res[1] = res[2] = res[3] = 0;
    if (has_res) load_res4 (L.R, lane, res);
    lpk = pack_add4 (pr, res);
  }
  * (LDS uint32_t*)&L.T[tY (ly, lx0)] = lpk;
  // ---- chroma pair: plane cp, row cy, cols cx, cx+1 --------------------------------------------------------------
  {
    int cpr[2];
    const uint32_t a = __builtin_amdgcn_alignbyte (crow[0].y, crow[0].x, csh);
    const uint32_t bb = __builtin_amdgcn_alignbyte (crow[1].y, crow[1].x, csh);
    mc_chroma_rows (a, bb, (cinfo >> 4) & 7, (cinfo >> 8) & 7, cpr[0], cpr[1]);
    if (wp) {
      // reference quirk (rec_mb.cpp:309-311): only the top-left (w>>2)x(h>>2) samples of the chroma block are weighted
      const int geo = L.mvi[crb][3];
      const int pox = (geo & 0xff) >> 1, poy = ((geo >> 8) & 0xff) >> 1, pw = (geo >> 16) & 0xff, ph = (geo >> 24) & 0xff;
      const int ri = (cinfo >> 16) & 15, ld = sl.chroma_denom(), wt = sl.chroma_weight (ri, cp), of = sl.chroma_offset (ri, cp);
#pragma unroll
      for (int i = 0; i < 2; i++) {
        if (cx + i - pox < (pw >> 2) && cy - poy < (ph >> 2)) {
          const int v = cpr[i];
          cpr[i] = clip_u8 (ld >= 1 ? ((v * wt + (1 << (ld - 1))) >> ld) + of : v * wt + of);
        }
      }
    }
    // residual of the pair: int16 values 2h, 2h + 1 of the strip's 4 (load_res4 layout)
    const int cr = has_res ? * (const LDS int32_t*) (L.R + 256 + 4 * (lane & 31) + 2 * ch) : 0;
    * (LDS uint16_t*)&L.C[cp][tC (cy, cx)] = (uint16_t) (clip_u8 (cpr[0] + sext16 (cr)) | clip_u8 (cpr[1] + (cr >> 16)) << 8);
  }
}

// ------------------------------------------------------------------------------------------------
// deblocking (deblocking.cpp / deblocking_common.cpp)
// ------------------------------------------------------------------------------------------------
// Boundary strengths from the blocks, not from the edges: DeblockingBsMarginalMBAvcbase deblocking.cpp:273-352,
// DeblockingBSInsideMB* :160-271, WelsDeblockingMb :815-862.  The strength of segment `seg` of edge `e` in direction dir (0: vertical
// edges) is a function of two 4x4 blocks: q = (e, seg) for dir 0, (seg, e) for dir 1, and p, the block to its left / above it - inside
// the macroblock, or in the left / upper neighbour for e == 0.  A lane holds q's data once (BsBlk), gets p's from the lane 4 below it
// (one DPP row shift serves both directions) or from the neighbour's record, and decides in straight-line code (bs_decide).

// what a strength needs of the 4x4 block (bx, by) of a staged record.  Under the 8x8 transform a block stands for its 8x8 block: the
// counts of all four blocks, the vector of the first one (deblocking.cpp:273-352).  nr: bits 0..7 ref_idx, bits 8.. nonzero if a count is
struct BsBlk { uint32_t mv; int nr; };
// ANY8 false: no 8x8 transform on either side of any edge of this macroblock (known per wave) - byte reads, nothing to remap
template <bool ANY8> __device__ __forceinline__ BsBlk bs_block (RecView r, int bx, int by, bool t8) {
  const int ri = (by & 2) + (bx >> 1);
  BsBlk o;
  if (!ANY8) {
    const int b = by * 4 + bx;
    o.mv = * (const LDS uint32_t*) (r.p + 60 + 4 * b);
    o.nr = r.p[32 + ri] | r.p[36 + b] << 8;
    return o;
  }
  const LDS uint32_t* w = (const LDS uint32_t*)r.p;          // dword 8: ref_idx[4], 9..12: nzc rows, 15..30: mv[16]
  const uint32_t n0 = w[9 + (by & 2)], n1 = w[10 + (by & 2)];
  const uint32_t nw = t8 ? (n0 | n1) : (by & 1) ? n1 : n0;
  const uint32_t nz = (nw >> (t8 ? 16 * (bx >> 1) : 8 * bx)) & (t8 ? 0xffffu : 0xffu);
  o.mv = w[15 + (t8 ? (by & 2) * 4 + (bx & 2) : by * 4 + bx)];
  o.nr = (int) ((w[8] >> (8 * ri)) & 0xffu) | (nz ? 0x100 : 0);
  return o;
}
// edge0: a macroblock edge (p lies in the neighbour: have_nb, nb_intra); intra / skip / mv_too / t8: of the current macroblock.
// Reference INDICES are compared, not pictures (MB_BS_MV deblocking.cpp:58-63); inside P16x16 no vectors are compared, SKIP has no
// inner edges, edges 1 and 3 do not exist under the 8x8 transform (deblocking.cpp:836-849).
__device__ __forceinline__ int bs_decide (BsBlk q, BsBlk p, bool edge0, int e, bool have_nb, bool nb_intra, bool intra, bool skip, bool mv_too, bool t8) {
  const int dx = sext16 ((int)q.mv) - sext16 ((int)p.mv), dy = ((int)q.mv >> 16) - ((int)p.mv >> 16);
  const bool mv = (((q.nr ^ p.nr) & 0xff) != 0) || (uint32_t) (dx + 3) > 6u || (uint32_t) (dy + 3) > 6u;      // |d| >= 4
  const int core = ((q.nr | p.nr) & 0xff00) ? 2 : (mv && (edge0 || mv_too)) ? 1 : 0;
  const int inner = intra ? 3 : skip ? 0 : core;
  const int outer = !have_nb ? 0 : (intra || nb_intra) ? 4 : core;
  return (t8 && (e & 1)) ? 0 : edge0 ? outer : inner;
}
// the strength of lane < 32 = (dir, edge, segment), the layout of L.bs
template <bool ANY8> __device__ __forceinline__ int bs_lane (RecView m, RecView lm, RecView tm, bool left_av, bool top_av, int mtype, int ltype, int ttype,
                                                            bool mintra, bool t8, bool lt8, bool tt8, int lane) {
  const int dir = lane >> 4, e = (lane >> 2) & 3, seg = lane & 3;
  const BsBlk q = bs_block<ANY8> (m, dir ? seg : e, dir ? e : seg, t8);
  // the block before the edge: lanes 0..15 hold the blocks column by column, lanes 16..31 row by row, so it is 4 lanes down in both
  BsBlk p;
  p.mv = (uint32_t)__builtin_amdgcn_update_dpp (0, (int)q.mv, 0x114, 0xf, 0xf, true);      // row_shr:4
  p.nr = __builtin_amdgcn_update_dpp (0, q.nr, 0x114, 0xf, 0xf, true);
  const RecView nb = {dir ? tm.p : lm.p};
  const BsBlk n = bs_block<ANY8> (nb, dir ? seg : 3, dir ? 3 : seg, dir ? tt8 : lt8);
  const bool edge0 = e == 0;
  if (edge0) p = n;
  return bs_decide (q, p, edge0, e, dir ? top_av : left_av, ((dir ? ttype : ltype) & LH264_MB_INTRA) != 0, mintra, mtype == LH264_MB_SKIP,
                    mtype != LH264_MB_P16x16, t8);
}

// Filter one line across one edge, samples in registers.  Luma: DeblockLumaLt4_c / DeblockLumaEq4_c
// (deblocking_common.cpp:5-83); chroma: DeblockChromaLt4_c / DeblockChromaEq4_c (:85-140), which only touch p0/q0 and
// use tc0+1.  One routine for both so that the luma lanes (0..15) and the chroma lanes (16..31) of a wave run the same
// instruction stream.  Every formula uses the samples as they were before this edge.
// Written without divergent branches: the lanes of a wave hold different lines with different strengths, so a branch per condition
// is a chain of exec-mask saves and restores around a few instructions each; here the normal filter is computed for every lane and
// selected, the strong one (bS 4: macroblock edges of intra macroblocks only) behind one wave-uniform branch.
__device__ __forceinline__ int absd (int a, int b) { return (int)__builtin_amdgcn_sad_u16 ((uint32_t)a, (uint32_t)b, 0u); }    // samples: 0..255
__device__ __forceinline__ void filter_edge (int& rp3, int& rp2, int& rp1, int& rp0, int& rq0, int& rq1, int& rq2, int& rq3,
                                             int bs, int alpha, int beta, int tc0, bool chroma) {
  const int p3 = rp3, p2 = rp2, p1 = rp1, p0 = rp0, q0 = rq0, q1 = rq1, q2 = rq2, q3 = rq3;
  const int d = absd (p0, q0);
  const bool on = bs != 0 && d < alpha && absd (p1, p0) < beta && absd (q1, q0) < beta;
  const bool ap = !chroma && absd (p2, p0) < beta, aq = !chroma && absd (q2, q0) < beta;
  // bS < 4
  const int t = tc0 + (ap ? 1 : 0) + (aq ? 1 : 0) + (chroma ? 1 : 0);    // (ap, aq are false on chroma lines)
  const int dl = clip3 ((((q0 - p0) << 2) + (p1 - q1) + 4) >> 3, -t, t);
  const int avg = (p0 + q0 + 1) >> 1;
  const int np0 = clip_u8 (p0 + dl), nq0 = clip_u8 (q0 - dl);
  const int np1 = p1 + (ap ? clip3 ((p2 + avg - (p1 << 1)) >> 1, -tc0, tc0) : 0);
  const int nq1 = q1 + (aq ? clip3 ((q2 + avg - (q1 << 1)) >> 1, -tc0, tc0) : 0);
  // p2 / q2 change under bS 4 only: the normal filter selects four samples, the strong one overrides up to six
  rp0 = on ? np0 : p0; rq0 = on ? nq0 : q0; rp1 = on ? np1 : p1; rq1 = on ? nq1 : q1;
  const bool on4 = on && bs == 4;
  if (__ballot (on4)) {                             // wave-uniform
    const bool small = !chroma && d < ((alpha >> 2) + 2);
    const bool sp = small && ap, sq = small && aq;
    const int wp0 = (2 * p1 + p0 + q1 + 2) >> 2, wq0 = (2 * q1 + q0 + p1 + 2) >> 2;
    const int xp0 = sp ? (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3 : wp0;
    const int xq0 = sq ? (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3 : wq0;
    const int xp1 = sp ? (p2 + p1 + p0 + q0 + 2) >> 2 : p1, xq1 = sq ? (p0 + q0 + q1 + q2 + 2) >> 2 : q1;
    const int xp2 = sp ? (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3 : p2, xq2 = sq ? (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3 : q2;
    rp0 = on4 ? xp0 : rp0; rq0 = on4 ? xq0 : rq0; rp1 = on4 ? xp1 : rp1; rq1 = on4 ? xq1 : rq1; rp2 = on4 ? xp2 : p2; rq2 = on4 ? xq2 : q2;
  }
}

// WelsDeblockingMb (deblocking.cpp:815-862) + FilteringEdgeLumaHV / FilteringEdgeChromaHV (:568-700): the macroblock's
// vertical edges then its horizontal edges, inside the tile.  Lane i < 16 owns luma line i (a row for the vertical
// edges, a column for the horizontal ones), lanes 16..31 own the 8 lines of Cb and Cr.  A line is loaded once, all its
// edges are filtered in registers, and it is written back once.
__device__ LH264_PHASE void deblock_phase (LDS WaveLds& L, const LDS WgLds& G, RecView m, RecView lm, RecView tm, SliceView sl,
                                            bool left_av, bool top_av, int lane) {
  const int mtype = uni (m.mb_type());
  const bool mintra = (mtype == LH264_MB_I4x4 || mtype == LH264_MB_I8x8 || mtype == LH264_MB_I16x16 || mtype == LH264_MB_IPCM);
  int my_bs = 0;
  if (lane < 32) {
    const bool t8 = (uni (m.flags()) & LH264_MBF_T8x8) != 0;
    const int ltype = uni (lm.mb_type()), ttype = uni (tm.mb_type());
    const bool lt8 = (uni (lm.flags()) & LH264_MBF_T8x8) != 0, tt8 = (uni (tm.flags()) & LH264_MBF_T8x8) != 0;
    if (t8 || lt8 || tt8) my_bs = bs_lane<true> (m, lm, tm, left_av, top_av, mtype, ltype, ttype, mintra, t8, lt8, tt8, lane);
    else my_bs = bs_lane<false> (m, lm, tm, left_av, top_av, mtype, ltype, ttype, mintra, false, false, false, lane);
    L.bs[lane] = (uint8_t)my_bs;
  }
  // which of the 2 x 4 edges have any strength at all: one scalar mask (bit 16 dir + 4 edge + segment), so that an edge nobody
  // filters costs a scalar branch and nothing else
  const uint32_t live = (uint32_t)__ballot (my_bs != 0);
  wsync();
  const v4u bs0 = * (const LDS v4u*)&L.bs[0], bs1 = * (const LDS v4u*)&L.bs[16];     // [edge] = 4 segment bytes
  const bool any0 = (live & 0xffffu) != 0, any1 = (live >> 16) != 0;
  if ((!any0 && !any1) || lane >= 32) return;
#ifdef LH264_ABL_BSONLY      // timing ablation only (wrong pictures): boundary strengths, no filtering
  return;
#endif
  const bool chroma = lane >= 16;
  const int cpl = (lane >> 3) & 1;                  // chroma plane of lanes 16..31
  const int li = chroma ? (lane & 7) : lane;        // line inside the plane
  const int sh8 = 8 * (chroma ? (li >> 1) : (li >> 2));   // this line's segment byte inside a bS dword
  // alpha / beta / tc0 for the three QP cases: inner edges, left macroblock edge, top macroblock edge
  const LDS uint8_t* tab = G.tab;
  const int ao = sl.alpha_off(), bo = sl.beta_off();
  const int qc = chroma ? m.qp_c (cpl) : m.qp_y();
  const int ql = (qc + (chroma ? lm.qp_c (cpl) : lm.qp_y()) + 1) >> 1;
  const int qt = (qc + (chroma ? tm.qp_c (cpl) : tm.qp_y()) + 1) >> 1;
  const int iac = tab_idx (qc + ao);
  const int alc = tab[TAB_ALPHA + iac], bec = tab[TAB_BETA + tab_idx (qc + bo)];
  const uint32_t tcc = * (const LDS uint32_t*)&tab[TAB_TC0 + 4 * iac];
  // The two macroblock edges take the mean of two QPs.  Where every line of the macroblock (all 32 lanes here: luma and both chroma
  // planes) finds both means equal to its own QP - a stream of one QP, the usual case - the inner edges' lookup serves all three.
  int all_ = alc, alt = alc, bel = bec, bet = bec;
  uint32_t tcl = tcc, tct = tcc;
#ifdef LH264_ABL_QP3         // timing ablation only (same pictures): three lookups always
  if (true) {
#else
  if (__ballot (ql != qc || qt != qc)) {            // (wave-uniform)
#endif
    const int ial = tab_idx (ql + ao), iat = tab_idx (qt + ao);
    all_ = tab[TAB_ALPHA + ial]; alt = tab[TAB_ALPHA + iat];
    bel = tab[TAB_BETA + tab_idx (ql + bo)]; bet = tab[TAB_BETA + tab_idx (qt + bo)];
    tcl = * (const LDS uint32_t*)&tab[TAB_TC0 + 4 * ial]; tct = * (const LDS uint32_t*)&tab[TAB_TC0 + 4 * iat];
  }
  // Reference behaviour kept bit for bit: for an INTRA macroblock whose Cb and Cr QPs differ, FilteringEdgeChromaHV looks tc0 up
  // in its "chroma v" loop only; its "chroma h" loop (deblocking.cpp:786-807) filters the inner edge of each plane with what that
  // loop left behind - Cr's tc0 whenever Cr's alpha | beta is nonzero.  So Cb's inner horizontal edge takes Cr's tc0 then.
  uint32_t tcc_h = tcc;
  if (mintra && uni (m.qp_c (0)) != uni (m.qp_c (1))) {
    const int qr = m.qp_c (1), iar = tab_idx (qr + ao);
    if (chroma && cpl == 0 && (tab[TAB_ALPHA + iar] | tab[TAB_BETA + tab_idx (qr + bo)])) tcc_h = * (const LDS uint32_t*)&tab[TAB_TC0 + 4 * iar];
  }
  int v[20];
  if (any0 && (live & 0xfff0u) == 0) {
    // ---- vertical edges, only the macroblock edge is live: samples -4..3 of the row ------------------------------------------------
    LDS uint32_t* rowp = (LDS uint32_t*) (chroma ? &L.C[cpl][tC (li, -4)] : &L.T[tY (li, -4)]);
    const uint32_t w0 = rowp[0], w1 = rowp[1];
    int p3 = BYTE (w0, 0), p2 = BYTE (w0, 1), p1 = BYTE (w0, 2), p0 = BYTE (w0, 3), q0 = BYTE (w1, 0), q1 = BYTE (w1, 1), q2 = BYTE (w1, 2), q3 = BYTE (w1, 3);
    const int bs = (int) ((bs0.x >> sh8) & 0xff);
    filter_edge (p3, p2, p1, p0, q0, q1, q2, q3, (all_ | bel) ? bs : 0, all_, bel, (int) ((tcl >> (8 * (bs & 3))) & 0xff), chroma);
    rowp[0] = (uint32_t)p3 | (uint32_t)p2 << 8 | (uint32_t)p1 << 16 | (uint32_t)p0 << 24;
    rowp[1] = (uint32_t)q0 | (uint32_t)q1 << 8 | (uint32_t)q2 << 16 | (uint32_t)q3 << 24;
  } else if (any0) {
    // ---- vertical edges: line = row li, samples -4..15 (chroma -4..7) ------------------------------------------
    LDS uint32_t* rowp = (LDS uint32_t*) (chroma ? &L.C[cpl][tC (li, -4)] : &L.T[tY (li, -4)]);
    uint32_t w[5];
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = rowp[k];
    w[4] = chroma ? 0u : rowp[4];
#pragma unroll
    for (int i = 0; i < 20; i++) v[i] = BYTE (w[i >> 2], i & 3);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      // (scalar; the chroma lines take the strengths of luma edge 2 for their edge 1)
      if ((((k == 1 ? live | live >> 4 : live) >> (4 * k)) & 15u) == 0) continue;
      // chroma edge k (k < 2) lies on luma edge 2k; chroma has no edges 2, 3
      const uint32_t bl = k == 0 ? bs0.x : k == 1 ? bs0.y : k == 2 ? bs0.z : bs0.w;
      const uint32_t bc = k == 0 ? bs0.x : k == 1 ? bs0.z : 0u;
      const int bs = (int) (((chroma ? bc : bl) >> sh8) & 0xff);
      const int alpha = k == 0 ? all_ : alc, beta = k == 0 ? bel : bec;
      const uint32_t tcw = k == 0 ? tcl : tcc;
      filter_edge (v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3], v[4 * k + 4], v[4 * k + 5], v[4 * k + 6], v[4 * k + 7],
                   (alpha | beta) ? bs : 0, alpha, beta, (int) ((tcw >> (8 * (bs & 3))) & 0xff), chroma);
    }
#pragma unroll
    for (int k = 0; k < 5; k++) w[k] = (uint32_t)v[4 * k] | (uint32_t)v[4 * k + 1] << 8 | (uint32_t)v[4 * k + 2] << 16 | (uint32_t)v[4 * k + 3] << 24;
#pragma unroll
    for (int k = 0; k < 3; k++) rowp[k] = w[k];
    if (!chroma) { rowp[3] = w[3]; rowp[4] = w[4]; }
  }
  wsync();
  if (any1 && (live & 0xfff00000u) == 0) {
    // ---- horizontal edges, only the macroblock edge is live: rows -4..3 of the column (chroma: -2..1) --------------------------------
    int p3 = 0, p2 = 0, p1, p0, q0, q1, q2 = 0, q3 = 0;
    const int bs = (int) ((bs1.x >> sh8) & 0xff);
    const int tc0 = (int) ((tct >> (8 * (bs & 3))) & 0xff);
    if (chroma) {
      LDS uint8_t* cp = &L.C[cpl][tC (-2, li)];
      p1 = cp[0]; p0 = cp[16]; q0 = cp[32]; q1 = cp[48];
      filter_edge (p3, p2, p1, p0, q0, q1, q2, q3, (alt | bet) ? bs : 0, alt, bet, tc0, true);
      cp[16] = (uint8_t)p0; cp[32] = (uint8_t)q0;
    } else {
      LDS uint8_t* cp = &L.T[tY (-4, li)];
      p3 = cp[0]; p2 = cp[32]; p1 = cp[64]; p0 = cp[96]; q0 = cp[128]; q1 = cp[160]; q2 = cp[192]; q3 = cp[224];
      filter_edge (p3, p2, p1, p0, q0, q1, q2, q3, (alt | bet) ? bs : 0, alt, bet, tc0, false);
      cp[32] = (uint8_t)p2; cp[64] = (uint8_t)p1; cp[96] = (uint8_t)p0; cp[128] = (uint8_t)q0; cp[160] = (uint8_t)q1; cp[192] = (uint8_t)q2;
    }
  } else if (any1) {
    // ---- horizontal edges: line = column li, luma rows -4..15 = v[0..19], chroma rows -2..7 = v[2..11] -----------
    LDS uint8_t* colp = chroma ? &L.C[cpl][tC (-2, li)] : &L.T[tY (-4, li)];
#pragma unroll
    for (int i = 0; i < 20; i++) {
      const int oc = (i < 2 ? 0 : i > 11 ? 9 : i - 2) * 16;
      v[i] = colp[chroma ? oc : i * 32];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if ((((k == 1 ? live | live >> 4 : live) >> (16 + 4 * k)) & 15u) == 0) continue;      // (scalar)
      const uint32_t bl = k == 0 ? bs1.x : k == 1 ? bs1.y : k == 2 ? bs1.z : bs1.w;
      const uint32_t bc = k == 0 ? bs1.x : k == 1 ? bs1.z : 0u;
      const int bs = (int) (((chroma ? bc : bl) >> sh8) & 0xff);
      const int alpha = k == 0 ? alt : alc, beta = k == 0 ? bet : bec;
      const uint32_t tcw = k == 0 ? tct : tcc_h;
      filter_edge (v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3], v[4 * k + 4], v[4 * k + 5], v[4 * k + 6], v[4 * k + 7],
                   (alpha | beta) ? bs : 0, alpha, beta, (int) ((tcw >> (8 * (bs & 3))) & 0xff), chroma);
    }
#pragma unroll
    for (int i = 1; i < 19; i++) {
      if (i >= 2 && i <= 11) colp[chroma ? (i - 2) * 16 : i * 32] = (uint8_t)v[i];
      else if (!chroma) colp[i * 32] = (uint8_t)v[i];
    }
  }
  wsync();
}

// ------------------------------------------------------------------------------------------------
// one macroblock: reconstruct (WelsTargetMbConstruction) + deblock (WelsDeblockingMb) + write back
// ------------------------------------------------------------------------------------------------
struct RowBufs {
  LDS uint8_t* lineCur; const LDS uint8_t* lineTop;     // unfiltered bottom rows
  LDS uint8_t* fCur; const LDS uint8_t* fTop;           // filtered bottom 4 / 2 rows
  int LY, LC, FW;                               // layout of a slot
};

// Wait until the wave of the row above has finished `need` (encoded as in WgLds::progress); nothing to wait for in the first row.
__device__ __forceinline__ void wait_row_above (volatile LDS int* prog_above, int need, bool have_row_above) {
  if (have_row_above) {
    while ((int) (*prog_above - need) < 0) __builtin_amdgcn_s_sleep (1);
    wsync();
  }
}

__device__ __forceinline__ void process_mb (const FrameCtx& F, LDS WaveLds& L, const LDS WgLds& G, const LDS FrameLds& FR, const RowBufs& B, const Pref& pf,
                                            int mbx, int mby, int par, int& slc_id, bool pub_line, bool pub_left, int lane,
                                            volatile LDS int* prog_above, int need_above
#ifdef LH264_STAMP
                                            , unsigned long long& st_t0, unsigned long long* st_acc
#endif
                                           ) {
  LDS uint8_t* T = L.T;
  LDS uint8_t* const tile = L.T;             // luma tile and, behind it (TILE_C), the two chroma tiles as one array
  // The row above must be two macroblocks ahead (top-right neighbour of intra prediction; raster order of the in-loop filter).  Only
  // an INTRA macroblock needs that before it starts: inter prediction and the residual read nothing of the row above, so every other
  // macroblock predicts first and waits where its filter takes the neighbours' filtered samples - the wait overlaps its own work.
  const bool early_wait = (uni ((int)pf.rec) & LH264_MB_INTRA) != 0;         // lane 0 holds the record's first dword: mb_type in the low half
  if (early_wait) wait_row_above (prog_above, need_above, mby > 0);
  // ---- 0. stage the prefetched records ----------------------------------------------------------
  if (lane < 32) L.rec[par][lane] = pf.rec; else L.trec[lane - 32] = pf.rec;
  wsync();
  const RecView m = { (const LDS uint8_t*)L.rec[par]}, lm = { (const LDS uint8_t*)L.rec[par ^ 1]}, tm = { (const LDS uint8_t*)L.trec};
  const int mb_type = uni (m.mb_type());
  const int cbp = uni (m.cbp());
  const int mflags = uni (m.flags());
  const int sid = uni (m.slice_id());
  if (sid != slc_id) {              // refresh the cached slice record
    if (lane < 58) L.slc[lane] = ((const GLB uint32_t*) (F.slices + sid))[lane];
    slc_id = sid;
    wsync();
  }
  const SliceView sl = { (const LDS uint8_t*)L.slc};
  const bool t8 = mflags & LH264_MBF_T8x8;
  const bool covered = mb_type != 0;
  const bool intra = (mb_type & LH264_MB_INTRA) != 0;

  const int b = lane >> 2, r = lane & 3;
  const int bx = (b & 1) | ((b >> 2) & 1) << 1, by = ((b >> 1) & 1) | ((b >> 3) & 1) << 1;
  const int ly = 4 * by + r, lx0 = 4 * bx;
  const int cp = (lane >> 4) & 1, cj = (lane >> 2) & 3;
  const int cy = 4 * (cj >> 1) + r, cx0 = 4 * (cj & 1);

  STAMP (0);
  // ---- 1. unfiltered neighbours -> tile (only intra prediction reads them) -------------------------
  if (intra && mby > 0) {
    if (lane < 8) * (LDS uint32_t*)&T[tY (-1, -4 + 4 * lane)] = * (const LDS uint32_t*)&B.lineTop[16 + 16 * mbx - 4 + 4 * lane];
    else if (lane < 16) {
      const int p = (lane - 8) >> 2, q = (lane - 8) & 3;
      * (LDS uint32_t*)&tile[TILE_C (p) + tC (-1, -4 + 4 * q)] = * (const LDS uint32_t*)&B.lineTop[B.LY + (p ? B.LC : 0) + 8 + 8 * mbx - 4 + 4 * q];
    }
  }
  if (intra && mbx > 0) {
    if (lane >= 16 && lane < 32) T[tY (lane - 16, -1)] = L.leftY[lane - 16];
    else if (lane >= 32 && lane < 48) { const int p = (lane - 32) >> 3, q = (lane - 32) & 7; tile[TILE_C (p) + tC (q, -1)] = L.leftC[0][lane - 32]; }
  }
  wsync();

  STAMP (1);
  if (covered) {
    // ---- 2. residual -> R ------------------------------------------------------------------------
    const bool i16 = mb_type == LH264_MB_I16x16;
    const bool has_res = cbp != 0 || i16;
    if (mb_type != LH264_MB_IPCM) {
      if (has_res) {
        const int dcw = sl.luma_dc_weight();
#ifndef LH264_ABL_NORES      // timing ablation only (wrong pictures)
        residual_phase (L, pf.l, pf.c, mb_type, cbp, t8, m.qp_y(), dcw ? dcw : 16, lane);
#endif
      } else if (intra) zero_residual (L, lane);
    }
    STAMP (2);
    // ---- 3. prediction + residual -> tile -----------------------------------------------------
    if (mb_type == LH264_MB_IPCM) {
      // samples travel in the coefficient slot, row-major (decode_slice.cpp:3213-3263 copies them at parse time)
      const v2i v = pf.l;
      const int yy = lane >> 2, xx = 4 * (lane & 3);
      * (LDS uint32_t*)&T[tY (yy, xx)] = (v.x & 0xff) | ((v.x >> 16) & 0xff) << 8 | (v.y & 0xff) << 16 | ((v.y >> 16) & 0xff) << 24;
      if (lane < 32) {
        const v2i cv = pf.c;
        const int p = lane >> 4, yy2 = (lane >> 1) & 7, xx2 = 4 * (lane & 1);
        * (LDS uint32_t*)&tile[TILE_C (p) + tC (yy2, xx2)] = (cv.x & 0xff) | ((cv.x >> 16) & 0xff) << 8 | (cv.y & 0xff) << 16 | ((cv.y >> 16) & 0xff) << 24;
      }
    } else if (intra) {
      if (i16) intra16_phase (L, uni (m.intra_mode (0)), lane);
      else if (mb_type == LH264_MB_I8x8) intra8x8_phase (L, m, lane);
      else intra4x4_phase (L, m, lane);
      intra_chroma_phase (L, uni (m.chroma_mode()), lane);
    } else if (mb_type & LH264_MB_INTER) {
#ifndef LH264_ABL_NOINTER    // timing ablation only (wrong pictures)
      inter_phase (L, G, FR, m, sl, mb_type, mbx, mby, has_res, lane);
#endif
    }
  } else {
    // macroblock not covered by any slice (lost data): pass the picture's current samples through
    * (LDS uint32_t*)&T[tY (ly, lx0)] = * (const GLB uint32_t*) (F.dy + ((size_t) (mby * 16) * F.sy + mbx * 16) + mad24 (ly, F.sy, lx0));
    if (lane < 32) * (LDS uint32_t*)&tile[TILE_C (cp) + tC (cy, cx0)] = * (const GLB uint32_t*) ((cp ? F.dv : F.du) + ((size_t) (mby * 8) * F.sc + mbx * 8) + mad24 (cy, F.sc, cx0));
  }
  wsync();

  STAMP (3);
  // ---- 4. publish unfiltered bottom row / right column, when an intra macroblock will read them -----
  if (pub_line) {
    if (lane < 4) * (LDS uint32_t*)&B.lineCur[16 + 16 * mbx + 4 * lane] = * (const LDS uint32_t*)&T[tY (15, 4 * lane)];
    else if (lane < 8) { const int p = (lane - 4) >> 1, q = (lane - 4) & 1; * (LDS uint32_t*)&B.lineCur[B.LY + (p ? B.LC : 0) + 8 + 8 * mbx + 4 * q] = * (const LDS uint32_t*)&tile[TILE_C (p) + tC (7, 4 * q)]; }
  }
  if (pub_left) {
    if (lane >= 16 && lane < 32) L.leftY[lane - 16] = T[tY (lane - 16, 15)];
    else if (lane >= 32 && lane < 48) { const int p = (lane - 32) >> 3, q = (lane - 32) & 7; L.leftC[0][lane - 32] = tile[TILE_C (p) + tC (q, 7)]; }
  }
  if (pub_line || pub_left) wsync();

  STAMP (4);
  // ---- 5. in-loop filter inside the tile ---------------------------------------------------------
  const int stype = sl.slice_type();
  const int idc = sl.deblock_idc();
  const bool filt = covered && !(F.flags & LH264_JOB_NO_DEBLOCK) && idc != 1 && (stype == 0 || stype == 2);
  bool left_av = mbx > 0, top_av = mby > 0;
  if (filt) {                       // an edge towards a concealed macroblock is not filtered: it takes no part in the filter
    if (lm.mb_type() & LH264_MB_CONCEAL) left_av = false;
    if (tm.mb_type() & LH264_MB_CONCEAL) top_av = false;
  }
  if (filt && idc == 2) {           // DeblockingAvailableNoInterlayer deblocking.cpp:354-369
    if (left_av) left_av = lm.slice_id() == sid;
    if (top_av) top_av = tm.slice_id() == sid;
  }
  if (!early_wait) wait_row_above (prog_above, need_above, mby > 0);
  // neighbours' filtered samples: left 4 columns carried from the previous step, top rows from `fline`.
  // The carry (lfY, lfC) and the tiles (T, C) are one array each: lane l < 40 moves dword l of the carry, whose place in the tiles is
  // row l of the luma tile (32 bytes a row) or row l - 20 of the chroma tiles (16 bytes a row, 10 rows each).
  const int carry_off = lane < 20 ? 32 * lane : 16 * lane + 320;      // tile offset of columns -4..-1 of the lane's row
  if (mbx > 0 && lane < 40) * (LDS uint32_t*)&tile[carry_off] = L.lfY[lane];
  if (mby > 0 && lane >= 40) {
    // lanes 40..55: luma rows -4..-1 x 4 dwords; lanes 56..63: chroma plane p rows -2, -1 x 2 dwords.  `fline` holds 4 luma rows of
    // FW bytes, then 4 chroma rows (plane, row) of FW / 2 bytes: row a of FW / 2 bytes each
    const bool ch = lane >= 56;
    const int j = ch ? (lane - 56) >> 1 : (lane - 40) >> 2;           // luma row, or chroma (plane * 2 + row)
    const int q = ch ? lane & 1 : lane & 3;
    const int dst = ch ? TILE_C (j >> 1) + tC (-2 + (j & 1), 4 * q) : tY (-4 + j, 4 * q);
    const int src = (int)mad24 (ch ? 8 + j : 2 * j, B.FW >> 1, 4 * q) + (ch ? mbx * 8 : mbx * 16);
    * (LDS uint32_t*)&tile[dst] = * (const LDS uint32_t*)&B.fTop[src];
  }
  wsync();
  STAMP (5);
  if (filt) deblock_phase (L, G, m, lm, tm, sl, left_av, top_av, lane);
  STAMP (6);
  // carry the (filtered) right 4 columns to the next macroblock of this row
  if (lane < 40) L.lfY[lane] = * (const LDS uint32_t*)&tile[carry_off + (lane < 20 ? 16 : 8)];

  // ---- 6. write the samples that became final: 16x16 window at (-4,-3), chroma 8x8 at (-4,-1) --------
  // Every store goes to a wave-uniform 64-bit base (the window's first sample) plus the lane's unsigned 32-bit offset row * stride + col.
  const bool last_x = mbx == F.mb_w - 1, last_y = mby == F.mb_h - 1;
  const bool has_l = mbx > 0, has_t = mby > 0;
#ifndef LH264_ABL_NOSTORE    // timing ablation only (no pictures)
  GLB uint8_t* const wy = F.dy + ((ptrdiff_t) (mby * 16 - 3) * F.sy + (mbx * 16 - 4));
  const ptrdiff_t wc_off = (ptrdiff_t) (mby * 8 - 1) * F.sc + (mbx * 8 - 4);
  GLB uint8_t* const wu = F.du + wc_off;
  GLB uint8_t* const wv = F.dv + wc_off;
  {
    const int wr = lane >> 2, wc = lane & 3;             // window row 0..15 (picture row -3 + wr), dword 0..3
    if ((wr >= 3 || has_t) && (wc || has_l))
      * (GLB uint32_t*) (wy + mad24 (wr, F.sy, 4 * wc)) = * (const LDS uint32_t*)&tile[32 * (wr + 1) + 4 * wc];
    {                                                    // lanes 0..15 U, 16..31 V: one store each from its own uniform base
      const int p = (lane >> 4) & 1, cr = (lane >> 1) & 7, cc = lane & 1;    // window row 0..7 (picture row -1 + cr), dword 0..1
      const bool on = lane < 32 && (cr || has_t) && (cc || has_l);
      const uint32_t v = * (const LDS uint32_t*)&tile[TILE_C (p) + 16 * (cr + 1) + 4 * cc];
      const uint32_t o = mad24 (cr, F.sc, 4 * cc);
      if (on && !p) * (GLB uint32_t*) (wu + o) = v;
      if (on && p) * (GLB uint32_t*) (wv + o) = v;
    }
  }
  if (last_x) {                     // right-most columns never get a successor: lanes 0..15 luma, 16..23 U, 24..31 V
    const int p = (lane >> 3) & 1, cr = lane & 7;
    const bool luma = lane < 16;
    const uint32_t v = * (const LDS uint32_t*)&tile[luma ? 32 * (lane + 1) + 16 : TILE_C (p) + 16 * (cr + 1) + 8];
    const uint32_t o = luma ? mad24 (lane, F.sy, 16) : mad24 (cr, F.sc, 8);
    const bool con = lane < 32 && !luma && (cr || has_t);
    if (luma && (lane >= 3 || has_t)) * (GLB uint32_t*) (wy + o) = v;
    if (con && !p) * (GLB uint32_t*) (wu + o) = v;
    if (con && p) * (GLB uint32_t*) (wv + o) = v;
  }
  // the bottom rows, to the picture (last_y) or to `fline`: 8 lanes a row, of which dwords 0..4 (chroma 4 lanes, 0..2) exist: columns
  // -4..15 (-4..7), the first one only behind a left neighbour, the last one only at the last macroblock of the row
  const int bq = lane & 7, bcq = lane & 3;
  const bool bl_on = bq < 5 && (bq || has_l) && (bq < 4 || last_x);
  const bool bc_on = bcq < 3 && (bcq || has_l) && (bcq < 2 || last_x);
  if (last_y) {                     // bottom rows never get a successor
    if (lane < 24) {                // luma rows 13..15 = window rows 16..18
      const int wr = 16 + (lane >> 3);
      if (bl_on) * (GLB uint32_t*) (wy + mad24 (wr, F.sy, 4 * bq)) = * (const LDS uint32_t*)&tile[32 * (wr + 1) + 4 * bq];
    } else if (lane >= 32 && lane < 40) {   // chroma row 7 = window row 8 of either plane
      const int p = (lane >> 2) & 1;
      const uint32_t v = * (const LDS uint32_t*)&tile[TILE_C (p) + 16 * 9 + 4 * bcq];
      const uint32_t o = 8u * F.sc + 4u * bcq;
      if (bc_on && !p) * (GLB uint32_t*) (wu + o) = v;
      if (bc_on && p) * (GLB uint32_t*) (wv + o) = v;
    }
  }
#endif
  STAMP (7);
  // filtered bottom rows for the row below: tile rows 12..15 x cols [-4,11] (+ [12,15] at the last MB)
  if (!last_y) {
    if (lane < 32) {
      const int rr = lane >> 3;
      if (bl_on) * (LDS uint32_t*)&B.fCur[(int)mad24 (rr, B.FW, 4 * bq) + mbx * 16 - 4] = * (const LDS uint32_t*)&tile[32 * (16 + rr) + 4 * bq];
    } else if (lane < 48) {
      const int j = (lane - 32) >> 2;                    // plane * 2 + row
      if (bc_on) * (LDS uint32_t*)&B.fCur[(int)mad24 (8 + j, B.FW >> 1, 4 * bcq) + mbx * 8 - 4] = * (const LDS uint32_t*)&tile[TILE_C (j >> 1) + 16 * (8 + (j & 1)) + 4 * bcq];
    }
  }
  wsync();
}

// ------------------------------------------------------------------------------------------------
// ExpandReferencingPicture (expand_pic.cpp:145-174): every padding sample = nearest picture sample.
// Done band by band by single waves as the rows of a picture become final.
// ------------------------------------------------------------------------------------------------
// left and right padding of picture rows [r0, r1): every lane replicates one edge sample into 16 (PADW == 32: luma)
// or 16 (PADW == 16: chroma, the whole side) bytes
template <int PADW>
__device__ __forceinline__ void expand_rows (GLB uint8_t* p, int stride, int w, int r0, int r1, int lane) {
  constexpr int UPS = PADW / 16;                       // 16-byte units per side
  const int n = (r1 - r0) * 2 * UPS;
  for (int i = lane; i < n; i += 64) {
    const int rr = r0 + i / (2 * UPS), j = i % (2 * UPS);
    const bool right = j >= UPS;
    GLB uint8_t* row = p + (ptrdiff_t)rr * stride;
    const uint32_t v = 0x01010101u * row[right ? w - 1 : 0];
    GLB uint8_t* d = right ? row + w + 16 * (j - UPS) : row - PADW + 16 * j;
    * (GLB v4u*)d = (v4u) (v);
  }
}
// the band of PADW rows above (bottom == false) or below the picture, full padded width.  Each lane owns a column
// group of sizeof (U) bytes of the source row (replicated edge samples in the corners) and stores it to the band rows.
template <int PADW, typename U>
__device__ __forceinline__ void expand_band (GLB uint8_t* p, int stride, int w, int h, bool bottom, int lane) {
  constexpr int UB = (int)sizeof (U);
  const int nu = (w + 2 * PADW) / UB;                  // units per padded row
  const GLB uint8_t* src = p + (ptrdiff_t) (bottom ? h - 1 : 0) * stride;
  GLB uint8_t* dst0 = p + (ptrdiff_t) (bottom ? h : -PADW) * stride - PADW;
  const int rpi = nu >= 64 ? 1 : 64 / nu;              // band rows covered by one wave-wide store
  for (int c0 = 0; c0 < nu; c0 += 64) {
    const int cu = c0 + (rpi > 1 ? lane % nu : lane);   // this lane's unit
    const int rsub = rpi > 1 ? lane / nu : 0;
    const bool act = rpi > 1 ? lane < rpi * nu : cu < nu;
    U v = (U) (0u);
    if (act) {
      const int col = cu * UB - PADW;                  // first picture column of the unit
      if (col < 0) v = (U) (0x01010101u * src[0]);
      else if (col >= w) v = (U) (0x01010101u * src[w - 1]);
      else v = * (const GLB U*) (src + col);
    }
    for (int rr = rsub; rr < PADW; rr += rpi)
      if (act) * (GLB U*) (dst0 + (ptrdiff_t)rr * stride + cu * UB) = v;
  }
}
struct PadCtx { GLB uint8_t* dy; GLB uint8_t* du; GLB uint8_t* dv; int sy, sc, mb_w, mb_h; };
// padding that depends on macroblock row r only (its samples must be final and visible)
__device__ __noinline__ void pad_mb_row (const PadCtx F, int r, int lane) {
  const int W = F.mb_w * 16, H = F.mb_h * 16;
  expand_rows<LH264_PAD_LUMA> (F.dy, F.sy, W, 16 * r, 16 * r + 16, lane);
  expand_rows<LH264_PAD_CHROMA> (F.du, F.sc, W >> 1, 8 * r, 8 * r + 8, lane);
  expand_rows<LH264_PAD_CHROMA> (F.dv, F.sc, W >> 1, 8 * r, 8 * r + 8, lane);
  if (r == 0) {
    expand_band<LH264_PAD_LUMA, v4u> (F.dy, F.sy, W, H, false, lane);
    expand_band<LH264_PAD_CHROMA, v2u> (F.du, F.sc, W >> 1, H >> 1, false, lane);
    expand_band<LH264_PAD_CHROMA, v2u> (F.dv, F.sc, W >> 1, H >> 1, false, lane);
  }
  if (r == F.mb_h - 1) {
    expand_band<LH264_PAD_LUMA, v4u> (F.dy, F.sy, W, H, true, lane);
    expand_band<LH264_PAD_CHROMA, v2u> (F.du, F.sc, W >> 1, H >> 1, true, lane);
    expand_band<LH264_PAD_CHROMA, v2u> (F.dv, F.sc, W >> 1, H >> 1, true, lane);
  }
}

__global__ void __launch_bounds__ (512, LH264_MIN_WAVES)
recon_chain_kernel (const lh264_frame_job_t* __restrict__ jobs, const int32_t* __restrict__ chain_first, int n_chains,
                    int slot_bytes) {
  extern __shared__ __attribute__ ((aligned (16))) uint8_t smem_generic[];
  LDS uint8_t* smem = (LDS uint8_t*) (uintptr_t) (uint32_t) (uintptr_t)smem_generic;
  const int NW = blockDim.x >> 6;
  const int tid = threadIdx.x;
  const int wave = uni (tid >> 6);
  const int lane = tid & 63;
  LDS WgLds& G = * (LDS WgLds*)smem;
  LDS WaveLds* wl = (LDS WaveLds*) (smem + ((sizeof (WgLds) + 15) & ~15));
  LDS uint8_t* slots = (LDS uint8_t*) (wl + NW);                           // [NW + 1][slot_bytes]
  LDS WaveLds& L = wl[wave];
  const int NL = NW + 1;
  volatile LDS int* progress = G.progress;
  volatile LDS int* stored = G.stored;

  for (int i = tid; i < (int)sizeof (G.tab); i += blockDim.x) G.tab[i] = kTables[i];
  if (tid < 8) { progress[tid] = 0; stored[tid] = -1; }
  if (lane == 0) L.known_prefix = -1;
  __syncthreads();

  const int chain = blockIdx.x;
  if (chain >= n_chains) return;
  const int first = chain_first[chain], last = chain_first[chain + 1];

  // this wave's cursor over the chain's rows: global row g = base + row of job ji; the wave owns g == wave (mod NW)
  int ji = first, row = wave, base = 0, cur_ji = -1;
  int jw = 0;                               // rows this wave has started so far
  bool overlap_ok = false;
  int slc_id = -1;
  FrameCtx F;
  F.prev_base = 0;
  RowBufs B;
  int lu = 0;
  STAMP_DECL
  for (;;) {
    while (ji < last) {
      const int h = jobs[ji].mb_h;
      if (row < h) break;
      row -= h; base += h; ji++;
    }
    if (ji >= last) break;
    if (ji != cur_ji) {                      // entering a new frame
      const lh264_frame_job_t* J = jobs + ji;
      F.mbs = glb<const lh264_mb_t> (J->mbs_dev); F.coeffs = glb<const int16_t> (J->coeffs_dev); F.slices = glb<const lh264_slice_t> (J->slices_dev);
      F.dy = glb<uint8_t> (J->dst.y_dev); F.du = glb<uint8_t> (J->dst.u_dev); F.dv = glb<uint8_t> (J->dst.v_dev);
      F.mb_w = J->mb_w; F.mb_h = J->mb_h; F.sy = J->stride_y; F.sc = J->stride_c; F.flags = J->flags;
      B.LY = F.mb_w * 16 + 48; B.LC = F.mb_w * 8 + 24; B.FW = F.mb_w * 16;
      lu = B.LY + 2 * B.LC;
      wsync();
      static_assert (sizeof (lh264_pic_t) == 24, "refp mirrors lh264_frame_job_t::ref word for word");
      if (lane < LH264_MAX_REFS * 3) (&L.refp[0][0])[lane] = ((const uint64_t*)J->ref)[lane];
      overlap_ok = false;
      uint64_t prev_dy = 0;
      int prev_h = 1;
      if (ji > first) {
        const lh264_frame_job_t* P = J - 1;
        prev_dy = (uint64_t) (uintptr_t)P->dst.y_dev; prev_h = P->mb_h; F.prev_base = base - P->mb_h;
#ifndef LH264_NO_OVERLAP
        // two frames may be in flight only if this frame's picture is not one the previous frame still reads
        overlap_ok = true;
        for (int k = 0; k < LH264_MAX_REFS; k++) overlap_ok = overlap_ok && P->ref[k].y_dev != J->dst.y_dev;
        overlap_ok = overlap_ok && P->dst.y_dev != J->dst.y_dev;
#endif
      }
      slc_id = -1;
      cur_ji = ji;
      wsync();
      // everything older than the previous frame must be complete (and the previous frame too if pictures alias)
      if (ji > first) wait_prefix (G, L, (overlap_ok ? F.prev_base : base) - 1, NW);
      // ... so nothing reads the frame block of frame ji - 2 any more: it becomes this frame's
      if (lane == 0) {
        LDS FrameLds& W = G.frame[ji & 1];
        W.prev_dy = prev_dy; W.sy = F.sy; W.sc = F.sc; W.mb_w = F.mb_w; W.mb_h = F.mb_h; W.prev_base = F.prev_base; W.prev_h_nw = prev_h | NW << 16;
      }
      wsync();
    }
    // everything older than the previous frame must be complete (and the previous frame too if pictures alias)
    if (ji > first) wait_prefix (G, L, (overlap_ok ? F.prev_base : base) - 1, NW);

    STAMP (10);
    const int g = base + row;
    LDS uint8_t* cur = slots + (g % NL) * slot_bytes;
    const LDS uint8_t* top = slots + ((g + NL - 1) % NL) * slot_bytes;
    B.lineCur = cur; B.lineTop = top; B.fCur = cur + lu; B.fTop = top + lu;
    const int wprev = (wave + NW - 1) % NW;
    const int jprev = row > 0 ? (g - 1 - wprev) / NW : 0;
    Pref pf = prefetch_mb (F, row * F.mb_w, row > 0, lane);
    unsigned long long below = 0;            // bit i: macroblock 64*(x/64)+i of the row below is intra
    unsigned long long ahead = 0;            // bit i: macroblock 64*(x/64)+i+1 of this row is intra
    for (int x = 0; x < F.mb_w; x++) {
      if ((x & 63) == 0) {                   // (before the prefetch: these two loads are waited for at once)
        int t = 0, u = 0;
        if (row + 1 < F.mb_h && x + lane < F.mb_w) t = * (const GLB uint16_t*) (sbase (F.mbs + (size_t) (row + 1) * F.mb_w + x) + lane);
        if (x + 1 + lane < F.mb_w) u = * (const GLB uint16_t*) (sbase (F.mbs + (size_t)row * F.mb_w + x + 1) + lane);
        below = __ballot ((t & LH264_MB_INTRA) != 0);
        ahead = __ballot ((u & LH264_MB_INTRA) != 0);
      }
      Pref nx = pf;
      if (x + 1 < F.mb_w) nx = prefetch_mb (F, row * F.mb_w + x + 1, row > 0, lane);
      // does an intra macroblock read this one's unfiltered bottom row (below-left, below, below-right) / right column?
      // (the type of the next macroblock comes from the row's mask, not from the record just requested: looking at that one here
      // would wait for the prefetch the moment it is issued)
      const int xi = x & 63;
      const bool pub_line = row + 1 < F.mb_h && (xi == 0 || xi >= 62 || ((below >> (xi - 1)) & 7) != 0);
      const bool pub_left = x + 1 < F.mb_w && ((ahead >> xi) & 1) != 0;
      const int need = (jprev << 12) | min (x + 2, F.mb_w);
      STAMP (8);
      // The lane index goes in opaque: otherwise every lane-dependent address and mask of the macroblock's steps is hoisted out of
      // this loop, and at 128 registers 47 of them live in scratch (12.8 KB per wave, more than the L2 holds for a full chip: the
      // reloads were most of the kernel's HBM traffic).  Recomputing them per macroblock costs a few dozen VALU instructions.
#ifndef LH264_HOIST_LANE
      int lane_mb = lane;
      asm volatile ("" : "+v" (lane_mb));
#else
      const int lane_mb = lane;
#endif
#ifdef LH264_STAMP
      process_mb (F, L, G, G.frame[ji & 1], B, pf, x, row, x & 1, slc_id, pub_line, pub_left, lane_mb, &progress[wprev], need, st_t0, st_acc);
#else
      process_mb (F, L, G, G.frame[ji & 1], B, pf, x, row, x & 1, slc_id, pub_line, pub_left, lane_mb, &progress[wprev], need);
#endif
      if (lane == 0) progress[wave] = (jw << 12) | (x + 1);
      pf = nx;
    }
    // ---- row end: wait for this row's stores, pad what became final, publish ----------------------------------
    __builtin_amdgcn_fence (__ATOMIC_RELEASE, "workgroup");
    if (!(F.flags & LH264_JOB_NO_EXPAND)) {
      PadCtx pc;
      pc.dy = F.dy; pc.du = F.du; pc.dv = F.dv; pc.sy = F.sy; pc.sc = F.sc; pc.mb_w = F.mb_w; pc.mb_h = F.mb_h;
      if (row > 0) {                         // the row above is final now (its last 3 sample rows were written by this wave)
        while ((int) (stored[wprev] - jprev) < 0) __builtin_amdgcn_s_sleep (1);
        __builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "workgroup");
        pad_mb_row (pc, row - 1, lane);
      }
      if (row == F.mb_h - 1) pad_mb_row (pc, row, lane);
      __builtin_amdgcn_fence (__ATOMIC_RELEASE, "workgroup");
    }
    if (lane == 0) stored[wave] = jw;
    STAMP (9);
    jw++;
    row += NW;
  }
  STAMP_FLUSH;
}

#ifdef LH264_STAMP
void read_stamps (unsigned long long* out, bool reset) {
  (void)hipMemcpyFromSymbol (out, HIP_SYMBOL (g_stamps), sizeof (g_stamps));
  if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol (HIP_SYMBOL (g_stamps), z, sizeof (z)); }
}
#endif
size_t wave_lds_bytes() { return sizeof (WaveLds); }
size_t wg_lds_bytes() { return (sizeof (WgLds) + 15) & ~ (size_t)15; }

}  // namespace lh264
