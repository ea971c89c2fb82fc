// lh264_coder_dev.h - device-only helpers shared by the two forms of the coder (lh264_coder.hip: wave per (stream, partition);
// lh264_coder_sw.hip: stream per workgroup) and, for the address-space cast, by lh264_ctx.hip and lh264_kernels.hip.  Everything
// here is bit-exact arithmetic of the reference or wave plumbing that both forms must agree on, so it exists once.  Internal, like
// lh264_coder.h: the namespaces of the kernels (lh264, lh264sw) pull lh264dev in with a using directive.
#ifndef LH264_CODER_DEV_H_
#define LH264_CODER_DEV_H_
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lh264.h"

#define GLB __attribute__ ((address_space (1)))
#define LDS __attribute__ ((address_space (3)))

namespace lh264dev {

typedef uint32_t u32x4 __attribute__ ((ext_vector_type (4)));
template <typename T> __device__ __forceinline__ GLB T* glb (const void* p) { return (GLB T*) (uintptr_t)p; }
__device__ __forceinline__ int uniform (int v) { return __builtin_amdgcn_readfirstlane (v); }

// ---- wave-wide inclusive scan over 64 lanes with DPP: Hillis-Steele inside each row of 16 (row_shr 1, 2, 4, 8), then lane 15
// of rows 0 and 2 into rows 1 and 3 (row_bcast:15), then lane 31 into rows 2 and 3 (row_bcast:31).  Lanes without a source add 0.
template <int CTRL, int ROWS> __device__ __forceinline__ int dpp0 (int x) { return __builtin_amdgcn_update_dpp (0, x, CTRL, ROWS, 0xf, false); }
__device__ __forceinline__ int wave_scan_add (int x) {
  x += dpp0<0x111, 0xf> (x); x += dpp0<0x112, 0xf> (x); x += dpp0<0x114, 0xf> (x); x += dpp0<0x118, 0xf> (x);
  x += dpp0<0x142, 0xa> (x); x += dpp0<0x143, 0xc> (x);
  return x;
}

// which lanes of the wave hold the same `nbits`-bit key as this lane (valid lanes only)
template <int NBITS> __device__ __forceinline__ void wave_match (uint32_t key, unsigned long long valid, uint32_t& lo, uint32_t& hi) {
  uint32_t dlo = 0, dhi = 0;
#pragma unroll
  for (int b = 0; b < NBITS; b++) {
    const int xb = __builtin_amdgcn_sbfe ((int)key, b, 1);             // 0 or -1
    const unsigned long long m = __ballot (xb != 0);
    dlo |= (uint32_t)m ^ (uint32_t)xb; dhi |= (uint32_t) (m >> 32) ^ (uint32_t)xb;
  }
  lo = ~dlo & (uint32_t)valid; hi = ~dhi & (uint32_t) (valid >> 32);
}
__device__ __forceinline__ int below (uint32_t lo, uint32_t hi) { return (int)__builtin_amdgcn_mbcnt_hi (hi, __builtin_amdgcn_mbcnt_lo (lo, 0u)); }

// ---- DynProb (compression_stream.h:87-115): the probability from the two counters -------------------------------------------
// floor (256 (c0+1) / (c0+c1+2)) < 256: numerator < 2^18, divisor <= 516: a float quotient is within one of the exact one
__device__ __forceinline__ uint32_t dp_ratio (uint32_t c0, uint32_t c1) {
  const uint32_t num = 256u * (c0 + 1u), den = c0 + c1 + 2u;
  uint32_t prob = (uint32_t) ((float)num * __builtin_amdgcn_rcpf ((float)den));
  if (prob * den > num) prob--;
  else if ((prob + 1u) * den <= num) prob++;
  return prob;
}

// ---- tags ------------------------------------------------------------------------------------------------------------------------
// the tags the coefficient symbols are billed to (the others come with the symbol, in its pad byte)
enum { T_LDC = 17, T_CRDC = 18, T_LAC_0_EOB = 19, T_LAC_N_EOB = 24, T_CRAC_EOB = 29 };
__device__ __forceinline__ int tag_slot (int tag) { return tag == 69 ? 34 : tag; }

// the tag of a coefficient / nonzero-count symbol: the context-index kernel leaves it in the symbol's pad byte (lh264_ctx.hip mk_sym);
// symbols from elsewhere (pad 0) have it taken out of the prior: colour, first scan position and macroblock class (encode4x4)
__device__ __forceinline__ int ac_tag_base (uint32_t prior, int kind, int pad) {
  if (pad) return pad;
  const uint32_t nco = kind == LH264_SYM_AC4 ? 16u : 64u;
  const uint32_t outer = prior / 3125u;
  const int emitted = (int) (outer % nco), color = (int) ((outer / nco) % 3u), code = (int) ((outer / nco / 3u) % 16u);
  const int first = color == 0 && emitted == 0 && code != 1;
  return color ? 29 : (first ? 19 : 24);
}
__device__ __forceinline__ int nz_tag (uint32_t prior, int pad) { return pad ? pad : (((prior / 27u) % 3u) ? 29 : 19); }

// where the coefficient symbols of macroblock k of a picture start (in symbols behind ctx_syms_dev): its fixed slot, or - compact
// layout - the picture's first symbol in the pool + the macroblock's offset
__device__ __forceinline__ size_t ctx_sym_at (const lh264_code_job_t* J, int k) {
  return J->ctx_sym_off_dev ? (size_t)*glb<const unsigned long long> (J->ctx_sym_base_dev) + glb<const uint32_t> (J->ctx_sym_off_dev)[k] : (size_t)k * LH264_CTX_MAX_SYMS;
}

}  // namespace lh264dev

#endif
