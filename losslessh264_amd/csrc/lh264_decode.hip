// lh264_decode.hip - the decode direction behind one C call (include/lh264.h: lh264_decode_batch): n Annex-B streams in host memory ->
// their pictures, cropped and packed as I420 or NV12, in host memory, in device memory or through a sink.  What the reference's console
// application does picture by picture (h264dec.cpp:246-330: DecodeFrameNoDelay, then Write2File of the cropped planes), here per batch
// of independent streams in ROUNDS: every stream of the round contributes its next few pictures, one lh264_recon_chains launch
// reconstructs them (one chain per stream; with opts->pick only intra or IDR pictures are decoded, the others are walked by their headers,
// and every picture is a chain of its own), decode_pack_kernel behind it crops and packs them into the round's output buffer, and the
// download of that buffer runs on a second HIP stream while the host threads parse and stage the next round.  DESIGN.md section 4.6.
// lh264_decode_batch_ex is the same call with a second struct of options: with a colour, decode_pack_rgb_kernel takes the pack kernel's
// place and the round's output buffer holds RGB24 or planar RGB pictures, converted from the planes the pack step would have delivered.
// lh264_decode_batch_ex2 adds a third struct, the sample type: with a float type decode_pack_sample_kernel takes that place and the
// buffer holds float32, float16 or bfloat16 elements, one fused multiply-add of each RGB byte, which itself is never stored.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/lh264.h"
#include "host/h264_parser.h"
#include "host/capi_internal.h"
#include "host/device_mem.h"
#include "lh264_sha1.h"
#include "lh264_slice_cabac.h"

// ---- the pack step: crop + I420 / NV12, host and device from one source ------------------------------------------------------------
// A picture is cut into bands of 16 luma rows (and the 8 chroma rows that belong to them); a band's rows are cut into PIECES: the
// 16-byte blocks of the DESTINATION, counted from the aligned address at or below the row's first byte.  Destinations are tight, so a
// row starts wherever the row before ended: a whole piece is one aligned 16-byte store fed by an unaligned 16-byte load (crop_x is
// even, not 16-aligned), the pieces at a row's head and tail go byte by byte and touch nothing outside the row.
namespace lh264pack {

constexpr int kBandRows = 16;

__host__ __device__ inline uint32_t interleave_lo (uint32_t u, uint32_t v) {      // u0 v0 u1 v1
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm (v, u, 0x05010400u);
#else
  return (u & 0xffu) | (v & 0xffu) << 8 | (u & 0xff00u) << 8 | (v & 0xff00u) << 16;
#endif
}
__host__ __device__ inline uint32_t interleave_hi (uint32_t u, uint32_t v) {      // u2 v2 u3 v3
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm (v, u, 0x07030602u);
#else
  return (u >> 16 & 0xffu) | (v >> 16 & 0xffu) << 8 | (u >> 24) << 16 | (v >> 24) << 24;
#endif
}

// piece p of a row of w bytes copied from s to d
__host__ __device__ inline void piece_copy (uint8_t* d, const uint8_t* s, int w, int p) {
  int a = p * 16 - (int) ((uintptr_t)d & 15u), b = a + 16;
  if (a >= 0 && b <= w) {
    uint4 x;
    __builtin_memcpy (&x, s + a, 16);
    * (uint4*) (d + a) = x;
    return;
  }
  if (a < 0) a = 0;
  if (b > w) b = w;
  for (int k = a; k < b; k++) d[k] = s[k];
}
// piece p of a row of w bytes: Cb and Cr (w / 2 bytes each) interleaved
__host__ __device__ inline void piece_interleave (uint8_t* d, const uint8_t* u, const uint8_t* v, int w, int p) {
  int a = p * 16 - (int) ((uintptr_t)d & 15u), b = a + 16;
  if (a >= 0 && b <= w && !(a & 1)) {
    uint2 x, y;
    __builtin_memcpy (&x, u + (a >> 1), 8);
    __builtin_memcpy (&y, v + (a >> 1), 8);
    uint4 o;
    o.x = interleave_lo (x.x, y.x); o.y = interleave_hi (x.x, y.x); o.z = interleave_lo (x.y, y.y); o.w = interleave_hi (x.y, y.y);
    * (uint4*) (d + a) = o;
    return;
  }
  if (a < 0) a = 0;
  if (b > w) b = w;
  for (int k = a; k < b; k++) d[k] = (k & 1) ? v[k >> 1] : u[k >> 1];
}

// band `band` of one job, worked on by item t of nt (the lanes of a workgroup; the host steps it with t = 0, nt = 1)
__host__ __device__ inline void pack_band (const lh264_pack_job_t& j, int band, int t, int nt) {
  const int w = j.crop_w, h = j.crop_h, cw = w >> 1, ch = h >> 1;
  const int r0 = band * kBandRows, r1 = r0 + kBandRows < h ? r0 + kBandRows : h;
  if (r1 > r0) {
    const int pieces = (w + 30) >> 4, items = (r1 - r0) * pieces;
    const uint8_t* s = j.y + (size_t)j.crop_y * j.stride_y + j.crop_x;
    for (int it = t; it < items; it += nt) {
      const int r = r0 + it / pieces, p = it % pieces;
      piece_copy (j.dst + (size_t)r * w, s + (size_t)r * j.stride_y, w, p);
    }
  }
  const int c0 = band * (kBandRows / 2), c1 = c0 + kBandRows / 2 < ch ? c0 + kBandRows / 2 : ch;
  if (c1 <= c0) return;
  const size_t co = (size_t) (j.crop_y >> 1) * j.stride_c + (j.crop_x >> 1);
  uint8_t* dc = j.dst + (size_t)w * h;
  if (j.format == LH264_FMT_NV12) {
    const int pieces = (w + 30) >> 4, items = (c1 - c0) * pieces;
    for (int it = t; it < items; it += nt) {
      const int r = c0 + it / pieces, p = it % pieces;
      piece_interleave (dc + (size_t)r * w, j.u + co + (size_t)r * j.stride_c, j.v + co + (size_t)r * j.stride_c, w, p);
    }
  } else {
    const int pieces = (cw + 30) >> 4, per_plane = (c1 - c0) * pieces;
    for (int it = t; it < 2 * per_plane; it += nt) {
      const int plane = it >= per_plane, q = it - plane * per_plane;
      const int r = c0 + q / pieces, p = q % pieces;
      piece_copy (dc + (size_t)plane * cw * ch + (size_t)r * cw, (plane ? j.v : j.u) + co + (size_t)r * j.stride_c, cw, p);
    }
  }
}

// ---- the reduced-size pack step: scale_log2 = s in 1..3, B = 1 << s (the definition: include/lh264.h at lh264_decode_batch) ---------
// A plane of w x h window samples is delivered as pw x ph means of B x B blocks, pw = ceil (w / B) for chroma and twice the chroma
// size for luma; block coordinates are clamped to the WINDOW.  The bands are 16 DELIVERED luma rows (and their 8 chroma rows), the
// pieces 4 bytes of the destination counted from the aligned address at or below the row's first byte: a whole piece whose 4 blocks
// lie inside the window is one aligned 4-byte store fed by B unaligned loads of 4 * B bytes; heads, tails and pieces whose blocks
// cross the window's right or bottom edge go sample by sample through the clamped rule.  Byte sums are 4-byte dot products against
// 0x01 masks; the largest sum is 64 * 255.  No LDS; no byte outside the window is read, none outside the picture's bytes written.

// the delivered luma size of a w x h window (both even) at scale s (0..3); the chroma planes are half of it each way
__host__ __device__ inline void scaled_size (int w, int h, int s, int* ow, int* oh) {
  const int B = 1 << s;
  *ow = s ? 2 * (((w >> 1) + B - 1) >> s) : w;
  *oh = s ? 2 * (((h >> 1) + B - 1) >> s) : h;
}

// acc + the bytes of x that mask picks (0x01 per byte)
__host__ __device__ inline uint32_t byte_sum (uint32_t x, uint32_t mask, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4 (x, mask, acc, false);
#else
  for (int k = 0; k < 4; k++) acc += (x >> (8 * k) & 0xffu) * (mask >> (8 * k) & 1u);
  return acc;
#endif
}

// N (2 or 4) neighbouring means whose blocks lie inside the window: B rows of N * B bytes from p -> mean k in byte k
template <int S, int N>
__host__ __device__ inline uint32_t means_whole (const uint8_t* p, int stride) {
  constexpr int B = 1 << S, W = N * B / 4;
  uint32_t acc[N];
  for (int k = 0; k < N; k++) acc[k] = 0;
  for (int r = 0; r < B; r++) {
    uint32_t x[W];
    __builtin_memcpy (x, p + (size_t)r * stride, W * 4);
    if constexpr (S == 1) {
      for (int k = 0; k < N / 2; k++) { acc[2 * k] = byte_sum (x[k], 0x00000101u, acc[2 * k]); acc[2 * k + 1] = byte_sum (x[k], 0x01010000u, acc[2 * k + 1]); }
    } else {
      for (int k = 0; k < N; k++) for (int q = 0; q < B / 4; q++) acc[k] = byte_sum (x[k * (B / 4) + q], 0x01010101u, acc[k]);
    }
  }
  uint32_t o = 0;
  for (int k = 0; k < N; k++) o |= ((acc[k] + (1u << (2 * S - 1))) >> (2 * S)) << (8 * k);
  return o;
}
// the mean at (X, Y) by the definition: a plane whose window of w x h samples begins at p
template <int S>
__host__ __device__ inline uint8_t mean_clamped (const uint8_t* p, int stride, int w, int h, int X, int Y) {
  constexpr int B = 1 << S;
  uint32_t sum = 0;
  for (int j = 0; j < B; j++) {
    const int y = Y * B + j < h - 1 ? Y * B + j : h - 1;
    const uint8_t* row = p + (size_t)y * stride;
    for (int i = 0; i < B; i++) sum += row[X * B + i < w - 1 ? X * B + i : w - 1];
  }
  return (uint8_t) ((sum + (1u << (2 * S - 1))) >> (2 * S));
}

// piece p of delivered row Y (pw bytes at d) of one plane (window w x h at src)
template <int S>
__host__ __device__ inline void piece_means (uint8_t* d, const uint8_t* src, int stride, int w, int h, int pw, int Y, int p) {
  constexpr int B = 1 << S;
  int a = p * 4 - (int) ((uintptr_t)d & 3u), b = a + 4;
  if (a >= 0 && b <= pw && b * B <= w && (Y + 1) * B <= h) {
    * (uint32_t*) (d + a) = means_whole<S, 4> (src + (size_t)Y * B * stride + a * B, stride);
    return;
  }
  if (a < 0) a = 0;
  if (b > pw) b = pw;
  for (int k = a; k < b; k++) d[k] = mean_clamped<S> (src, stride, w, h, k, Y);
}
// piece p of delivered NV12 chroma row Y (ow bytes at d): the Cb and Cr means (windows cw x ch at u and v) interleaved
template <int S>
__host__ __device__ inline void piece_means_interleave (uint8_t* d, const uint8_t* u, const uint8_t* v, int stride, int cw, int ch, int ow, int Y, int p) {
  constexpr int B = 1 << S;
  int a = p * 4 - (int) ((uintptr_t)d & 3u), b = a + 4;
  if (a >= 0 && b <= ow && !(a & 1) && (b >> 1) * B <= cw && (Y + 1) * B <= ch) {
    const size_t at = (size_t)Y * B * stride + (a >> 1) * B;
    * (uint32_t*) (d + a) = interleave_lo (means_whole<S, 2> (u + at, stride), means_whole<S, 2> (v + at, stride));
    return;
  }
  if (a < 0) a = 0;
  if (b > ow) b = ow;
  for (int k = a; k < b; k++) d[k] = mean_clamped<S> ((k & 1) ? v : u, stride, cw, ch, k >> 1, Y);
}

template <int S>
__host__ __device__ inline void pack_band_scaled_by (const lh264_pack_job_t& j, int band, int t, int nt) {
  const int w = j.crop_w, h = j.crop_h, cw = w >> 1, ch = h >> 1;
  int ow, oh;
  scaled_size (w, h, S, &ow, &oh);
  const int ocw = ow >> 1, och = oh >> 1;
  const int r0 = band * kBandRows, r1 = r0 + kBandRows < oh ? r0 + kBandRows : oh;
  if (r1 > r0) {
    const int pieces = (ow + 6) >> 2, items = (r1 - r0) * pieces;
    const uint8_t* s = j.y + (size_t)j.crop_y * j.stride_y + j.crop_x;
    for (int it = t; it < items; it += nt) {
      const int r = r0 + it / pieces, p = it % pieces;
      piece_means<S> (j.dst + (size_t)r * ow, s, j.stride_y, w, h, ow, r, p);
    }
  }
  const int c0 = band * (kBandRows / 2), c1 = c0 + kBandRows / 2 < och ? c0 + kBandRows / 2 : och;
  if (c1 <= c0) return;
  const size_t co = (size_t) (j.crop_y >> 1) * j.stride_c + (j.crop_x >> 1);
  uint8_t* dc = j.dst + (size_t)ow * oh;
  if (j.format == LH264_FMT_NV12) {
    const int pieces = (ow + 6) >> 2, items = (c1 - c0) * pieces;
    for (int it = t; it < items; it += nt) {
      const int r = c0 + it / pieces, p = it % pieces;
      piece_means_interleave<S> (dc + (size_t)r * ow, j.u + co, j.v + co, j.stride_c, cw, ch, ow, r, p);
    }
  } else {
    const int pieces = (ocw + 6) >> 2, per_plane = (c1 - c0) * pieces;
    for (int it = t; it < 2 * per_plane; it += nt) {
      const int plane = it >= per_plane, q = it - plane * per_plane;
      const int r = c0 + q / pieces, p = q % pieces;
      piece_means<S> (dc + (size_t)plane * ocw * och + (size_t)r * ocw, (plane ? j.v : j.u) + co, j.stride_c, cw, ch, ocw, r, p);
    }
  }
}
// band `band` (of DELIVERED rows) of one job whose `reserved` word is its scale_log2 (1..3; anything else: nothing is done),
// worked on by item t of nt (the host steps it with t = 0, nt = 1)
__host__ __device__ inline void pack_band_scaled (const lh264_pack_job_t& j, int band, int t, int nt) {
  if (j.reserved == 1) pack_band_scaled_by<1> (j, band, t, nt);
  else if (j.reserved == 2) pack_band_scaled_by<2> (j, band, t, nt);
  else if (j.reserved == 3) pack_band_scaled_by<3> (j, band, t, nt);
}

// ---- the pack step to one given size: out_width x out_height (the definition: include/lh264.h at lh264_decode_batch) ---------------
// Every plane of w x h window samples is delivered as ow x oh exact area means: ow x oh for luma, half of it each way for chroma,
// whatever the window is.  Delivered column X covers the interval [X*w, (X+1)*w) of a line on which every source column is ow long:
// source columns x0 = X*w / ow .. x1 = ((X+1)*w - 1) / ow, the two end columns by what they share with the interval, every column
// between them by ow; the weights of one X sum to w.  Rows likewise with h and oh.  S = the weighted sum, D = w*h, the sample is
// (2*S + D) / (2*D), round half up.  A row's sum is at most 255*w; S is kept in 64 bits, since the front end delivers windows of up
// to 139,264 macroblocks (35.7 M samples) and 2*S + D passes 2^32 at 8.4 M.  The bands are 16 delivered luma rows (and their 8 chroma
// rows), the pieces 4 bytes of the destination counted from the aligned address at or below the row's first byte: a whole piece is
// one aligned 4-byte store, heads and tails go sample by sample.  The spans and weights of a piece's row are worked out once per
// piece, those of a column once per sample, never per source row.  The bytes between a span's end columns are summed by unaligned
// 4-byte loads and dot products, the last 0..3 of them byte by byte: no byte outside the window is read, none outside the picture's
// bytes written.  No LDS.

// what a call delivers for a w x h window: out_w x out_h where a size is set (both non-zero), else the window at scale s
__host__ __device__ inline void delivered_size (int w, int h, int s, int out_w, int out_h, int* ow, int* oh) {
  if (out_w) { *ow = out_w; *oh = out_h; }
  else scaled_size (w, h, s, ow, oh);
}

// the source columns (or rows) of one delivered column (or row): a .. b, `wa` of a and `wb` of b, every one between them whole.
// (a == b: the one column carries the whole weight in wa, wb = 0)
struct Span { int a, b; uint32_t wa, wb; };
__host__ __device__ inline Span span_of (uint32_t X, uint32_t w, uint32_t ow) {
  const uint32_t lo = X * w, hi = lo + w;      // (X < 4096, w <= 16384)
  Span s;
  s.a = (int) (lo / ow); s.b = (int) ((hi - 1) / ow);
  if (s.a == s.b) { s.wa = w; s.wb = 0; }
  else { s.wa = (uint32_t) (s.a + 1) * ow - lo; s.wb = hi - (uint32_t)s.b * ow; }
  return s;
}
// the weighted sum of one source row over the span sx (every whole column weighs ow)
__host__ __device__ inline uint32_t row_sum (const uint8_t* row, const Span& sx, uint32_t ow) {
  const uint8_t* q = row + sx.a + 1;
  int n = sx.b - sx.a - 1;
  uint32_t mid = 0;
  for (; n >= 4; n -= 4, q += 4) { uint32_t x; __builtin_memcpy (&x, q, 4); mid = byte_sum (x, 0x01010101u, mid); }
  for (; n > 0; n--) mid += *q++;
  return sx.wa * row[sx.a] + ow * mid + sx.wb * row[sx.b];
}
// floor ((2*S + D) / (2*D)) for a quotient of at most 255: a float estimate, then made exact against the remainder
__host__ __device__ inline uint8_t rounded_mean (uint64_t S, uint64_t D) {
  const uint64_t num = 2 * S + D, den = 2 * D;
  uint32_t q = (uint32_t) ((float)num / (float)den);
  int64_t r = (int64_t)num - (int64_t) (q * den);
  while (r < 0) { q--; r += (int64_t)den; }
  while (r >= (int64_t)den) { q++; r -= (int64_t)den; }
  return (uint8_t)q;
}
// one plane as the resize step sees it: the window's first sample, its size, the delivered size
struct ResizePlane { const uint8_t* p; int stride; uint32_t w, h, ow, oh; };
// delivered sample X of the delivered row whose source rows are sy
__host__ __device__ inline uint8_t resized_sample (const ResizePlane& pl, const Span& sy, int X) {
  const Span sx = span_of ((uint32_t)X, pl.w, pl.ow);
  const uint8_t* row = pl.p + (size_t)sy.a * pl.stride;
  uint64_t S = (uint64_t)sy.wa * row_sum (row, sx, pl.ow);
  for (int y = sy.a + 1; y < sy.b; y++) { row += pl.stride; S += (uint64_t)pl.oh * row_sum (row, sx, pl.ow); }
  if (sy.wb) S += (uint64_t)sy.wb * row_sum (pl.p + (size_t)sy.b * pl.stride, sx, pl.ow);
  return rounded_mean (S, (uint64_t)pl.w * pl.h);
}
// piece p of delivered row Y (n bytes at d): byte k is sample k of plane a - or, interleaved (NV12 chroma), sample k / 2 of a (k even) or b
__host__ __device__ inline void piece_resized (uint8_t* d, int n, int Y, int p, const ResizePlane& a, const ResizePlane& b, bool interleaved) {
  int k0 = p * 4 - (int) ((uintptr_t)d & 3u), k1 = k0 + 4;
  const bool whole = k0 >= 0 && k1 <= n;
  if (k0 < 0) k0 = 0;
  if (k1 > n) k1 = n;
  if (k1 <= k0) return;
  const Span sy = span_of ((uint32_t)Y, a.h, a.oh);
  uint32_t o = 0;
  for (int k = k0; k < k1; k++) {
    const uint8_t v = interleaved ? resized_sample ((k & 1) ? b : a, sy, k >> 1) : resized_sample (a, sy, k);
    if (whole) o |= (uint32_t)v << (8 * (k - k0));
    else d[k] = v;
  }
  if (whole) * (uint32_t*) (d + k0) = o;
}
// band `band` (16 delivered luma rows, 8 chroma rows) of one job delivered as ow x oh, worked on by item t of nt (the host steps it
// with t = 0, nt = 1)
__host__ __device__ inline void pack_band_resized (const lh264_pack_job_t& j, int ow, int oh, int band, int t, int nt) {
  const int w = j.crop_w, h = j.crop_h, ocw = ow >> 1, och = oh >> 1;
  const int r0 = band * kBandRows, r1 = r0 + kBandRows < oh ? r0 + kBandRows : oh;
  if (r1 > r0) {
    const ResizePlane y = {j.y + (size_t)j.crop_y * j.stride_y + j.crop_x, j.stride_y, (uint32_t)w, (uint32_t)h, (uint32_t)ow, (uint32_t)oh};
    const int pieces = (ow + 6) >> 2, items = (r1 - r0) * pieces;
    for (int it = t; it < items; it += nt) {
      const int r = r0 + it / pieces, p = it % pieces;
      piece_resized (j.dst + (size_t)r * ow, ow, r, p, y, y, false);
    }
  }
  const int c0 = band * (kBandRows / 2), c1 = c0 + kBandRows / 2 < och ? c0 + kBandRows / 2 : och;
  if (c1 <= c0) return;
  const size_t co = (size_t) (j.crop_y >> 1) * j.stride_c + (j.crop_x >> 1);
  const ResizePlane u = {j.u + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t)ocw, (uint32_t)och};
  const ResizePlane v = {j.v + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t)ocw, (uint32_t)och};
  uint8_t* dc = j.dst + (size_t)ow * oh;
  if (j.format == LH264_FMT_NV12) {
    const int pieces = (ow + 6) >> 2, items = (c1 - c0) * pieces;
    for (int it = t; it < items; it += nt) {
      const int r = c0 + it / pieces, p = it % pieces;
      piece_resized (dc + (size_t)r * ow, ow, r, p, u, v, true);
    }
  } else {
    const int pieces = (ocw + 6) >> 2, per_plane = (c1 - c0) * pieces;
    for (int it = t; it < 2 * per_plane; it += nt) {
      const int plane = it >= per_plane, q = it - plane * per_plane;
      const int r = c0 + q / pieces, p = q % pieces;
      piece_resized (dc + (size_t)plane * ocw * och + (size_t)r * ocw, ocw, r, p, plane ? v : u, u, false);
    }
  }
}
// what the resize entry points and the call accept as a size: both even, 2..4096
inline bool size_ok (int64_t out_w, int64_t out_h) {
  return out_w >= 2 && out_w <= 4096 && out_h >= 2 && out_h <= 4096 && !((out_w | out_h) & 1);
}

// ---- the placed pack step: LH264_FIT_CONTAIN (the definition: include/lh264.h at lh264_decode_batch_ex3) ---------------------------
// The window is resampled to pl.w x pl.h - resized_sample with the plane's ow, oh set to that and the coordinates shifted - and lies at
// (pl.x, pl.y) of the ow x oh picture; every other sample is the fill.  Bands and pieces are those of the step to one size.  A piece
// whose bytes lie wholly in a bar is one aligned 4-byte store of a word built from the fill and computes nothing, a piece wholly inside
// the rectangle is the resize step's piece, only a piece on a seam decides per sample.  All rectangles are even, so the chroma planes'
// are the luma's halved.  No byte outside the window is read, none outside the picture's bytes written.  No LDS.

// piece p of delivered row Y (n bytes at d): bytes b0 .. b1 - 1 of rows y0 .. y0 + a.oh - 1 are the picture's, byte k of them sample
// k - b0 of plane a (interleaved: sample (k - b0) / 2 of a or b, b0 even); every other byte is fa (k even) or fb (k odd)
__host__ __device__ inline void piece_placed (uint8_t* d, int n, int Y, int p, const ResizePlane& a, const ResizePlane& b, bool interleaved,
                                              int b0, int b1, int y0, uint32_t fa, uint32_t fb) {
  int k0 = p * 4 - (int) ((uintptr_t)d & 3u), k1 = k0 + 4;
  const bool whole = k0 >= 0 && k1 <= n;
  if (k0 < 0) k0 = 0;
  if (k1 > n) k1 = n;
  if (k1 <= k0) return;
  if (Y < y0 || Y >= y0 + (int)a.oh || k1 <= b0 || k0 >= b1) {      // wholly in a bar
    if (whole) { const uint32_t pair = (k0 & 1) ? fb | fa << 8 : fa | fb << 8; * (uint32_t*) (d + k0) = pair | pair << 16; }
    else for (int k = k0; k < k1; k++) d[k] = (uint8_t) ((k & 1) ? fb : fa);
    return;
  }
  const Span sy = span_of ((uint32_t) (Y - y0), a.h, a.oh);
  uint32_t o = 0;
  for (int k = k0; k < k1; k++) {
    uint8_t v;
    if (k < b0 || k >= b1) v = (uint8_t) ((k & 1) ? fb : fa);
    else { const int x = k - b0; v = interleaved ? resized_sample ((x & 1) ? b : a, sy, x >> 1) : resized_sample (a, sy, x); }
    if (whole) o |= (uint32_t)v << (8 * (k - k0));
    else d[k] = v;
  }
  if (whole) * (uint32_t*) (d + k0) = o;
}
// band `band` (16 delivered luma rows, 8 chroma rows) of one job delivered as ow x oh with its window placed by pl, worked on by item
// t of nt (the host steps it with t = 0, nt = 1)
__host__ __device__ inline void pack_band_placed (const lh264_pack_job_t& j, const lh264_pack_place_t& pl, int ow, int oh, int band, int t, int nt) {
  const int w = j.crop_w, h = j.crop_h, ocw = ow >> 1, och = oh >> 1;
  const uint32_t fy = pl.fill & 0xffu, fcb = pl.fill >> 8 & 0xffu, fcr = pl.fill >> 16 & 0xffu;
  const int r0 = band * kBandRows, r1 = r0 + kBandRows < oh ? r0 + kBandRows : oh;
  if (r1 > r0) {
    const ResizePlane y = {j.y + (size_t)j.crop_y * j.stride_y + j.crop_x, j.stride_y, (uint32_t)w, (uint32_t)h, (uint32_t)pl.w, (uint32_t)pl.h};
    const int pieces = (ow + 6) >> 2, items = (r1 - r0) * pieces;
    for (int it = t; it < items; it += nt) {
      const int r = r0 + it / pieces, p = it % pieces;
      piece_placed (j.dst + (size_t)r * ow, ow, r, p, y, y, false, pl.x, pl.x + pl.w, pl.y, fy, fy);
    }
  }
  const int c0 = band * (kBandRows / 2), c1 = c0 + kBandRows / 2 < och ? c0 + kBandRows / 2 : och;
  if (c1 <= c0) return;
  const size_t co = (size_t) (j.crop_y >> 1) * j.stride_c + (j.crop_x >> 1);
  const ResizePlane u = {j.u + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pl.w >> 1), (uint32_t) (pl.h >> 1)};
  const ResizePlane v = {j.v + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pl.w >> 1), (uint32_t) (pl.h >> 1)};
  uint8_t* dc = j.dst + (size_t)ow * oh;
  if (j.format == LH264_FMT_NV12) {
    const int pieces = (ow + 6) >> 2, items = (c1 - c0) * pieces;
    for (int it = t; it < items; it += nt) {
      const int r = c0 + it / pieces, p = it % pieces;
      piece_placed (dc + (size_t)r * ow, ow, r, p, u, v, true, pl.x, pl.x + pl.w, pl.y >> 1, fcb, fcr);
    }
  } else {
    const int pieces = (ocw + 6) >> 2, per_plane = (c1 - c0) * pieces;
    for (int it = t; it < 2 * per_plane; it += nt) {
      const int plane = it >= per_plane, q = it - plane * per_plane;
      const int r = c0 + q / pieces, p = q % pieces;
      const uint32_t f = plane ? fcr : fcb;
      piece_placed (dc + (size_t)plane * ocw * och + (size_t)r * ocw, ocw, r, p, plane ? v : u, u, false, pl.x >> 1, (pl.x + pl.w) >> 1, pl.y >> 1, f, f);
    }
  }
}
// what the placed entry points and the call accept as a place: an even rectangle of at least 2 x 2 inside out_w x out_h, a 24-bit fill
inline bool place_ok (const lh264_pack_place_t& pl, int out_w, int out_h) {
  return pl.x >= 0 && pl.y >= 0 && pl.w >= 2 && pl.h >= 2 && !((pl.x | pl.y | pl.w | pl.h) & 1) && pl.x <= out_w - pl.w && pl.y <= out_h - pl.h &&
         !(pl.fill >> 24) && pl.reserved == 0;
}

// ---- the pack step to RGB: lh264_decode_batch_ex (the definition: include/lh264.h at lh264_decode_batch_ex) -------------------------
// The delivered planes are never stored: a sample of the ow x oh luma plane or of the ow/2 x oh/2 chroma planes is worked out where it
// is needed, by the rule of the job's sizing - the window's own sample, mean_clamped / means_whole of the reduced-size step, or
// resized_sample of the step to one size - and goes through the integer function with the factors of LH264_COLOUR_FACTORS.  The bands
// are 16 delivered luma rows = 8 PAIRS of rows; a pair's rows are cut into pieces of 8 pixels' bytes (24 in RGB24, 8 per plane in
// RGBP) of the DESTINATION, counted from the aligned address at or below the first byte of the pair's upper row - and of its lower row,
// whose alignment differs by 0 or 2 (a row is 3*ow or ow bytes, ow even).  An item is one piece of both rows: it converts the 2x2 quads
// under its bytes, each quad's chroma sample and chroma terms once for its four pixels (a quad on the seam of two pieces is worked out
// by both: 5 or 6 quads per item where 4 are its own), lays the pixels out as the row's byte stream in registers, and shifts the
// stream to the piece's alignment.  A whole piece leaves as aligned 4-byte stores, the pieces at a row's head and tail byte by byte: no
// byte outside the window is read, none outside the picture's bytes written.  No LDS.
constexpr int32_t kColourFactors[4][5] = LH264_COLOUR_FACTORS;
constexpr int kRgbQuads = 6;       // the quads an item can touch: 8 pixels' bytes at any alignment of either row lie within 12 pixels

// clamp to 0..255.  On the device one v_med3_i32, written out: left to the compiler, two neighbouring clamps of shifted sums are fused
// into gfx950's v_ashr_pk_u8_i32, and the bytes that came back from an MI355X for exactly those pairs were not the clamp's where a sum
// was negative
__host__ __device__ inline uint32_t clip8 (int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  int32_t r;
  asm ("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(v), "v"(255));
  return (uint32_t)r;
#else
  return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v;
#endif
}

// delivered sample (X, Y) of one plane under sizing M: 0 the window, 1..3 the means of scale_log2, 4 the given size (sy: the rows of Y)
template <int M>
__host__ __device__ inline int plane_sample (const ResizePlane& pl, const Span& sy, int X, int Y) {
  if constexpr (M == 0) return pl.p[(size_t)Y * pl.stride + X];
  else if constexpr (M <= 3) return mean_clamped<M> (pl.p, pl.stride, (int)pl.w, (int)pl.h, X, Y);
  else return resized_sample (pl, sy, X);
}
// delivered luma samples (X, Y) and (X + 1, Y), X even: the second in bits 8..15
template <int M>
__host__ __device__ inline uint32_t luma_pair (const ResizePlane& pl, const Span& sy, int X, int Y) {
  if constexpr (M >= 1 && M <= 3) {
    constexpr int B = 1 << M;
    if ((X + 2) * B <= (int)pl.w && (Y + 1) * B <= (int)pl.h) return means_whole<M, 2> (pl.p + (size_t)Y * B * pl.stride + X * B, pl.stride) & 0xffffu;
  }
  return (uint32_t)plane_sample<M> (pl, sy, X, Y) | (uint32_t)plane_sample<M> (pl, sy, X + 1, Y) << 8;
}

// the 2x2 quad whose first pixel is delivered luma sample (X, 2*R), X even: the chroma sample and the chroma terms once for its four
// pixels -> o[rr][i][c] = channel c (0 R, 1 G, 2 B) of pixel (X + i, 2*R + rr).  The one place where a pixel is converted: piece_rgb
// and piece_sample both read their bytes here
template <int M>
__host__ __device__ inline void quad_rgb (const ResizePlane& py, const ResizePlane& pu, const ResizePlane& pv, const Span* sy, const Span& sc,
                                          const int32_t* f, int y0, int X, int R, uint32_t o[2][2][3]) {
  const int D = plane_sample<M> (pu, sc, X >> 1, R) - 128, E = plane_sample<M> (pv, sc, X >> 1, R) - 128;
  const int32_t tr = f[1] * E + 32768, tg = 32768 - f[3] * D - f[4] * E, tb = f[2] * D + 32768;
  _Pragma ("unroll")
  for (int rr = 0; rr < 2; rr++) {
    const uint32_t yy = luma_pair<M> (py, sy[rr], X, 2 * R + rr);
    _Pragma ("unroll")
    for (int i = 0; i < 2; i++) {
      const int32_t yt = f[0] * ((int32_t) (yy >> (8 * i) & 0xffu) - y0);
      o[rr][i][0] = clip8 ((yt + tr) >> 16); o[rr][i][1] = clip8 ((yt + tg) >> 16); o[rr][i][2] = clip8 ((yt + tb) >> 16);
    }
  }
}

// sizing M = 5, "placed" (LH264_FIT_CONTAIN): the planes' ow x oh is the rectangle the window is resampled to, which lies at (x, y) of
// the delivered picture; every pixel outside it is the conversion of the fill.  x, y and the rectangle are even, so a quad is wholly
// picture - quad_rgb<4> with the coordinates shifted - or wholly bar
struct Placed { int x, y; uint32_t fill; };
// the bar's pixel: quad_rgb's arithmetic on (fill_y, fill_cb, fill_cr), once per item
__host__ __device__ inline void bar_rgb (uint32_t fill, const int32_t* f, int y0, uint32_t o[3]) {
  const int D = (int) (fill >> 8 & 0xffu) - 128, E = (int) (fill >> 16 & 0xffu) - 128;
  const int32_t yt = f[0] * ((int32_t) (fill & 0xffu) - y0);
  o[0] = clip8 ((yt + f[1] * E + 32768) >> 16); o[1] = clip8 ((yt + 32768 - f[3] * D - f[4] * E) >> 16); o[2] = clip8 ((yt + f[2] * D + 32768) >> 16);
}

// piece p of row pair R of one job delivered as ow x oh in layout L (LH264_COLOUR_RGB24 / _RGBP) with the factors f and luma offset y0
// (pc: read under M = 5 only)
template <int M, int L>
__host__ __device__ inline void piece_rgb (uint8_t* dst, const ResizePlane& py, const ResizePlane& pu, const ResizePlane& pv, int ow, int oh,
                                           const int32_t* f, int y0, int R, int p, const Placed& pc) {
  constexpr int BPP = L == (int)LH264_COLOUR_RGB24 ? 3 : 1, NP = L == (int)LH264_COLOUR_RGB24 ? 1 : 3;      // bytes per pixel and planes of the destination
  constexpr int PB = 8 * BPP, ND = PB / 4, NW = 12 * BPP / 4;                                                 // a piece's bytes and words; the words of 12 pixels
  const int row_bytes = BPP * ow;
  uint8_t* d[2] = {dst + (size_t) (2 * R) * row_bytes, dst + (size_t) (2 * R + 1) * row_bytes};
  int a[2];
  for (int rr = 0; rr < 2; rr++) a[rr] = p * PB - (int) ((uintptr_t)d[rr] & 3u);
  if ((a[0] < a[1] ? a[0] : a[1]) >= row_bytes) return;
  // the first pixel of the item's 12: the even pixel at or below the first byte of either row's piece (a may be -3 .. -1 at a row's head)
  const int amin = a[0] < a[1] ? a[0] : a[1];
  const int x0 = 2 * ((amin + 2 * BPP * 4) / (2 * BPP) - 4);
  Span sy[2], sc;
  if constexpr (M == 4) { sy[0] = span_of ((uint32_t) (2 * R), py.h, py.oh); sy[1] = span_of ((uint32_t) (2 * R + 1), py.h, py.oh); sc = span_of ((uint32_t)R, pu.h, pu.oh); }
  else { sy[0] = sy[1] = sc = Span(); }
  // M = 5: the bar's pixel, and whether the pair's rows cross the rectangle at all (then their spans, counted from its first row)
  uint32_t bar[3] = {0, 0, 0};
  bool rows_in = false;
  if constexpr (M == 5) {
    bar_rgb (pc.fill, f, y0, bar);
    rows_in = 2 * R >= pc.y && 2 * R < pc.y + (int)py.oh;
    if (rows_in) { sy[0] = span_of ((uint32_t) (2 * R - pc.y), py.h, py.oh); sy[1] = span_of ((uint32_t) (2 * R + 1 - pc.y), py.h, py.oh); sc = span_of ((uint32_t) (R - (pc.y >> 1)), pu.h, pu.oh); }
  }
  // the 12 pixels of both rows as byte streams: RGB24 one stream of 36 bytes, RGBP three of 12
  uint32_t W[2][NP][NW + 1];
  for (int rr = 0; rr < 2; rr++) for (int c = 0; c < NP; c++) for (int k = 0; k <= NW; k++) W[rr][c][k] = 0;
  _Pragma ("unroll")
  for (int q = 0; q < kRgbQuads; q++) {
    const int X = x0 + 2 * q;
    if (X < 0 || X >= ow) continue;
    uint32_t px[2][2][3];
    if constexpr (M == 5) {
      if (rows_in && X >= pc.x && X < pc.x + (int)py.ow) quad_rgb<4> (py, pu, pv, sy, sc, f, y0, X - pc.x, R - (pc.y >> 1), px);
      else for (int rr = 0; rr < 2; rr++) for (int i = 0; i < 2; i++) for (int c = 0; c < 3; c++) px[rr][i][c] = bar[c];
    } else quad_rgb<M> (py, pu, pv, sy, sc, f, y0, X, R, px);
    _Pragma ("unroll")
    for (int rr = 0; rr < 2; rr++) {
      _Pragma ("unroll")
      for (int i = 0; i < 2; i++) {
        const uint32_t r = px[rr][i][0], g = px[rr][i][1], b = px[rr][i][2];
        const int k = 2 * q + i;                                   // the pixel's place among the 12
        if constexpr (L == (int)LH264_COLOUR_RGB24) {
          const uint32_t px = r | g << 8 | b << 16;
          const int bit = 24 * k;                                  // (compile-time once the loops are unrolled)
          W[rr][0][bit >> 5] |= px << (bit & 31);
          if ((bit & 31) > 8) W[rr][0][(bit >> 5) + 1] |= px >> (32 - (bit & 31));
        } else {
          W[rr][0][k >> 2] |= r << (8 * (k & 3)); W[rr][1][k >> 2] |= g << (8 * (k & 3)); W[rr][2][k >> 2] |= b << (8 * (k & 3));
        }
      }
    }
  }
  for (int rr = 0; rr < 2; rr++) {
    if (a[rr] >= row_bytes) continue;
    const int s = a[rr] - BPP * x0;                                // where the piece begins in the stream: 0 .. 2*BPP + 1
    const int h = s >> 2, sh = 8 * (s & 3);
    const bool whole = a[rr] >= 0 && a[rr] + PB <= row_bytes;
    for (int c = 0; c < NP; c++) {
      uint8_t* o = d[rr] + (size_t)c * ow * oh + a[rr];
      _Pragma ("unroll")
      for (int j = 0; j < ND; j++) {
        // word j of the piece = stream bytes s + 4*j .. s + 4*j + 3; s < 8, so it begins in word j or j + 1 (j + 2 <= NW in both layouts)
        const uint32_t lo = h ? W[rr][c][j + 1] : W[rr][c][j], hi = h ? W[rr][c][j + 2] : W[rr][c][j + 1];
        const uint32_t v = sh ? lo >> sh | hi << (32 - sh) : lo;
        if (whole) * (uint32_t*) (o + 4 * j) = v;
        else for (int i = 0; i < 4; i++) { const int at = a[rr] + 4 * j + i; if (at >= 0 && at < row_bytes) o[4 * j + i] = (uint8_t) (v >> (8 * i)); }
      }
    }
  }
}

// band `band` (16 delivered luma rows) of one job delivered as ow x oh RGB, worked on by item t of nt (the host steps it with t = 0, nt = 1)
// (pl: the job's place, read under M = 5 only - the planes are then resampled to pl->w x pl->h)
template <int M, int L>
__host__ __device__ inline void pack_band_rgb_as (const lh264_pack_job_t& j, int ow, int oh, int std_byte, int band, int t, int nt, const lh264_pack_place_t* pl = nullptr) {
  const int w = j.crop_w, h = j.crop_h;
  const int R0 = band * (kBandRows / 2), R1 = R0 + kBandRows / 2 < (oh >> 1) ? R0 + kBandRows / 2 : (oh >> 1);
  if (R1 <= R0) return;
  const size_t co = (size_t) (j.crop_y >> 1) * j.stride_c + (j.crop_x >> 1);
  const int pw = M == 5 ? pl->w : ow, ph = M == 5 ? pl->h : oh;
  const Placed pc = M == 5 ? Placed {pl->x, pl->y, pl->fill} : Placed {0, 0, 0u};
  const ResizePlane py = {j.y + (size_t)j.crop_y * j.stride_y + j.crop_x, j.stride_y, (uint32_t)w, (uint32_t)h, (uint32_t)pw, (uint32_t)ph};
  const ResizePlane pu = {j.u + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pw >> 1), (uint32_t) (ph >> 1)};
  const ResizePlane pv = {j.v + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pw >> 1), (uint32_t) (ph >> 1)};
  int32_t f[5];
  for (int k = 0; k < 5; k++) f[k] = kColourFactors[std_byte & 3][k];
  const int y0 = (std_byte & 2) ? 0 : 16;
  constexpr int PB = L == (int)LH264_COLOUR_RGB24 ? 24 : 8;
  const int row_bytes = (L == (int)LH264_COLOUR_RGB24 ? 3 : 1) * ow;
  const int pieces = (row_bytes + 3 + PB - 1) / PB, items = (R1 - R0) * pieces;
  for (int it = t; it < items; it += nt) piece_rgb<M, L> (j.dst, py, pu, pv, ow, oh, f, y0, R0 + it / pieces, it % pieces, pc);
}
// ... of a job whose sizing is its `reserved` scale (out_w == 0) or the given size; layout and standard byte as given.  Anything that is
// not defined: nothing is done
__host__ __device__ inline void pack_band_rgb (const lh264_pack_job_t& j, int out_w, int out_h, int layout, int std_byte, int band, int t, int nt) {
  if (j.crop_w <= 0 || j.crop_h <= 0 || j.reserved < 0 || j.reserved > 3 || (out_w && j.reserved)) return;
  int ow, oh;
  delivered_size (j.crop_w, j.crop_h, j.reserved, out_w, out_h, &ow, &oh);
  const int m = out_w ? 4 : j.reserved;
  if (layout == (int)LH264_COLOUR_RGB24) {
    if (m == 0) pack_band_rgb_as<0, (int)LH264_COLOUR_RGB24> (j, ow, oh, std_byte, band, t, nt);
    else if (m == 1) pack_band_rgb_as<1, (int)LH264_COLOUR_RGB24> (j, ow, oh, std_byte, band, t, nt);
    else if (m == 2) pack_band_rgb_as<2, (int)LH264_COLOUR_RGB24> (j, ow, oh, std_byte, band, t, nt);
    else if (m == 3) pack_band_rgb_as<3, (int)LH264_COLOUR_RGB24> (j, ow, oh, std_byte, band, t, nt);
    else pack_band_rgb_as<4, (int)LH264_COLOUR_RGB24> (j, ow, oh, std_byte, band, t, nt);
  } else if (layout == (int)LH264_COLOUR_RGBP) {
    if (m == 0) pack_band_rgb_as<0, (int)LH264_COLOUR_RGBP> (j, ow, oh, std_byte, band, t, nt);
    else if (m == 1) pack_band_rgb_as<1, (int)LH264_COLOUR_RGBP> (j, ow, oh, std_byte, band, t, nt);
    else if (m == 2) pack_band_rgb_as<2, (int)LH264_COLOUR_RGBP> (j, ow, oh, std_byte, band, t, nt);
    else if (m == 3) pack_band_rgb_as<3, (int)LH264_COLOUR_RGBP> (j, ow, oh, std_byte, band, t, nt);
    else pack_band_rgb_as<4, (int)LH264_COLOUR_RGBP> (j, ow, oh, std_byte, band, t, nt);
  }
}
// ... of a job placed by pl in an out_w x out_h picture (LH264_FIT_CONTAIN)
__host__ __device__ inline void pack_band_rgb_placed (const lh264_pack_job_t& j, const lh264_pack_place_t& pl, int out_w, int out_h, int layout, int std_byte, int band, int t, int nt) {
  if (j.crop_w <= 0 || j.crop_h <= 0 || j.reserved) return;
  if (layout == (int)LH264_COLOUR_RGB24) pack_band_rgb_as<5, (int)LH264_COLOUR_RGB24> (j, out_w, out_h, std_byte, band, t, nt, &pl);
  else if (layout == (int)LH264_COLOUR_RGBP) pack_band_rgb_as<5, (int)LH264_COLOUR_RGBP> (j, out_w, out_h, std_byte, band, t, nt, &pl);
}

// ---- the pack step to float RGB: lh264_decode_batch_ex2 with a float sample type (the definition: include/lh264.h at that call) -------
// Element e of a picture is fma ((float) c, mul[ch], add[ch]) of byte e of the RGB picture above, as binary32, binary16 or bfloat16; the
// bytes come from quad_rgb, the code piece_rgb reads, and never reach memory.  Every row of every plane begins at a multiple of 4 bytes
// (ow and oh are even, the picture's first byte is 4-aligned), so nothing is shifted to the destination: the bands are 16 delivered luma
// rows = 8 pairs of rows, an item is 8 pixels of both rows of a pair counted from pixel 0 - 4 quads, 24 elements a row in RGB24, 8 a
// row and plane in RGBP.  A row of a plane whose address is a multiple of 16 leaves as aligned 16-byte stores (an item's bytes are a
// multiple of 16 in every type and layout, so the row's alignment is every item's: the choice is uniform over the workgroup), any other
// row and the last item of a row whose ow is no multiple of 8 (its 1..3 quads) as aligned 4-byte stores.  Lane t takes items t, t + nt,
// ..: neighbouring lanes write neighbouring bytes.  No byte outside the window is read, none outside the picture's bytes written.  No LDS.

// (the walk below is inlined into the kernel whatever its size: called as a function it would take the job through scratch memory)
#if defined(__HIP_DEVICE_COMPILE__)
#define LH264_SAMPLE_INLINE __attribute__ ((always_inline)) inline
#else
#define LH264_SAMPLE_INLINE inline
#endif

// binary32 -> the bits of binary16, round to nearest even, gradual underflow, overflow to infinity.  On the device the conversion
// instruction (the mode's rounding is nearest even and half denormals are kept: hipcc's defaults); on the host integer arithmetic
__host__ __device__ inline uint32_t half_bits (float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_bit_cast (uint16_t, (_Float16)v);
#else
  uint32_t x;
  __builtin_memcpy (&x, &v, 4);
  const uint32_t sign = x >> 16 & 0x8000u, a = x & 0x7fffffffu;
  if (a >= 0x7f800000u) return sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0u);
  if (a >= 0x38800000u) {                                          // 2^-14 and above: a normal half, or infinity
    uint32_t r = a - 0x38000000u;                                  // the exponent rebiased by 112; the carry of the rounding may enter it
    r = (r + 0xfffu + (r >> 13 & 1u)) >> 13;
    return sign | (r > 0x7c00u ? 0x7c00u : r);
  }
  const int s = 126 - (int) (a >> 23);                             // a subnormal half: m * 2^(e - 150) in units of 2^-24 is m >> s
  if (s > 24) return sign;                                         // below 2^-25: nearer to zero than to the smallest half
  const uint32_t m = (a & 0x7fffffu) | 0x800000u, rem = m & ((1u << s) - 1u), half = 1u << (s - 1);
  uint32_t q = m >> s;
  if (rem > half || (rem == half && (q & 1u))) q++;
  return sign | q;                                                 // (q == 0x400 is the smallest normal half: the same bits)
#endif
}
// binary32 -> the bits of bfloat16, round to nearest even (subnormals as they come: a bfloat16 is the upper half of a binary32)
__host__ __device__ inline uint32_t bfloat_bits (float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_bit_cast (uint16_t, (__bf16)v);
#else
  uint32_t x;
  __builtin_memcpy (&x, &v, 4);
  if ((x & 0x7fffffffu) > 0x7f800000u) return x >> 16 | 0x40u;
  return (x + 0x7fffu + (x >> 16 & 1u)) >> 16;
#endif
}
// element `lo`, and in the 16-bit types the element `hi` behind it, as one word of the destination
template <int T>
__host__ __device__ inline uint32_t sample_word (float lo, float hi) {
  if constexpr (T == (int)LH264_SAMPLE_F32) return __builtin_bit_cast (uint32_t, lo);
  else if constexpr (T == (int)LH264_SAMPLE_F16) return half_bits (lo) | half_bits (hi) << 16;
  else return bfloat_bits (lo) | bfloat_bits (hi) << 16;
}

// item p (pixels 8*p .. 8*p + 7) of row pair R of one job delivered as ow x oh in layout L, sample type T (LH264_SAMPLE_F32 / _F16 /
// _BF16), with the colour factors f, luma offset y0 and the caller's mul / add
template <int M, int L, int T>
__host__ __device__ LH264_SAMPLE_INLINE void piece_sample (uint8_t* dst, const ResizePlane& py, const ResizePlane& pu, const ResizePlane& pv, int ow, int oh,
                                              const int32_t* f, int y0, const float* mul, const float* add, int R, int p, const Placed& pc) {
  constexpr bool kPacked = L == (int)LH264_COLOUR_RGB24;
  constexpr int ES = T == (int)LH264_SAMPLE_F32 ? 4 : 2, NP = kPacked ? 1 : 3;      // an element's bytes; the planes of the destination
  constexpr int EQ = kPacked ? 6 : 2;                                                // the elements of a quad in one row of one plane
  constexpr int WQ = EQ * ES / 4, NW = 4 * WQ;                                       // ... and their words: 6, 3, 2, 1 and 24, 12, 8, 4
  const int X0 = 8 * p;
  if (X0 >= ow) return;
  const int nq = (ow - X0) >> 1 < 4 ? (ow - X0) >> 1 : 4;                            // the item's quads: 4, at a row's tail 1..3
  Span sy[2], sc;
  if constexpr (M == 4) { sy[0] = span_of ((uint32_t) (2 * R), py.h, py.oh); sy[1] = span_of ((uint32_t) (2 * R + 1), py.h, py.oh); sc = span_of ((uint32_t)R, pu.h, pu.oh); }
  else { sy[0] = sy[1] = sc = Span(); }
  // M = 5: the bar's three elements, once per item, and whether the pair's rows cross the rectangle (piece_rgb has the same lines)
  float barv[3] = {0.0f, 0.0f, 0.0f};
  bool rows_in = false;
  if constexpr (M == 5) {
    uint32_t bar[3];
    bar_rgb (pc.fill, f, y0, bar);
    for (int c = 0; c < 3; c++) barv[c] = __builtin_fmaf ((float)bar[c], mul[c], add[c]);
    rows_in = 2 * R >= pc.y && 2 * R < pc.y + (int)py.oh;
    if (rows_in) { sy[0] = span_of ((uint32_t) (2 * R - pc.y), py.h, py.oh); sy[1] = span_of ((uint32_t) (2 * R + 1 - pc.y), py.h, py.oh); sc = span_of ((uint32_t) (R - (pc.y >> 1)), pu.h, pu.oh); }
  }
  uint32_t W[2][NP][NW];                                                             // the item's words, per row and plane
  for (int rr = 0; rr < 2; rr++) for (int c = 0; c < NP; c++) for (int k = 0; k < NW; k++) W[rr][c][k] = 0;
  _Pragma ("unroll")
  for (int q = 0; q < 4; q++) {
    if (q >= nq) continue;
    uint32_t px[2][2][3];
    bool in_bar = false;
    if constexpr (M == 5) {
      const int X = X0 + 2 * q;
      in_bar = !(rows_in && X >= pc.x && X < pc.x + (int)py.ow);
      if (!in_bar) quad_rgb<4> (py, pu, pv, sy, sc, f, y0, X - pc.x, R - (pc.y >> 1), px);
      else for (int rr = 0; rr < 2; rr++) for (int i = 0; i < 2; i++) for (int c = 0; c < 3; c++) px[rr][i][c] = 0;
    } else quad_rgb<M> (py, pu, pv, sy, sc, f, y0, X0 + 2 * q, R, px);
    _Pragma ("unroll")
    for (int rr = 0; rr < 2; rr++) {
      float v[2][3];
      _Pragma ("unroll")
      for (int i = 0; i < 2; i++) {
        _Pragma ("unroll")
        for (int c = 0; c < 3; c++) v[i][c] = (M == 5 && in_bar) ? barv[c] : __builtin_fmaf ((float)px[rr][i][c], mul[c], add[c]);      // one fused multiply-add: the definition's
      }
      // the quad's elements of this row in memory order: R G B R G B in one plane, or the pixel pair in each of three
      if constexpr (kPacked) {
        const float e[6] = {v[0][0], v[0][1], v[0][2], v[1][0], v[1][1], v[1][2]};
        _Pragma ("unroll")
        for (int k = 0; k < WQ; k++) W[rr][0][WQ * q + k] = ES == 4 ? sample_word<T> (e[k], 0.0f) : sample_word<T> (e[(2 * k) % 6], e[(2 * k + 1) % 6]);
      } else {
        _Pragma ("unroll")
        for (int c = 0; c < 3; c++) {
          if constexpr (ES == 4) { W[rr][c][2 * q] = sample_word<T> (v[0][c], 0.0f); W[rr][c][2 * q + 1] = sample_word<T> (v[1][c], 0.0f); }
          else W[rr][c][q] = sample_word<T> (v[0][c], v[1][c]);
        }
      }
    }
  }
  const size_t row_bytes = (size_t) (kPacked ? 3 : 1) * ow * ES, plane_bytes = (size_t)ow * oh * ES;
  _Pragma ("unroll")
  for (int rr = 0; rr < 2; rr++) {
    _Pragma ("unroll")
    for (int c = 0; c < NP; c++) {
      uint8_t* row = dst + (size_t)c * plane_bytes + (size_t) (2 * R + rr) * row_bytes;
      uint8_t* o = row + (size_t)p * (NW * 4);
      if (nq == 4 && !((uintptr_t)row & 15u)) {
        _Pragma ("unroll")
        for (int k = 0; k < NW / 4; k++) { uint4 x; x.x = W[rr][c][4 * k]; x.y = W[rr][c][4 * k + 1]; x.z = W[rr][c][4 * k + 2]; x.w = W[rr][c][4 * k + 3]; * (uint4*) (o + 16 * k) = x; }
      } else {
        _Pragma ("unroll")
        for (int q = 0; q < 4; q++) {
          if (q >= nq) continue;
          _Pragma ("unroll")
          for (int k = 0; k < WQ; k++) * (uint32_t*) (o + 4 * (WQ * q + k)) = W[rr][c][WQ * q + k];
        }
      }
    }
  }
}

// band `band` (16 delivered luma rows) of one job delivered as ow x oh float RGB, worked on by item t of nt (the host steps it with t = 0, nt = 1)
template <int M, int L, int T>
__host__ __device__ LH264_SAMPLE_INLINE void pack_band_sample_as (const lh264_pack_job_t& j, int ow, int oh, int std_byte, const float* mul, const float* add, int band, int t, int nt, const lh264_pack_place_t* pl = nullptr) {
  const int w = j.crop_w, h = j.crop_h;
  const int R0 = band * (kBandRows / 2), R1 = R0 + kBandRows / 2 < (oh >> 1) ? R0 + kBandRows / 2 : (oh >> 1);
  if (R1 <= R0) return;
  const size_t co = (size_t) (j.crop_y >> 1) * j.stride_c + (j.crop_x >> 1);
  const int pw = M == 5 ? pl->w : ow, ph = M == 5 ? pl->h : oh;      // (pl: the job's place, read under M = 5 only)
  const Placed pc = M == 5 ? Placed {pl->x, pl->y, pl->fill} : Placed {0, 0, 0u};
  const ResizePlane py = {j.y + (size_t)j.crop_y * j.stride_y + j.crop_x, j.stride_y, (uint32_t)w, (uint32_t)h, (uint32_t)pw, (uint32_t)ph};
  const ResizePlane pu = {j.u + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pw >> 1), (uint32_t) (ph >> 1)};
  const ResizePlane pv = {j.v + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pw >> 1), (uint32_t) (ph >> 1)};
  int32_t f[5];
  for (int k = 0; k < 5; k++) f[k] = kColourFactors[std_byte & 3][k];
  const int y0 = (std_byte & 2) ? 0 : 16;
  const int pieces = (ow + 7) >> 3, items = (R1 - R0) * pieces;
  for (int it = t; it < items; it += nt) piece_sample<M, L, T> (j.dst, py, pu, pv, ow, oh, f, y0, mul, add, R0 + it / pieces, it % pieces, pc);
}
template <int L, int T>
__host__ __device__ LH264_SAMPLE_INLINE void pack_band_sample_sized (const lh264_pack_job_t& j, int ow, int oh, int m, int std_byte, const float* mul, const float* add, int band, int t, int nt) {
  if (m == 0) pack_band_sample_as<0, L, T> (j, ow, oh, std_byte, mul, add, band, t, nt);
  else if (m == 1) pack_band_sample_as<1, L, T> (j, ow, oh, std_byte, mul, add, band, t, nt);
  else if (m == 2) pack_band_sample_as<2, L, T> (j, ow, oh, std_byte, mul, add, band, t, nt);
  else if (m == 3) pack_band_sample_as<3, L, T> (j, ow, oh, std_byte, mul, add, band, t, nt);
  else pack_band_sample_as<4, L, T> (j, ow, oh, std_byte, mul, add, band, t, nt);
}
template <int L>
__host__ __device__ LH264_SAMPLE_INLINE void pack_band_sample_typed (const lh264_pack_job_t& j, int ow, int oh, int m, int type, int std_byte, const float* mul, const float* add, int band, int t, int nt) {
  if (type == (int)LH264_SAMPLE_F32) pack_band_sample_sized<L, (int)LH264_SAMPLE_F32> (j, ow, oh, m, std_byte, mul, add, band, t, nt);
  else if (type == (int)LH264_SAMPLE_F16) pack_band_sample_sized<L, (int)LH264_SAMPLE_F16> (j, ow, oh, m, std_byte, mul, add, band, t, nt);
  else if (type == (int)LH264_SAMPLE_BF16) pack_band_sample_sized<L, (int)LH264_SAMPLE_BF16> (j, ow, oh, m, std_byte, mul, add, band, t, nt);
}
// ... of a job whose sizing is its `reserved` scale (out_w == 0) or the given size; layout, standard byte and sample as given.  Anything
// that is not defined, and a destination that is no multiple of 4: nothing is done
__host__ __device__ LH264_SAMPLE_INLINE void pack_band_sample (const lh264_pack_job_t& j, int out_w, int out_h, int layout, int std_byte, const lh264_decode_sample_t& sm, int band, int t, int nt) {
  if (j.crop_w <= 0 || j.crop_h <= 0 || j.reserved < 0 || j.reserved > 3 || (out_w && j.reserved) || ((uintptr_t)j.dst & 3u)) return;
  int ow, oh;
  delivered_size (j.crop_w, j.crop_h, j.reserved, out_w, out_h, &ow, &oh);
  const int m = out_w ? 4 : j.reserved;
  if (layout == (int)LH264_COLOUR_RGB24) pack_band_sample_typed<(int)LH264_COLOUR_RGB24> (j, ow, oh, m, (int)sm.type, std_byte, sm.mul, sm.add, band, t, nt);
  else if (layout == (int)LH264_COLOUR_RGBP) pack_band_sample_typed<(int)LH264_COLOUR_RGBP> (j, ow, oh, m, (int)sm.type, std_byte, sm.mul, sm.add, band, t, nt);
}
// ... of a job placed by pl in an out_w x out_h picture (LH264_FIT_CONTAIN)
template <int L>
__host__ __device__ LH264_SAMPLE_INLINE void pack_band_sample_placed_in (const lh264_pack_job_t& j, const lh264_pack_place_t& pl, int ow, int oh, int type, int std_byte, const float* mul, const float* add, int band, int t, int nt) {
  if (type == (int)LH264_SAMPLE_F32) pack_band_sample_as<5, L, (int)LH264_SAMPLE_F32> (j, ow, oh, std_byte, mul, add, band, t, nt, &pl);
  else if (type == (int)LH264_SAMPLE_F16) pack_band_sample_as<5, L, (int)LH264_SAMPLE_F16> (j, ow, oh, std_byte, mul, add, band, t, nt, &pl);
  else if (type == (int)LH264_SAMPLE_BF16) pack_band_sample_as<5, L, (int)LH264_SAMPLE_BF16> (j, ow, oh, std_byte, mul, add, band, t, nt, &pl);
}
__host__ __device__ LH264_SAMPLE_INLINE void pack_band_sample_placed (const lh264_pack_job_t& j, const lh264_pack_place_t& pl, int out_w, int out_h, int layout, int std_byte, const lh264_decode_sample_t& sm, int band, int t, int nt) {
  if (j.crop_w <= 0 || j.crop_h <= 0 || j.reserved || ((uintptr_t)j.dst & 3u)) return;
  if (layout == (int)LH264_COLOUR_RGB24) pack_band_sample_placed_in<(int)LH264_COLOUR_RGB24> (j, pl, out_w, out_h, (int)sm.type, std_byte, sm.mul, sm.add, band, t, nt);
  else if (layout == (int)LH264_COLOUR_RGBP) pack_band_sample_placed_in<(int)LH264_COLOUR_RGBP> (j, pl, out_w, out_h, (int)sm.type, std_byte, sm.mul, sm.add, band, t, nt);
}

// ---- the motion fields: lh264_decode_batch_ex4 (the definition: include/lh264.h at that call) ---------------------------------------
// A gather / transpose from the 128-byte records to dense planes; nothing of a reconstructed picture is read.  The unit of work is a
// CHUNK: up to kMotionChunkMbs neighbouring macroblocks of one macroblock row.  Its records are fetched once (on the device: 16-byte loads
// into LDS, a record 33 words apart, so that the lanes of a wave - one macroblock each - read one field of 64 records from 64 banks)
// and every field is read from there as 32-bit words.  An item of the motion block is the four cells of one cell row of one macroblock
// in one plane: one aligned 8-byte store (a block begins at a multiple of 8 bytes and a cell row of a macroblock is 8 bytes), item k
// and k + 1 are neighbouring macroblocks: the lanes of a wave write a plane row's bytes one behind the other.  The reference lookups of
// plane 2 are two per item, one per quadrant the row crosses.  An item of the macroblock block is a PIECE of one plane's row: 8 bytes of
// the destination counted from the aligned address at or below the chunk's first byte (a plane row begins wherever the row before
// ended); a whole piece is one aligned 8-byte store, heads and tails go byte by byte and touch nothing outside the chunk's bytes.
constexpr int kMotionChunkMbs = LH264_MOTION_CHUNK_MBS;
constexpr int kMotionRecStride = 33;       // words between two records in LDS

// [0] of the macroblock block
__host__ __device__ inline uint32_t motion_kind (uint32_t mb_type) {
  if (mb_type & LH264_MB_I4x4) return 1;
  if (mb_type & LH264_MB_I8x8) return 2;
  if (mb_type & LH264_MB_I16x16) return 3;
  if (mb_type & LH264_MB_IPCM) return 4;
  if (mb_type & LH264_MB_SKIP) return 5;
  if (mb_type & LH264_MB_P16x16) return 6;
  if (mb_type & LH264_MB_P16x8) return 7;
  if (mb_type & LH264_MB_P8x16) return 8;
  if (mb_type & LH264_MB_P8x8) return 9;
  if (mb_type & LH264_MB_P8x8REF0) return 10;
  return 0;
}
// `back` of quadrant q of the record whose words are rec
__host__ __device__ inline uint32_t motion_back (const uint32_t* rec, int q, const lh264_slice_t* slices, int n_slices, const int16_t* back) {
  const int r = (int8_t) (rec[8] >> (8 * q));
  const int sid = (int) (rec[6] >> 16);
  if (r < 0 || r >= LH264_MAX_REFS || sid >= n_slices) return 0xffffu;
  const int slot = slices[sid].ref_slot[r];
  if (slot < 0 || slot >= LH264_MAX_REFS) return 0xffffu;
  return (uint32_t) (uint16_t)back[slot];
}
// cells 4 * mbx .. 4 * mbx + 3 of cell row y (0..3) of the macroblock in plane p: four int16
__host__ __device__ inline uint2 motion_cells (const uint32_t* rec, int p, int y, const lh264_slice_t* slices, int n_slices, const int16_t* back) {
  const uint32_t type = rec[0] & 0xffffu;
  uint2 o = {0u, 0u};
  if (motion_kind (type) < 5) return o;
  if (p == 2) {
    const uint32_t b0 = motion_back (rec, (y >> 1) * 2, slices, n_slices, back), b1 = motion_back (rec, (y >> 1) * 2 + 1, slices, n_slices, back);
    o.x = b0 | b0 << 16; o.y = b1 | b1 << 16;
    return o;
  }
  const uint32_t* mv = rec + 15 + ((type & LH264_MB_CONCEAL) ? 0 : 4 * y);       // (mv[b] is word 15 + b: dx below dy)
  const bool one = (type & LH264_MB_CONCEAL) != 0;
  const int sh = 16 * p;
  const uint32_t c0 = mv[0] >> sh & 0xffffu, c1 = (one ? mv[0] : mv[1]) >> sh & 0xffffu, c2 = (one ? mv[0] : mv[2]) >> sh & 0xffffu, c3 = (one ? mv[0] : mv[3]) >> sh & 0xffffu;
  o.x = c0 | c1 << 16; o.y = c2 | c3 << 16;
  return o;
}
// the macroblock's byte in plane pl of the macroblock block
__host__ __device__ inline uint32_t motion_info (const uint32_t* rec, int pl) {
  const uint32_t type = rec[0] & 0xffffu;
  if (pl == 0) return motion_kind (type);
  if (pl == 1) return rec[0] >> 24;
  if (pl == 2) return rec[0] >> 16 & 0xffu;
  if (pl == 3) return (rec[1] >> 16 & LH264_MBF_T8x8) | ((type & LH264_MB_CONCEAL) ? 2u : 0u);
  const uint32_t k = motion_kind (type);
  return k == 9 || k == 10 ? rec[7] >> (8 * (pl - 4)) & 0xffu : 0u;
}
// macroblocks c0 .. c0 + n - 1 of macroblock row `row` of one job, worked on by item t of nt (the lanes of a workgroup; the host steps
// it with t = 0, nt = 1).  rec_at (m): the 32 words of the chunk's record m; back: the job's table
template <class RecAt>
__host__ __device__ inline void motion_chunk (const lh264_motion_job_t& j, const int16_t* back, int row, int c0, int n, const RecAt& rec_at, int t, int nt) {
  const size_t cw = 4 * (size_t)j.mb_w, plane = cw * 4 * (size_t)j.mb_h;
  for (int it = t; it < 12 * n; it += nt) {
    const int m = it % n, py = it / n, p = py >> 2, y = py & 3;
    const uint2 v = motion_cells (rec_at (m), p, y, j.slices, j.n_slices, back);
    * (uint2*) (j.motion + (size_t)p * plane + (size_t) (4 * row + y) * cw + 4 * (size_t) (c0 + m)) = v;
  }
  const size_t ip = (size_t)j.mb_w * j.mb_h;
  const int pieces = (n + 14) >> 3;
  for (int it = t; it < 8 * pieces; it += nt) {
    const int pl = it / pieces, pc = it % pieces;
    uint8_t* d = j.info + (size_t)pl * ip + (size_t)row * j.mb_w + c0;
    int a = pc * 8 - (int) ((uintptr_t)d & 7u), b = a + 8;
    if (a >= 0 && b <= n) {
      uint2 o = {0u, 0u};
      for (int k = 0; k < 4; k++) { o.x |= motion_info (rec_at (a + k), pl) << (8 * k); o.y |= motion_info (rec_at (a + 4 + k), pl) << (8 * k); }
      * (uint2*) (d + a) = o;
      continue;
    }
    if (a < 0) a = 0;
    if (b > n) b = n;
    for (int k = a; k < b; k++) d[k] = (uint8_t)motion_info (rec_at (k), pl);
  }
}
// what the entry points accept as a job: sizes the front end can deliver, destinations at multiples of 8 bytes
inline bool motion_job_ok (const lh264_motion_job_t& j) {
  return j.mbs && j.motion && j.info && (j.slices || !j.n_slices) && j.mb_w >= 1 && j.mb_w <= 1024 && j.mb_h >= 1 && j.mb_h <= 1024 && j.n_slices >= 0 && j.n_slices <= 65535 &&
         j.reserved == 0 && !((uintptr_t)j.motion & 7u) && !((uintptr_t)j.info & 7u);
}
inline int motion_chunks (int mb_w) { return (mb_w + kMotionChunkMbs - 1) / kMotionChunkMbs; }

}  // namespace lh264pack

// one workgroup per (picture, chunk of a macroblock row): the chunk's records go to LDS once, then every lane takes items of both blocks
__global__ void __launch_bounds__ (256) decode_pack_motion_kernel (const lh264_motion_job_t* __restrict__ jobs) {
  __shared__ uint32_t s_rec[lh264pack::kMotionChunkMbs * lh264pack::kMotionRecStride];
  __shared__ int16_t s_back[LH264_MAX_REFS];
  const lh264_motion_job_t j = jobs[blockIdx.x];
  const int chunks = (j.mb_w + lh264pack::kMotionChunkMbs - 1) / lh264pack::kMotionChunkMbs;
  if ((int)blockIdx.y >= j.mb_h * chunks) return;
  const int row = (int)blockIdx.y / chunks, c0 = ((int)blockIdx.y % chunks) * lh264pack::kMotionChunkMbs;
  const int n = j.mb_w - c0 < lh264pack::kMotionChunkMbs ? j.mb_w - c0 : lh264pack::kMotionChunkMbs;
  const int t = (int)threadIdx.x;
  if (t < LH264_MAX_REFS) s_back[t] = jobs[blockIdx.x].back[t];
  const uint4* src = (const uint4*) (j.mbs + (size_t)row * j.mb_w + c0);      // (records are 128 bytes and begin at a multiple of 16)
  for (int q = t; q < 8 * n; q += 256) {
    const uint4 v = src[q];
    uint32_t* d = s_rec + (q >> 3) * lh264pack::kMotionRecStride + (q & 7) * 4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();
  lh264pack::motion_chunk (j, s_back, row, c0, n, [&] (int m) { return (const uint32_t*)s_rec + m * lh264pack::kMotionRecStride; }, t, 256);
}

// one workgroup per (picture, band)
__global__ void __launch_bounds__ (256) decode_pack_kernel (const lh264_pack_job_t* __restrict__ jobs) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  if ((int)blockIdx.y * lh264pack::kBandRows >= j.crop_h) return;
  lh264pack::pack_band (j, (int)blockIdx.y, (int)threadIdx.x, 256);
}
// one workgroup per (picture, band of 16 delivered luma rows): the jobs of a launch share one scale_log2 in 1..3
__global__ void __launch_bounds__ (256) decode_pack_scaled_kernel (const lh264_pack_job_t* __restrict__ jobs) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  if (j.reserved < 1 || j.reserved > 3) return;
  int ow, oh;
  lh264pack::scaled_size (j.crop_w, j.crop_h, j.reserved, &ow, &oh);
  if ((int)blockIdx.y * lh264pack::kBandRows >= oh) return;
  lh264pack::pack_band_scaled (j, (int)blockIdx.y, (int)threadIdx.x, 256);
}
// one workgroup per (picture, band of 16 delivered luma rows): every job of the launch is delivered as out_w x out_h (a withheld
// picture's job has no window and nothing is done for it)
__global__ void __launch_bounds__ (256) decode_pack_resized_kernel (const lh264_pack_job_t* __restrict__ jobs, int out_w, int out_h) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  if (j.crop_w <= 0 || j.crop_h <= 0 || (int)blockIdx.y * lh264pack::kBandRows >= out_h) return;
  lh264pack::pack_band_resized (j, out_w, out_h, (int)blockIdx.y, (int)threadIdx.x, 256);
}

// one workgroup per (picture, band of 16 delivered luma rows): the jobs as RGB in one layout, job k by the standard byte std[k]; out_w,
// out_h the given size or 0, 0 (then each job by its `reserved` scale).  A withheld picture's job has no window and nothing is done for it
__global__ void __launch_bounds__ (256) decode_pack_rgb_kernel (const lh264_pack_job_t* __restrict__ jobs, const uint8_t* __restrict__ std, int out_w, int out_h, int layout) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  lh264pack::pack_band_rgb (j, out_w, out_h, layout, (int)std[blockIdx.x], (int)blockIdx.y, (int)threadIdx.x, 256);
}

// one workgroup per (picture, band of 16 delivered luma rows): the jobs as float RGB - decode_pack_rgb_kernel's arguments and the sample
// struct (a float type, six finite factors).  Every job's dst is a multiple of 4
__global__ void __launch_bounds__ (256) decode_pack_sample_kernel (const lh264_pack_job_t* __restrict__ jobs, const uint8_t* __restrict__ std, int out_w, int out_h, int layout, lh264_decode_sample_t sample) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  lh264pack::pack_band_sample (j, out_w, out_h, layout, (int)std[blockIdx.x], sample, (int)blockIdx.y, (int)threadIdx.x, 256);
}

// LH264_FIT_CONTAIN: the three kernels above with every job's window placed by places[job] in the out_w x out_h picture and the bars
// filled (a withheld picture's job has no window and nothing is done for it).  Kernels of their own: the launches above stay as they were
__global__ void __launch_bounds__ (256) decode_pack_placed_kernel (const lh264_pack_job_t* __restrict__ jobs, const lh264_pack_place_t* __restrict__ places, int out_w, int out_h) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  if (j.crop_w <= 0 || j.crop_h <= 0 || (int)blockIdx.y * lh264pack::kBandRows >= out_h) return;
  const lh264_pack_place_t pl = places[blockIdx.x];
  lh264pack::pack_band_placed (j, pl, out_w, out_h, (int)blockIdx.y, (int)threadIdx.x, 256);
}
__global__ void __launch_bounds__ (256) decode_pack_rgb_placed_kernel (const lh264_pack_job_t* __restrict__ jobs, const lh264_pack_place_t* __restrict__ places, const uint8_t* __restrict__ std, int out_w, int out_h, int layout) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  const lh264_pack_place_t pl = places[blockIdx.x];
  lh264pack::pack_band_rgb_placed (j, pl, out_w, out_h, layout, (int)std[blockIdx.x], (int)blockIdx.y, (int)threadIdx.x, 256);
}
__global__ void __launch_bounds__ (256) decode_pack_sample_placed_kernel (const lh264_pack_job_t* __restrict__ jobs, const lh264_pack_place_t* __restrict__ places, const uint8_t* __restrict__ std, int out_w, int out_h, int layout, lh264_decode_sample_t sample) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  const lh264_pack_place_t pl = places[blockIdx.x];
  lh264pack::pack_band_sample_placed (j, pl, out_w, out_h, layout, (int)std[blockIdx.x], sample, (int)blockIdx.y, (int)threadIdx.x, 256);
}

// ---- the digests: SHA-1 of packed pictures where they lie ---------------------------------------------------------------------------
// One lane per span job, 64 jobs per wave (a message is serial; the width comes from the batch).  The host orders a launch's jobs by
// descending length, so the lanes of a wave end near one another.  No LDS, no wave waits for another; every bound is the job's.
__global__ void __launch_bounds__ (64) sha1_spans_kernel (const lh264_sha1_job_t* __restrict__ jobs, int n) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n) return;
  lh264sha1::run_job (jobs[i]);
}

struct lh264_decoded {
  int status = LH264_OK;
  std::string error;
  std::vector<lh264_decoded_pic_t> pics;
  std::vector<int32_t> concealed;               // per picture: its concealed macroblocks
  std::vector<int32_t> source_wh;               // per picture: width, height of its cropped window before scaling
  std::vector<int32_t> view;                    // per picture: its source rectangle in the window, its destination rectangle in the delivered picture (x, y, w, h each)
  int parse_path = LH264_PARSE_PATH_HOST;
  long device_cabac_slices = 0;                 // ... of them CABAC slices (slice_parse_cabac_kernel)
  long device_slices = 0;                       // slices of the stream that slice_parse_kernel parsed and the host kept
  long parsed_slices = 0;                       // distinct slices whose slice data was parsed, on either route
  std::vector<int32_t> index;                   // per delivered picture: its number among the stream's pictures in decode order
  std::vector<uint8_t> colour;                  // lh264_decode_batch_ex with colour: per delivered picture the standard byte that was applied
  int sample_type = (int)LH264_SAMPLE_U8;       // lh264_decode_batch_ex2: the LH264_SAMPLE_* of the call
  std::vector<uint8_t> bytes;                   // host mode
  uint8_t* dev = nullptr; size_t dev_len = 0, dev_cap = 0; int device = 0;      // LH264_DECODE_DEVICE_OUT
  uint32_t sha = 0;                             // the LH264_DECODE_SHA1_* bits of the call
  std::vector<uint8_t> pic_sha;                 // 20 bytes per delivered picture
  lh264_sha1_state_t stream_state;              // the stream's message behind the last round delivered
  uint8_t stream_sha[20];
  // lh264_decode_batch_ex4 with fields: per delivered picture its geometry and offsets, the stream's motion blocks and macroblock
  // blocks in host memory, or in device memory (LH264_DECODE_DEVICE_OUT)
  uint32_t fields = 0;
  std::vector<lh264_decoded_motion_t> motion_geo;
  std::vector<uint8_t> mot, mbi;
  uint8_t* mot_dev = nullptr; size_t mot_len = 0, mot_cap = 0;
  uint8_t* mbi_dev = nullptr; size_t mbi_len = 0, mbi_cap = 0;
  lh264_decoded() { lh264sha1::init (&stream_state); memset (stream_sha, 0, 20); }
  ~lh264_decoded() {
    if (!dev && !mot_dev && !mbi_dev) return;
    int cur = 0;
    hipGetDevice (&cur);
    if (cur != device) hipSetDevice (device);
    if (dev) hipFree (dev);
    if (mot_dev) hipFree (mot_dev);
    if (mbi_dev) hipFree (mbi_dev);
    if (cur != device) hipSetDevice (cur);
  }
};

namespace {

using lh264host::FrameOut;
using lh264host::Parser;

using lh264host::DevBuf;
using lh264host::PinBuf;
using lh264host::now_s;
bool trace_on() { static const bool t = lh264host::trace_on ("LH264_TRACE_DECODE"); return t; }

// padded pictures, handed out one by one and taken back when a stream is through; allocated in slabs of one picture size
struct PicCache {
  std::map<size_t, std::vector<uint8_t*>> free_;
  std::vector<void*> slabs;
  size_t bytes = 0;
  ~PicCache() { for (void* s : slabs) hipFree (s); }
  uint8_t* get (size_t pic_bytes, hipStream_t st) {
    std::vector<uint8_t*>& v = free_[pic_bytes];
    if (v.empty()) {
      const size_t n = std::min<size_t> (64, std::max<size_t> (1, ((size_t)32 << 20) / pic_bytes));
      void* s = nullptr;
      if (hipMalloc (&s, n * pic_bytes) != hipSuccess) return nullptr;
      slabs.push_back (s); bytes += n * pic_bytes;
      for (size_t k = n; k-- > 0; ) v.push_back ((uint8_t*)s + k * pic_bytes);
    }
    uint8_t* p = v.back(); v.pop_back();
    return p;
  }
  void put (size_t pic_bytes, uint8_t* p) { free_[pic_bytes].push_back (p); }
  // one picture per size that nothing ever writes: every sample 128, padding included.  It stands in for a reference a picture names
  // no picture for (see where the job tables are written)
  std::map<size_t, uint8_t*> grey_;
  const uint8_t* grey (size_t pic_bytes, hipStream_t st) {
    auto it = grey_.find (pic_bytes);
    if (it != grey_.end()) return it->second;
    uint8_t* p = get (pic_bytes, st);
    if (!p) return nullptr;
    if (hipMemsetAsync (p, 128, pic_bytes, st) != hipSuccess) { put (pic_bytes, p); return nullptr; }
    grey_[pic_bytes] = p;
    return p;
  }
};

// two of everything the host writes or reads while the device works on the round before
struct Arena {
  DevBuf d_mbs, d_coef, d_sparse, d_sl, d_jobs, d_first, d_pack, d_out[2];
  PinBuf h_mbs[2], h_sparse[2], h_sl[2], h_jobs[2], h_first[2], h_pack[2], h_out[2];
  DevBuf d_std; PinBuf h_std[2];      // lh264_decode_batch_ex with colour: the standard byte of every pack job, beside d_pack
  DevBuf d_place; PinBuf h_place[2];  // lh264_decode_batch_ex3 with LH264_FIT_CONTAIN: the place of every pack job, beside d_pack
  // lh264_decode_batch_ex4 with fields: the round's motion jobs, its motion blocks and macroblock blocks (downloaded like d_out)
  DevBuf d_mjobs, d_mot[2], d_mbi[2]; PinBuf h_mjobs[2], h_mot[2], h_mbi[2];
  hipEvent_t e_mot[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};      // around the round's decode_pack_motion_kernel launch (created on first use)
  // digests: the span jobs, a round's results (20 bytes per picture, then a copy of every chain's stream record), the records of the
  // picture messages (scratch), and one record per stream of the batch that lives as long as the call
  DevBuf d_sjobs, d_dig, d_rec, d_state;
  PinBuf h_sjobs[2], h_dig[2];
  // parse = LH264_PARSE_DEVICE: the round's slice payloads (+ scaling lists, + lines of wide pictures), tasks and results; the records and
  // coefficient planes slice_parse_kernel writes and recon_chain_kernel reads
  DevBuf d_pbytes, d_ptasks, d_pres, d_pmbs, d_pcoef;
  PinBuf h_pbytes, h_ptasks, h_pres;
  PicCache pics;
  hipStream_t s_run = nullptr, s_down = nullptr;
  hipEvent_t e_run[2] = {nullptr, nullptr}, e_down[2] = {nullptr, nullptr};
  bool ready = false;
  bool init() {
    if (ready) return true;
    bool ok = hipStreamCreateWithFlags (&s_run, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags (&s_down, hipStreamNonBlocking) == hipSuccess;
    for (int b = 0; b < 2 && ok; b++) ok = hipEventCreateWithFlags (&e_run[b], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags (&e_down[b], hipEventDisableTiming) == hipSuccess;
    ready = ok;
    return ok;
  }
  ~Arena() {
    for (int b = 0; b < 2; b++) { if (e_run[b]) hipEventDestroy (e_run[b]); if (e_down[b]) hipEventDestroy (e_down[b]); for (int k = 0; k < 2; k++) if (e_mot[b][k]) hipEventDestroy (e_mot[b][k]); }
    if (s_run) hipStreamDestroy (s_run);
    if (s_down) hipStreamDestroy (s_down);
  }
  size_t device_bytes() const {
    size_t n = pics.bytes + d_out[0].cap + d_out[1].cap + d_mjobs.cap + d_mot[0].cap + d_mot[1].cap + d_mbi[0].cap + d_mbi[1].cap;
    for (const DevBuf* b : {&d_mbs, &d_coef, &d_sparse, &d_sl, &d_jobs, &d_first, &d_pack, &d_sjobs, &d_dig, &d_rec, &d_state, &d_pbytes, &d_ptasks, &d_pres, &d_pmbs, &d_pcoef, &d_std, &d_place}) n += b->cap;
    return n;
  }
  size_t pinned_bytes() const {
    size_t n = h_pbytes.cap + h_ptasks.cap + h_pres.cap;
    for (int b = 0; b < 2; b++) n += h_mbs[b].cap + h_sparse[b].cap + h_sl[b].cap + h_jobs[b].cap + h_first[b].cap + h_pack[b].cap + h_out[b].cap + h_sjobs[b].cap + h_dig[b].cap + h_std[b].cap + h_place[b].cap + h_mjobs[b].cap + h_mot[b].cap + h_mbi[b].cap;
    return n;
  }
};

struct Geo {
  int mb_w = 0, mb_h = 0, stride_y = 0, stride_c = 0;
  size_t off[3] = {0, 0, 0}, bytes = 0;
};
struct Slot { uint8_t* base; int pic_id; };       // pic_id < 0: free

// a stream of the batch while it is being decoded
struct DStream {
  int i = 0;
  std::unique_ptr<Parser> parser;
  std::deque<std::unique_ptr<FrameOut>> pending;     // parsed, not yet in a round
  long next_picture = 0;                             // the stream's pictures in rounds so far
  long seen = 0;                                     // the pictures the parser has handed over so far (opts->pick: selected or not)
  long delivered = 0;                                // ... those of them that are handed out (a frozen picture is reconstructed only)
  uint64_t out_off = 0;                              // ... and their packed bytes
  uint64_t mot_off = 0, mbi_off = 0;                 // ... and with fields their motion blocks' and macroblock blocks' bytes
  size_t pic_mbs = 0;                                // macroblocks of the stream's last picture (0: none seen yet)
  Geo geo;
  const uint8_t* grey = nullptr;                     // the arena's 128 picture of this geometry
  std::vector<Slot> pool;
  std::map<int, long> held;                          // fields: id -> index of the pictures the pool holds (kept where no pool is used)
  // set by select(): the stream ends behind the pictures selected
  bool ending = false; int end_code = LH264_OK; std::string end_text;
  bool sha_started = false;                          // the stream's digest record on the device holds its message so far
  bool stopped = false;                              // the sink refused, or the device stage failed: nothing more is delivered
  std::vector<std::unique_ptr<FrameOut>> sel;        // the pictures of the round in preparation
  // parse = LH264_PARSE_DEVICE: the stream's CAVLC slices go to slice_parse_kernel (until a CABAC picture or a fallback ends that), and
  // where in the parse arena the records / the slice table of the pictures parsed there in this round lie
  bool dev_route = false;
  struct DevAt { size_t mb; };
  std::map<const FrameOut*, DevAt> dev_at;
};

// one chain of a round that is on the device: what its delivery needs
struct RoundChain {
  DStream* s = nullptr;
  int first_picture = 0;
  std::vector<lh264_decoded_pic_t> pics;
  std::vector<int32_t> concealed, source_wh, index, view;
  std::vector<uint8_t> colour;                      // lh264_decode_batch_ex with colour: per delivered picture its standard byte
  size_t at = 0, bytes = 0;                          // in the round's output buffer
  size_t n_out = 0, dig0 = 0;                        // pictures the chain delivers; the first one's place among the round's digests
  std::vector<lh264_decoded_motion_t> motion_geo;    // fields: per delivered picture; the chain's blocks in the round's two buffers
  size_t mot_at = 0, mot_bytes = 0, mbi_at = 0, mbi_bytes = 0, mjob0 = 0;
};
struct Round { std::vector<RoundChain> chains; size_t out_bytes = 0, dig_states_at = 0, mot_bytes = 0, mbi_bytes = 0; bool live = false, timed = false; };

// opts->pick: is the picture one of those the call decodes?  (slice_type: 0 P, 2 I)
bool picture_selected (const FrameOut& f, uint32_t pick) {
  if (pick == LH264_PICK_ALL) return true;
  if (f.slices.empty()) return false;
  if (pick == LH264_PICK_IDR) return f.idr;
  for (const lh264_slice_t& sl : f.slices) if (sl.slice_type != 2) return false;
  return true;
}

std::string refuse_picture (const FrameOut& f) {
  const size_t n = (size_t)f.mb_w * f.mb_h;
  if (f.covered.size() != n || f.mbs.size() != n) return "an incomplete picture";
  for (size_t k = 0; k < n; k++) if (!f.covered[k] && !(f.mbs[k].mb_type & LH264_MB_CONCEAL)) return "macroblocks no slice covers (the reference conceals them, which is not modelled)";
  if (f.slices.empty() || f.slice_syn.size() != f.slices.size()) return "an incomplete slice";
  if (f.crop_w <= 0 || f.crop_h <= 0 || (f.crop_w & 1) || (f.crop_h & 1) || f.crop_x < 0 || f.crop_y < 0 || (f.crop_x & 1) || (f.crop_y & 1) ||
      f.crop_x + f.crop_w > f.mb_w * 16 || f.crop_y + f.crop_h > f.mb_h * 16) return "a crop window outside the picture";
  return "";
}

// the standard byte of a picture under the call's matrix and range (see LH264_COLOUR_FACTORS); 0xff: the matrix is left to the stream
// and its matrix_coefficients has no conversion here
uint8_t picture_standard (const FrameOut& f, uint32_t matrix, uint32_t range) {
  int m;
  if (matrix != LH264_MATRIX_AUTO) m = matrix == LH264_MATRIX_BT709;
  else if (f.matrix_coefficients == 1) m = 1;
  else if (f.matrix_coefficients == 2 || f.matrix_coefficients == 5 || f.matrix_coefficients == 6) m = 0;
  else return 0xff;
  const int full = range != LH264_RANGE_AUTO ? range == LH264_RANGE_FULL : f.full_range;
  return (uint8_t) (m | full << 1);
}

// ---- views (the definition: include/lh264.h at lh264_decode_batch_ex3) ------------------------------------------------------------
// a caller's crop that is one: even, not negative, at least 2 x 2 - or none (w = h = 0)
bool crop_ok (const lh264_rect_t& c) {
  return c.x >= 0 && c.y >= 0 && c.w >= 0 && c.h >= 0 && !((c.x | c.y | c.w | c.h) & 1) && (c.w == 0) == (c.h == 0);
}
bool crop_fits (const lh264_rect_t& c, int w, int h) { return c.x <= w - c.w && c.y <= h - c.h; }
// the fit of a w x h window (after the caller's crop) to OW x OH: the source inside the window, the destination inside the output
void fit_rects (int w, int h, uint32_t fit, int OW, int OH, lh264_rect_t* src, lh264_rect_t* dst) {
  *src = {0, 0, w, h}; *dst = {0, 0, OW, OH};
  const int64_t a = (int64_t)w * OH, b = (int64_t)h * OW;
  if (fit == LH264_FIT_COVER && a != b) {
    if (a > b) src->w = std::max (2, 2 * (int) ((b + OH) / (2 * (int64_t)OH)));
    else src->h = std::max (2, 2 * (int) ((a + OW) / (2 * (int64_t)OW)));
    src->x = 2 * ((w - src->w) / 4); src->y = 2 * ((h - src->h) / 4);
  } else if (fit == LH264_FIT_CONTAIN && a != b) {
    if (a > b) dst->h = std::max (2, 2 * (int) ((b + w) / (2 * (int64_t)w)));
    else dst->w = std::max (2, 2 * (int) ((a + h) / (2 * (int64_t)h)));
    dst->x = 2 * ((OW - dst->w) / 4); dst->y = 2 * ((OH - dst->h) / 4);
  }
}
// the view of a picture whose window is w x h under a crop that fits (w = 0: none), a fit and a size (0, 0: the window at scale s):
// the source in window coordinates, the destination in the delivered ow x oh picture
void view_of (int w, int h, const lh264_rect_t& crop, uint32_t fit, int s, int out_w, int out_h, lh264_rect_t* src, lh264_rect_t* dst, int* ow, int* oh) {
  const lh264_rect_t c = crop.w ? crop : lh264_rect_t {0, 0, w, h};
  if (out_w) { fit_rects (c.w, c.h, fit, out_w, out_h, src, dst); *ow = out_w; *oh = out_h; }
  else { *src = {0, 0, c.w, c.h}; lh264pack::scaled_size (c.w, c.h, s, ow, oh); *dst = {0, 0, *ow, *oh}; }
  src->x += c.x; src->y += c.y;
}

lh264host::PerDevice<Arena> g_arena;     // one decode call at a time per device
double g_timing[6] = {0, 0, 0, 0, 0, 0};
double g_motion_ms = 0; unsigned long long g_motion_bytes = 0;      // lh264_decode_last_motion
long long g_chains[3] = {0, 0, 0};      // rounds, chains and jobs of the last call's lh264_recon_chains launches
double g_parse_timing[2] = {0, 0};      // of g_timing[1]: the device parse stage (tasks, upload, slice_parse_kernel, results), and its slices

const uint32_t kDefaultRoundPictures = 8;
const uint64_t kDefaultGroupMbs = 1000000;

}  // namespace

extern "C" {

int lh264_debug_pack_cpu (const lh264_pack_job_t* jobs, int n) {
  if (!jobs || n < 0) return LH264_E_ARG;
  for (int k = 0; k < n; k++) {
    const lh264_pack_job_t& j = jobs[k];
    if (!j.y || !j.u || !j.v || !j.dst || j.crop_w <= 0 || j.crop_h <= 0 || ((j.crop_w | j.crop_h | j.crop_x | j.crop_y) & 1) || j.crop_x < 0 || j.crop_y < 0 ||
        (j.format != LH264_FMT_I420 && j.format != LH264_FMT_NV12) || j.reserved < 0 || j.reserved > 3) return LH264_E_ARG;
    if (!j.reserved) { for (int band = 0; band * lh264pack::kBandRows < j.crop_h; band++) lh264pack::pack_band (j, band, 0, 1); continue; }
    int ow, oh;
    lh264pack::scaled_size (j.crop_w, j.crop_h, j.reserved, &ow, &oh);
    for (int band = 0; band * lh264pack::kBandRows < oh; band++) lh264pack::pack_band_scaled (j, band, 0, 1);
  }
  return LH264_OK;
}

int lh264_debug_pack_dev (const lh264_pack_job_t* jobs, int n) {
  if (!jobs || n < 0) return LH264_E_ARG;
  int max_bands = 0;
  for (int k = 0; k < n; k++) {
    const lh264_pack_job_t& j = jobs[k];
    if (!j.y || !j.u || !j.v || !j.dst || j.crop_w <= 0 || j.crop_h <= 0 || ((j.crop_w | j.crop_h | j.crop_x | j.crop_y) & 1) || j.crop_x < 0 || j.crop_y < 0 ||
        (j.format != LH264_FMT_I420 && j.format != LH264_FMT_NV12) || j.reserved < 0 || j.reserved > 3 || j.reserved != jobs[0].reserved) return LH264_E_ARG;
    int ow, oh;
    lh264pack::scaled_size (j.crop_w, j.crop_h, j.reserved, &ow, &oh);
    max_bands = std::max (max_bands, (oh + lh264pack::kBandRows - 1) / lh264pack::kBandRows);
  }
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  if (!n) return LH264_OK;
  lh264_pack_job_t* d_jobs = nullptr;
  bool ok = hipMalloc ((void**)&d_jobs, (size_t)n * sizeof (lh264_pack_job_t)) == hipSuccess && hipMemcpy (d_jobs, jobs, (size_t)n * sizeof (lh264_pack_job_t), hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    if (jobs[0].reserved) hipLaunchKernelGGL (decode_pack_scaled_kernel, dim3 ((unsigned)n, (unsigned)max_bands), dim3 (256), 0, 0, d_jobs);
    else hipLaunchKernelGGL (decode_pack_kernel, dim3 ((unsigned)n, (unsigned)max_bands), dim3 (256), 0, 0, d_jobs);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize (nullptr) == hipSuccess;
  }
  hipFree (d_jobs);
  return ok ? LH264_OK : LH264_E_HIP;
}

// a table of jobs the resize entry points take: windows the front end can deliver (even, up to 16,384 a side), reserved 0
static bool resize_jobs_ok (const lh264_pack_job_t* jobs, int n, int out_w, int out_h) {
  if (!jobs || n <= 0 || !lh264pack::size_ok (out_w, out_h)) return false;
  for (int k = 0; k < n; k++) {
    const lh264_pack_job_t& j = jobs[k];
    if (!j.y || !j.u || !j.v || !j.dst || j.crop_w <= 0 || j.crop_h <= 0 || j.crop_w > 16384 || j.crop_h > 16384 || ((j.crop_w | j.crop_h | j.crop_x | j.crop_y) & 1) ||
        j.crop_x < 0 || j.crop_y < 0 || (j.format != LH264_FMT_I420 && j.format != LH264_FMT_NV12) || j.reserved != 0) return false;
  }
  return true;
}

int lh264_debug_resize_cpu (const lh264_pack_job_t* jobs, int n, int out_w, int out_h) {
  if (!resize_jobs_ok (jobs, n, out_w, out_h)) return LH264_E_ARG;
  for (int k = 0; k < n; k++) for (int band = 0; band * lh264pack::kBandRows < out_h; band++) lh264pack::pack_band_resized (jobs[k], out_w, out_h, band, 0, 1);
  return LH264_OK;
}

int lh264_debug_resize_dev (const lh264_pack_job_t* jobs, int n, int out_w, int out_h) {
  if (!resize_jobs_ok (jobs, n, out_w, out_h)) return LH264_E_ARG;
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  lh264_pack_job_t* d_jobs = nullptr;
  bool ok = hipMalloc ((void**)&d_jobs, (size_t)n * sizeof (lh264_pack_job_t)) == hipSuccess && hipMemcpy (d_jobs, jobs, (size_t)n * sizeof (lh264_pack_job_t), hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL (decode_pack_resized_kernel, dim3 ((unsigned)n, (unsigned) ((out_h + lh264pack::kBandRows - 1) / lh264pack::kBandRows)), dim3 (256), 0, 0, d_jobs, out_w, out_h);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize (nullptr) == hipSuccess;
  }
  hipFree (d_jobs);
  return ok ? LH264_OK : LH264_E_HIP;
}

// a table the RGB entry points take: windows the front end can deliver, I420, a layout and standard bytes that are defined, and a sizing:
// the given size with reserved 0, or 0, 0 with reserved 0..3.  *max_bands: the bands of the tallest delivered picture
static bool rgb_jobs_ok (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job, int* max_bands) {
  if (!jobs || !std_per_job || n <= 0 || (layout != (int)LH264_COLOUR_RGB24 && layout != (int)LH264_COLOUR_RGBP)) return false;
  if ((out_w || out_h) && !lh264pack::size_ok (out_w, out_h)) return false;
  *max_bands = 1;
  for (int k = 0; k < n; k++) {
    const lh264_pack_job_t& j = jobs[k];
    if (!j.y || !j.u || !j.v || !j.dst || j.crop_w <= 0 || j.crop_h <= 0 || j.crop_w > 16384 || j.crop_h > 16384 || ((j.crop_w | j.crop_h | j.crop_x | j.crop_y) & 1) ||
        j.crop_x < 0 || j.crop_y < 0 || j.format != LH264_FMT_I420 || j.reserved < 0 || j.reserved > (out_w ? 0 : 3) || std_per_job[k] > 3) return false;
    int ow, oh;
    lh264pack::delivered_size (j.crop_w, j.crop_h, j.reserved, out_w, out_h, &ow, &oh);
    *max_bands = std::max (*max_bands, (oh + lh264pack::kBandRows - 1) / lh264pack::kBandRows);
  }
  return true;
}

int lh264_debug_rgb_cpu (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job) {
  int max_bands = 0;
  if (!rgb_jobs_ok (jobs, n, out_w, out_h, layout, std_per_job, &max_bands)) return LH264_E_ARG;
  for (int k = 0; k < n; k++) for (int band = 0; band < max_bands; band++) lh264pack::pack_band_rgb (jobs[k], out_w, out_h, layout, std_per_job[k], band, 0, 1);
  return LH264_OK;
}

int lh264_debug_rgb_dev (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job) {
  int max_bands = 0;
  if (!rgb_jobs_ok (jobs, n, out_w, out_h, layout, std_per_job, &max_bands)) return LH264_E_ARG;
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  lh264_pack_job_t* d_jobs = nullptr; uint8_t* d_std = nullptr;
  bool ok = hipMalloc ((void**)&d_jobs, (size_t)n * sizeof (lh264_pack_job_t)) == hipSuccess && hipMemcpy (d_jobs, jobs, (size_t)n * sizeof (lh264_pack_job_t), hipMemcpyHostToDevice) == hipSuccess &&
            hipMalloc ((void**)&d_std, (size_t)n) == hipSuccess && hipMemcpy (d_std, std_per_job, (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL (decode_pack_rgb_kernel, dim3 ((unsigned)n, (unsigned)max_bands), dim3 (256), 0, 0, d_jobs, d_std, out_w, out_h, layout);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize (nullptr) == hipSuccess;
  }
  hipFree (d_jobs); hipFree (d_std);
  return ok ? LH264_OK : LH264_E_HIP;
}

// a sample struct the call takes: 32 bytes, a type that is defined, with LH264_SAMPLE_U8 six floats whose bits are all clear, with a
// float type six finite floats
static bool sample_ok (const lh264_decode_sample_t* s) {
  if (s->struct_bytes != sizeof (lh264_decode_sample_t) || s->type > LH264_SAMPLE_BF16) return false;
  for (int k = 0; k < 6; k++) {
    uint32_t x;
    memcpy (&x, k < 3 ? &s->mul[k] : &s->add[k - 3], 4);
    if (s->type == LH264_SAMPLE_U8 ? x != 0 : (x & 0x7f800000u) == 0x7f800000u) return false;
  }
  return true;
}
// ... and what the float entry points take: a float type, every destination a multiple of 4
static bool sample_jobs_ok (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job, const lh264_decode_sample_t* sample, int* max_bands) {
  if (!sample || !sample_ok (sample) || sample->type == LH264_SAMPLE_U8 || !rgb_jobs_ok (jobs, n, out_w, out_h, layout, std_per_job, max_bands)) return false;
  for (int k = 0; k < n; k++) if ((uintptr_t)jobs[k].dst & 3u) return false;
  return true;
}

int lh264_debug_sample_cpu (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job, const lh264_decode_sample_t* sample) {
  int max_bands = 0;
  if (!sample_jobs_ok (jobs, n, out_w, out_h, layout, std_per_job, sample, &max_bands)) return LH264_E_ARG;
  for (int k = 0; k < n; k++) for (int band = 0; band < max_bands; band++) lh264pack::pack_band_sample (jobs[k], out_w, out_h, layout, std_per_job[k], *sample, band, 0, 1);
  return LH264_OK;
}

int lh264_debug_sample_dev (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job, const lh264_decode_sample_t* sample) {
  int max_bands = 0;
  if (!sample_jobs_ok (jobs, n, out_w, out_h, layout, std_per_job, sample, &max_bands)) return LH264_E_ARG;
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  lh264_pack_job_t* d_jobs = nullptr; uint8_t* d_std = nullptr;
  bool ok = hipMalloc ((void**)&d_jobs, (size_t)n * sizeof (lh264_pack_job_t)) == hipSuccess && hipMemcpy (d_jobs, jobs, (size_t)n * sizeof (lh264_pack_job_t), hipMemcpyHostToDevice) == hipSuccess &&
            hipMalloc ((void**)&d_std, (size_t)n) == hipSuccess && hipMemcpy (d_std, std_per_job, (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL (decode_pack_sample_kernel, dim3 ((unsigned)n, (unsigned)max_bands), dim3 (256), 0, 0, d_jobs, d_std, out_w, out_h, layout, *sample);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize (nullptr) == hipSuccess;
  }
  hipFree (d_jobs); hipFree (d_std);
  return ok ? LH264_OK : LH264_E_HIP;
}

int lh264_debug_sample_round (uint32_t type, const float* v, size_t n, uint16_t* out) {
  if ((type != LH264_SAMPLE_F16 && type != LH264_SAMPLE_BF16) || (n && (!v || !out))) return LH264_E_ARG;
  for (size_t k = 0; k < n; k++) out[k] = (uint16_t) (type == LH264_SAMPLE_F16 ? lh264pack::half_bits (v[k]) : lh264pack::bfloat_bits (v[k]));
  return LH264_OK;
}

// a table the placed entry points take: what the sibling of the path takes with a size, and a place per job that is one
static bool view_jobs_ok (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, int colour, const uint8_t* std_per_job, const lh264_decode_sample_t* sample, int* max_bands) {
  if (!places || !lh264pack::size_ok (out_w, out_h)) return false;
  const bool typed = sample && sample->type != LH264_SAMPLE_U8;
  if (sample && !sample_ok (sample)) return false;
  if (typed ? !sample_jobs_ok (jobs, n, out_w, out_h, colour, std_per_job, sample, max_bands) :
      colour ? !rgb_jobs_ok (jobs, n, out_w, out_h, colour, std_per_job, max_bands) : !resize_jobs_ok (jobs, n, out_w, out_h)) return false;
  *max_bands = (out_h + lh264pack::kBandRows - 1) / lh264pack::kBandRows;
  for (int k = 0; k < n; k++) if (!lh264pack::place_ok (places[k], out_w, out_h)) return false;
  return true;
}

int lh264_debug_view_cpu (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, int colour, const uint8_t* std_per_job, const lh264_decode_sample_t* sample) {
  int max_bands = 0;
  if (!view_jobs_ok (jobs, places, n, out_w, out_h, colour, std_per_job, sample, &max_bands)) return LH264_E_ARG;
  const bool typed = sample && sample->type != LH264_SAMPLE_U8;
  for (int k = 0; k < n; k++) for (int band = 0; band < max_bands; band++) {
    if (typed) lh264pack::pack_band_sample_placed (jobs[k], places[k], out_w, out_h, colour, std_per_job[k], *sample, band, 0, 1);
    else if (colour) lh264pack::pack_band_rgb_placed (jobs[k], places[k], out_w, out_h, colour, std_per_job[k], band, 0, 1);
    else lh264pack::pack_band_placed (jobs[k], places[k], out_w, out_h, band, 0, 1);
  }
  return LH264_OK;
}

int lh264_debug_view_dev (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, int colour, const uint8_t* std_per_job, const lh264_decode_sample_t* sample) {
  int max_bands = 0;
  if (!view_jobs_ok (jobs, places, n, out_w, out_h, colour, std_per_job, sample, &max_bands)) return LH264_E_ARG;
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  const bool typed = sample && sample->type != LH264_SAMPLE_U8;
  lh264_pack_job_t* d_jobs = nullptr; lh264_pack_place_t* d_places = nullptr; uint8_t* d_std = nullptr;
  bool ok = hipMalloc ((void**)&d_jobs, (size_t)n * sizeof (lh264_pack_job_t)) == hipSuccess && hipMemcpy (d_jobs, jobs, (size_t)n * sizeof (lh264_pack_job_t), hipMemcpyHostToDevice) == hipSuccess &&
            hipMalloc ((void**)&d_places, (size_t)n * sizeof (lh264_pack_place_t)) == hipSuccess && hipMemcpy (d_places, places, (size_t)n * sizeof (lh264_pack_place_t), hipMemcpyHostToDevice) == hipSuccess &&
            (!colour || (hipMalloc ((void**)&d_std, (size_t)n) == hipSuccess && hipMemcpy (d_std, std_per_job, (size_t)n, hipMemcpyHostToDevice) == hipSuccess));
  if (ok) {
    const dim3 grid ((unsigned)n, (unsigned)max_bands);
    if (typed) hipLaunchKernelGGL (decode_pack_sample_placed_kernel, grid, dim3 (256), 0, 0, d_jobs, d_places, d_std, out_w, out_h, colour, *sample);
    else if (colour) hipLaunchKernelGGL (decode_pack_rgb_placed_kernel, grid, dim3 (256), 0, 0, d_jobs, d_places, d_std, out_w, out_h, colour);
    else hipLaunchKernelGGL (decode_pack_placed_kernel, grid, dim3 (256), 0, 0, d_jobs, d_places, out_w, out_h);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize (nullptr) == hipSuccess;
  }
  hipFree (d_jobs); hipFree (d_places); hipFree (d_std);
  return ok ? LH264_OK : LH264_E_HIP;
}

int lh264_debug_motion_cpu (const lh264_motion_job_t* jobs, int n) {
  if (!jobs || n < 0) return LH264_E_ARG;
  for (int k = 0; k < n; k++) if (!lh264pack::motion_job_ok (jobs[k])) return LH264_E_ARG;
  for (int k = 0; k < n; k++) {
    const lh264_motion_job_t& j = jobs[k];
    for (int row = 0; row < j.mb_h; row++) for (int c0 = 0; c0 < j.mb_w; c0 += lh264pack::kMotionChunkMbs) {
      const lh264_mb_t* base = j.mbs + (size_t)row * j.mb_w + c0;
      uint32_t w[32];
      lh264pack::motion_chunk (j, j.back, row, c0, std::min (lh264pack::kMotionChunkMbs, j.mb_w - c0), [&] (int m) { memcpy (w, base + m, sizeof (w)); return (const uint32_t*)w; }, 0, 1);
    }
  }
  return LH264_OK;
}

int lh264_debug_motion_dev (const lh264_motion_job_t* jobs, int n) {
  if (!jobs || n < 0) return LH264_E_ARG;
  int units = 0;
  for (int k = 0; k < n; k++) {
    if (!lh264pack::motion_job_ok (jobs[k]) || ((uintptr_t)jobs[k].mbs & 15u)) return LH264_E_ARG;
    units = std::max (units, jobs[k].mb_h * lh264pack::motion_chunks (jobs[k].mb_w));
  }
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  if (!n) return LH264_OK;
  lh264_motion_job_t* d_jobs = nullptr;
  bool ok = hipMalloc ((void**)&d_jobs, (size_t)n * sizeof (lh264_motion_job_t)) == hipSuccess && hipMemcpy (d_jobs, jobs, (size_t)n * sizeof (lh264_motion_job_t), hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL (decode_pack_motion_kernel, dim3 ((unsigned)n, (unsigned)units), dim3 (256), 0, 0, d_jobs);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize (nullptr) == hipSuccess;
  }
  hipFree (d_jobs);
  return ok ? LH264_OK : LH264_E_HIP;
}

int lh264_debug_sha1 (const uint8_t* bytes, const uint64_t* spans, int n_spans, int n_messages, int on_device, uint8_t* out) {
  if (!out || n_spans < 0 || n_messages < 0 || (n_spans && (!spans || !bytes))) return LH264_E_ARG;
  std::vector<std::vector<std::pair<uint64_t, uint64_t>>> of ((size_t)n_messages);
  uint64_t end = 0;
  size_t steps = 1;
  for (int k = 0; k < n_spans; k++) {
    const uint64_t m = spans[3 * k], off = spans[3 * k + 1], ln = spans[3 * k + 2];
    if (m >= (uint64_t)n_messages || off + ln < off) return LH264_E_ARG;
    of[m].push_back ({off, ln});
    end = std::max (end, off + ln);
    steps = std::max (steps, of[m].size());
  }
  if (!n_messages) return LH264_OK;
  if (on_device && lh264_device_count() <= 0) return LH264_E_NODEVICE;
  std::vector<lh264_sha1_state_t> h_state ((size_t)n_messages);
  uint8_t* d_bytes = nullptr; lh264_sha1_state_t* d_state = nullptr; uint8_t* d_dig = nullptr; lh264_sha1_job_t* d_jobs = nullptr;
  bool ok = true;
  if (on_device) {
    ok = hipMalloc ((void**)&d_bytes, end + 16) == hipSuccess && hipMalloc ((void**)&d_state, (size_t)n_messages * sizeof (lh264_sha1_state_t)) == hipSuccess &&
         hipMalloc ((void**)&d_dig, (size_t)n_messages * 20) == hipSuccess && hipMalloc ((void**)&d_jobs, (size_t)n_messages * sizeof (lh264_sha1_job_t)) == hipSuccess &&
         (!end || hipMemcpy (d_bytes, bytes, end, hipMemcpyHostToDevice) == hipSuccess);
  }
  // step k: the k-th span of every message that has one (a message without spans is the empty message, ended in step 0)
  std::vector<lh264_sha1_job_t> jobs;
  for (size_t k = 0; k < steps && ok; k++) {
    jobs.clear();
    for (int m = 0; m < n_messages; m++) {
      const size_t ns = of[m].size();
      if (k >= ns && !(k == 0 && ns == 0)) continue;
      lh264_sha1_job_t j;
      j.src = (on_device ? d_bytes : bytes) + (ns ? of[m][k].first : 0); j.len = ns ? of[m][k].second : 0;
      j.state = on_device ? d_state + m : &h_state[m];
      j.out = (on_device ? d_dig : out) + (size_t)m * 20;
      j.flags = (k == 0 ? LH264_SHA1_FRESH : 0) | (k + 1 >= ns ? LH264_SHA1_FINAL : 0); j.reserved = 0;
      if (!(j.flags & LH264_SHA1_FINAL)) j.out = nullptr;
      jobs.push_back (j);
    }
    std::stable_sort (jobs.begin(), jobs.end(), [] (const lh264_sha1_job_t& a, const lh264_sha1_job_t& b) { return a.len > b.len; });
    if (!on_device) { for (const lh264_sha1_job_t& j : jobs) lh264sha1::run_job (j); continue; }
    if (jobs.empty()) continue;
    ok = hipMemcpy (d_jobs, jobs.data(), jobs.size() * sizeof (lh264_sha1_job_t), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) { hipLaunchKernelGGL (sha1_spans_kernel, dim3 ((unsigned) ((jobs.size() + 63) / 64)), dim3 (64), 0, 0, d_jobs, (int)jobs.size()); ok = hipGetLastError() == hipSuccess && hipStreamSynchronize (nullptr) == hipSuccess; }
  }
  if (on_device) {
    ok = ok && hipMemcpy (out, d_dig, (size_t)n_messages * 20, hipMemcpyDeviceToHost) == hipSuccess;
    hipFree (d_bytes); hipFree (d_state); hipFree (d_dig); hipFree (d_jobs);
  }
  return ok ? LH264_OK : LH264_E_HIP;
}

int lh264_decode_batch (const uint8_t* const* data, const size_t* len, int n, int threads, const lh264_decode_opts_t* opts, lh264_decoded_t** out) {
  return lh264_decode_batch_ex (data, len, n, threads, opts, nullptr, out);
}

int lh264_decode_batch_ex (const uint8_t* const* data, const size_t* len, int n, int threads, const lh264_decode_opts_t* opts, const lh264_decode_ext_t* ext, lh264_decoded_t** out) {
  return lh264_decode_batch_ex2 (data, len, n, threads, opts, ext, nullptr, out);
}

int lh264_decode_batch_ex2 (const uint8_t* const* data, const size_t* len, int n, int threads, const lh264_decode_opts_t* opts, const lh264_decode_ext_t* ext, const lh264_decode_sample_t* sample, lh264_decoded_t** out) {
  return lh264_decode_batch_ex3 (data, len, n, threads, opts, ext, sample, nullptr, out);
}

int lh264_decode_batch_ex3 (const uint8_t* const* data, const size_t* len, int n, int threads, const lh264_decode_opts_t* opts, const lh264_decode_ext_t* ext, const lh264_decode_sample_t* sample, const lh264_decode_view_t* view, lh264_decoded_t** out) {
  return lh264_decode_batch_ex4 (data, len, n, threads, opts, ext, sample, view, nullptr, out);
}

int lh264_decode_batch_ex4 (const uint8_t* const* data, const size_t* len, int n, int threads, const lh264_decode_opts_t* opts, const lh264_decode_ext_t* ext, const lh264_decode_sample_t* sample, const lh264_decode_view_t* view, const lh264_decode_motion_t* motion, lh264_decoded_t** out) {
  if (!data || !len || !out || n < 0) return LH264_E_ARG;
  if (motion && (motion->struct_bytes != sizeof (lh264_decode_motion_t) || motion->fields > LH264_MOTION_FIELDS || motion->reserved0 != 0 || motion->reserved1 != 0)) return LH264_E_ARG;
  // 0: the call is lh264_decode_batch_ex3; else decode_pack_motion_kernel gathers the round's records in front of the reconstruct launch
  const uint32_t fields = motion ? motion->fields : 0;
  if (view && (view->struct_bytes != sizeof (lh264_decode_view_t) || view->fit > LH264_FIT_CONTAIN || view->reserved0 != 0 || view->reserved1 != 0 ||
               (view->fill && (view->fit != LH264_FIT_CONTAIN || view->fill >> 24)) || (view->n_crops != 0 && view->n_crops != 1 && view->n_crops != (uint32_t)n) ||
               (view->n_crops != 0 && !view->crops))) return LH264_E_ARG;
  if (view) for (uint32_t k = 0; k < view->n_crops; k++) if (!crop_ok (view->crops[k])) return LH264_E_ARG;
  // the view: the fit, the bars' fill, and every stream's crop (w = 0: none)
  const uint32_t fit = view ? view->fit : LH264_FIT_STRETCH, fill = view ? view->fill : 0;
  std::vector<lh264_rect_t> crops ((size_t)n, lh264_rect_t {0, 0, 0, 0});
  if (view && view->n_crops) for (int i = 0; i < n; i++) crops[i] = view->crops[view->n_crops == 1 ? 0 : i];
  if (ext && ext->struct_bytes != sizeof (lh264_decode_ext_t)) return LH264_E_ARG;      // (before ext->colour is read below)
  if (sample && (!sample_ok (sample) || (sample->type != LH264_SAMPLE_U8 && (!ext || ext->colour == LH264_COLOUR_YUV)))) return LH264_E_ARG;
  // 0: bytes, the pack kernels as ever; else decode_pack_sample_kernel in decode_pack_rgb_kernel's place, es bytes per element
  const int stype = sample ? (int)sample->type : (int)LH264_SAMPLE_U8;
  const size_t es = stype == (int)LH264_SAMPLE_U8 ? 1 : stype == (int)LH264_SAMPLE_F32 ? 4 : 2;
  lh264_decode_sample_t sample_arg;
  memset (&sample_arg, 0, sizeof (sample_arg));
  if (sample) sample_arg = *sample;
  if (ext && (ext->struct_bytes != sizeof (lh264_decode_ext_t) || ext->colour > LH264_COLOUR_RGBP || ext->matrix > LH264_MATRIX_BT709 || ext->range > LH264_RANGE_FULL ||
              ext->reserved0 != 0 || ext->reserved1 != 0 || (ext->colour == LH264_COLOUR_YUV && (ext->matrix != LH264_MATRIX_AUTO || ext->range != LH264_RANGE_AUTO)) ||
              (ext->colour != LH264_COLOUR_YUV && opts && opts->format != LH264_FMT_I420))) return LH264_E_ARG;
  // 0: the planes, decode_pack_kernel and its siblings as ever; else decode_pack_rgb_kernel in their place, 3 bytes per delivered luma sample
  const int colour = ext ? (int)ext->colour : 0;
  const uint32_t ext_matrix = ext ? ext->matrix : LH264_MATRIX_AUTO, ext_range = ext ? ext->range : LH264_RANGE_AUTO;
  if (opts && ((opts->struct_bytes != sizeof (lh264_decode_opts_t) && opts->struct_bytes != LH264_DECODE_OPTS_BYTES_V5 && opts->struct_bytes != LH264_DECODE_OPTS_BYTES_V4 && opts->struct_bytes != LH264_DECODE_OPTS_BYTES_V3 && opts->struct_bytes != LH264_DECODE_OPTS_BYTES_V2 && opts->struct_bytes != LH264_DECODE_OPTS_BYTES_V1) || opts->format > LH264_FMT_NV12 ||
               (opts->flags & ~ (LH264_DECODE_DEVICE_OUT | LH264_DECODE_SHA1_PICTURES | LH264_DECODE_SHA1_STREAM | LH264_DECODE_NO_PICTURES)) ||
               (opts->sink && (opts->flags & LH264_DECODE_DEVICE_OUT)) ||
               ((opts->flags & LH264_DECODE_NO_PICTURES) && ((!fields && (!(opts->flags & (LH264_DECODE_SHA1_PICTURES | LH264_DECODE_SHA1_STREAM)) || (opts->flags & LH264_DECODE_DEVICE_OUT))) || opts->sink)))) return LH264_E_ARG;
  const int conceal = opts && opts->struct_bytes >= LH264_DECODE_OPTS_BYTES_V2 ? (int)opts->conceal : 0;
  const uint32_t parse = opts && opts->struct_bytes >= LH264_DECODE_OPTS_BYTES_V3 ? opts->parse : LH264_PARSE_HOST;
  if (parse != LH264_PARSE_HOST && parse != LH264_PARSE_DEVICE) return LH264_E_ARG;
  const uint32_t parse_flags = opts && opts->struct_bytes >= LH264_DECODE_OPTS_BYTES_V3 ? opts->parse_flags : 0;
  if ((parse_flags & ~LH264_PARSE_FLAG_CABAC) || (parse_flags && parse != LH264_PARSE_DEVICE)) return LH264_E_ARG;
  const bool opts_v4 = opts && opts->struct_bytes >= LH264_DECODE_OPTS_BYTES_V4;
  if (opts_v4 && (opts->scale_log2 > 3 || opts->reserved2 != 0)) return LH264_E_ARG;
  const int scale = opts_v4 ? (int)opts->scale_log2 : 0;      // 0: decode_pack_kernel, as ever; 1..3: decode_pack_scaled_kernel
  const bool opts_v5 = opts && opts->struct_bytes >= LH264_DECODE_OPTS_BYTES_V5;
  if (opts_v5 && (opts->pick > LH264_PICK_IDR || opts->reserved3 != 0 || (opts->pick != LH264_PICK_ALL && conceal != 0))) return LH264_E_ARG;
  const uint32_t pick = opts_v5 ? opts->pick : LH264_PICK_ALL;
  const bool picking = pick != LH264_PICK_ALL;      // unselected pictures are walked by their headers only, every selected one is a chain
  const bool opts_v6 = opts && opts->struct_bytes == sizeof (lh264_decode_opts_t);
  const bool sized = opts_v6 && (opts->out_width || opts->out_height);
  if (opts_v6 && (opts->reserved4 != 0 || opts->reserved5 != 0 || (sized && (!lh264pack::size_ok (opts->out_width, opts->out_height) || scale != 0)))) return LH264_E_ARG;
  const int out_w = sized ? (int)opts->out_width : 0, out_h = sized ? (int)opts->out_height : 0;      // 0, 0: the window (or its scale); else decode_pack_resized_kernel
  if (fit != LH264_FIT_STRETCH && !out_w) return LH264_E_ARG;
  const bool placed = fit == LH264_FIT_CONTAIN;      // the placed kernels and a place per pack job (else the kernels of the calls above, whatever the crop)
  if (!Parser::conceal_method_ok (conceal)) return LH264_E_ARG;           // a method that is not provided (FRAME_COPY), or no method at all
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  const int format = opts ? (int)opts->format : LH264_FMT_I420;
  const bool device_out = opts && (opts->flags & LH264_DECODE_DEVICE_OUT);
  const bool no_pictures = opts && (opts->flags & LH264_DECODE_NO_PICTURES);          // digests only: nothing is downloaded or kept
  const bool sha_pics = opts && (opts->flags & LH264_DECODE_SHA1_PICTURES), sha_stream = opts && (opts->flags & LH264_DECODE_SHA1_STREAM);
  const bool sha = sha_pics || sha_stream;
  const bool motion_only = fields && no_pictures && !sha;      // no picture pool, no reconstruct, pack or digest kernel
  const bool down = !device_out && (!no_pictures || fields);   // the round has bytes to bring down on the second stream
  double motion_ms = 0; unsigned long long motion_bytes = 0;   // lh264_decode_last_motion
  const lh264_decode_sink_fn sink = opts ? opts->sink : nullptr;
  void* const sink_user = opts ? opts->user : nullptr;
  const size_t R = opts && opts->round_pictures ? opts->round_pictures : kDefaultRoundPictures;
  const size_t group_mbs = opts && opts->group_mbs ? (size_t)opts->group_mbs : (size_t)kDefaultGroupMbs;
  if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
  if (threads < 1) threads = 1;
  int device = 0;
  if (hipGetDevice (&device) != hipSuccess || device < 0 || device >= lh264host::kMaxDevices) return LH264_E_ARG;
  for (int i = 0; i < n; i++) { out[i] = new lh264_decoded(); out[i]->device = device; out[i]->sample_type = stype; out[i]->fields = fields; out[i]->sha = opts ? opts->flags & (LH264_DECODE_SHA1_PICTURES | LH264_DECODE_SHA1_STREAM) : 0; }
  auto arena_lock = g_arena.lock (device);
  Arena& A = arena_lock.get();
  if (!A.init()) { for (int i = 0; i < n; i++) { out[i]->status = LH264_E_HIP; out[i]->error = "creating the HIP streams failed"; } return LH264_OK; }
  const double t_call = now_s();
  long long n_rounds = 0, n_launched = 0, n_launched_jobs = 0;      // lh264_decode_last_chains
  double t_parse = 0, t_stage = 0, t_enqueue = 0, t_wait = 0, t_deliver = 0, t_dev_parse = 0, n_dev_slices = 0;

  std::vector<std::unique_ptr<DStream>> active;
  std::vector<std::unique_ptr<DStream>> retired;   // streams that are through (a round on the device still names them)
  int next_stream = 0;
  const int kWave = std::max (8, 4 * threads);
  Round rounds[2];
  int rb = 0;                                       // the buffers the next round takes
  bool device_failed = false;
  std::string device_error;
  const bool parse_dev = parse == LH264_PARSE_DEVICE && conceal == 0;      // (concealment builds records on the host)
  // LH264_SLICE_PARSE_FAIL=k (tests): task k of the call's first parse launch reports a status unwalked, which forces the fallback
  int force_fail = parse_dev && getenv ("LH264_SLICE_PARSE_FAIL") ? atoi (getenv ("LH264_SLICE_PARSE_FAIL")) : -1;
  // LH264_PARSE_FLAG_CABAC: CABAC slices are deferred and become tasks too; LH264_SLICE_PARSE_FAIL_CABAC=k: the same for task k of the
  // call's first CABAC launch
  const bool parse_cabac = parse_dev && (parse_flags & LH264_PARSE_FLAG_CABAC);
  int force_fail_cabac = parse_cabac && getenv ("LH264_SLICE_PARSE_FAIL_CABAC") ? atoi (getenv ("LH264_SLICE_PARSE_FAIL_CABAC")) : -1;

  auto release_pool = [&] (DStream& s) {
    for (Slot& sl : s.pool) A.pics.put (s.geo.bytes, sl.base);
    s.pool.clear();
  };
  auto finish = [&] (DStream& s) {                  // the stream leaves: its result stands, its memory goes back
    lh264_decoded_t& r = *out[s.i];
    if (r.status == LH264_OK && device_failed) { r.status = LH264_E_HIP; r.error = device_error; }
    if (r.status == LH264_OK && s.end_code != LH264_OK) { r.status = s.end_code; r.error = s.end_text; }
    release_pool (s);
    s.parser.reset(); s.pending.clear(); s.sel.clear();
  };

  // host threads: parse until the stream has a round's pictures (or ends), then pick the round's pictures
  // tentative (a stream on the device route): the round's candidates, before their slice data is parsed - nothing is refused yet
  auto fill_and_select = [&] (DStream& s, bool fill, bool tentative) {
    Parser& P = *s.parser;
    while (fill && s.pending.size() < R && !P.file_finished()) {
      const size_t want = s.pic_mbs ? (R - s.pending.size()) * s.pic_mbs - 1 : 0;
      P.feed_file_some (want);
      for (auto& f : P.frames()) {
        s.pic_mbs = (size_t)f->mb_w * f->mb_h;
        s.seen = f->index + 1;
        // (slices parsed on the spot; the deferred ones are counted where they are resolved)
        out[s.i]->parsed_slices += (long) (f->slices.size() - f->deferred.size());
        // opts->pick: an unselected picture leaves here, its slice data unseen
        if (picking && !picture_selected (*f, pick)) continue;
        s.pending.push_back (std::move (f));
      }
      P.frames().clear();
    }
    s.ending = false; s.end_code = LH264_OK; s.end_text.clear();
    const bool has_err = !tentative && !P.error().empty();
    const long limit = has_err ? P.error_pictures() : 0x7fffffffffffffffl;
    while (s.sel.size() < R) {
      // the picture's number in the stream: with opts->pick the next selected picture's own, or where the pictures seen so far end
      const long idx = !picking ? s.next_picture + (long)s.sel.size() : !s.pending.empty() ? s.pending.front()->index : s.seen;
      if (idx >= limit) { s.ending = true; s.end_code = LH264_E_UNSUPPORTED; s.end_text = "picture " + std::to_string (picking ? limit : idx) + ": " + P.error(); break; }
      if (s.pending.empty()) {
        if (P.file_finished()) { s.ending = true; if (has_err) { s.end_code = LH264_E_UNSUPPORTED; s.end_text = P.error(); } }
        break;
      }
      FrameOut& f = *s.pending.front();
      // a change of resolution ends the round: the next one starts with a new pool.  (Asked first: on the device route the tentative
      // pass stopped here too, so the picture's slice data is not parsed yet and there is nothing to refuse it by)
      if (!s.sel.empty() && (f.mb_w != s.sel[0]->mb_w || f.mb_h != s.sel[0]->mb_h)) break;
      std::string why = tentative ? std::string() : refuse_picture (f);
      if (!tentative && why.empty() && colour && picture_standard (f, ext_matrix, ext_range) > 3) why = "matrix_coefficients " + std::to_string (f.matrix_coefficients) + " has no conversion here (BT.601: 5, 6, 2 or none; BT.709: 1): name a matrix";
      if (!why.empty()) { s.ending = true; s.end_code = LH264_E_UNSUPPORTED; s.end_text = "picture " + std::to_string (idx) + ": " + why; break; }
      // the caller's crop against this picture's window (a stream may change size): the stream stops here, as for the matrix
      const lh264_rect_t& cr = crops[s.i];
      if (!tentative && cr.w && !crop_fits (cr, f.crop_w, f.crop_h)) {
        s.ending = true; s.end_code = LH264_E_ARG;
        s.end_text = "picture " + std::to_string (idx) + ": the crop {" + std::to_string (cr.x) + ", " + std::to_string (cr.y) + ", " + std::to_string (cr.w) + ", " + std::to_string (cr.h) +
                     "} does not fit the picture's " + std::to_string (f.crop_w) + " x " + std::to_string (f.crop_h) + " window";
        break;
      }
      s.sel.push_back (std::move (s.pending.front())); s.pending.pop_front();
    }
  };
  // what the call delivers for a picture of stream s: its view's size (a picture select() let through: the crop fits)
  auto delivered = [&] (const DStream& s, const FrameOut& f, int* ow, int* oh) {
    lh264_rect_t vs, vd;
    view_of (f.crop_w, f.crop_h, crops[s.i], fit, scale, out_w, out_h, &vs, &vd, ow, oh);
  };
  auto unselect = [&] (DStream& s) {                // the round was full: the pictures wait for the next one
    for (size_t q = s.sel.size(); q-- > 0; ) s.pending.push_front (std::move (s.sel[q]));
    s.sel.clear(); s.ending = false;
  };

  auto fail_device = [&] (const std::string& what) {
    device_failed = true; device_error = what;
    const char* he = hipGetErrorString (hipGetLastError());
    if (he && *he) device_error += std::string (" (") + he + ")";
  };

  // a round that is on the device: wait for its bytes and hand them on
  auto deliver = [&] (Round& rd, int b) {
    if (!rd.live) return;
    rd.live = false;
    const double t0 = now_s();
    if (!device_failed && hipEventSynchronize (down ? A.e_down[b] : A.e_run[b]) != hipSuccess) fail_device ("the device stage failed");
    const double t1 = now_s();
    t_wait += t1 - t0;
    if (device_failed) {
      for (RoundChain& c : rd.chains) { c.s->stopped = true; lh264_decoded_t& r = *out[c.s->i]; if (r.status == LH264_OK) { r.status = LH264_E_HIP; r.error = device_error; } }
      return;
    }
    const uint8_t* hb = A.h_out[b].as<uint8_t>();
    if (rd.timed) { float ms = 0; if (hipEventElapsedTime (&ms, A.e_mot[b][0], A.e_mot[b][1]) == hipSuccess) motion_ms += ms; motion_bytes += rd.mot_bytes + rd.mbi_bytes; }
    // the round's fields: geometry per picture, and in host mode the chain's blocks behind what the handle holds
    auto take_fields = [&] (RoundChain& c, lh264_decoded_t& r) {
      r.motion_geo.insert (r.motion_geo.end(), c.motion_geo.begin(), c.motion_geo.end());
      if (device_out) return;
      const uint8_t* hm = A.h_mot[b].as<uint8_t>(); const uint8_t* hi = A.h_mbi[b].as<uint8_t>();
      r.mot.insert (r.mot.end(), hm + c.mot_at, hm + c.mot_at + c.mot_bytes);
      r.mbi.insert (r.mbi.end(), hi + c.mbi_at, hi + c.mbi_at + c.mbi_bytes);
    };
    // the round's digests came down on the run stream, in front of the event: the pictures' 20 bytes, and the stream's record as this
    // round leaves it (a stream's digest covers the rounds that were delivered, whatever is on the device behind them)
    const uint8_t* hd = A.h_dig[b].as<uint8_t>();
    auto take_digests = [&] (RoundChain& c, lh264_decoded_t& r, int k) {
      if (sha_pics) r.pic_sha.insert (r.pic_sha.end(), hd + c.dig0 * 20, hd + (c.dig0 + c.pics.size()) * 20);
      if (sha_stream) memcpy (&r.stream_state, hd + rd.dig_states_at + (size_t)k * sizeof (lh264_sha1_state_t), sizeof (lh264_sha1_state_t));
    };
    if (sink) {
      for (size_t k = 0; k < rd.chains.size(); k++) {
        RoundChain& c = rd.chains[k];
        if (c.s->stopped) continue;
        lh264_decoded_t& r = *out[c.s->i];
        if (c.pics.empty()) continue;
        if (sink (sink_user, c.s->i, c.first_picture, (int)c.pics.size(), c.pics.data(), hb + c.at, c.bytes) != 0) {
          c.s->stopped = true; r.status = LH264_E_ARG; r.error = "sink";
          continue;
        }
        r.pics.insert (r.pics.end(), c.pics.begin(), c.pics.end());
        r.concealed.insert (r.concealed.end(), c.concealed.begin(), c.concealed.end());
        r.source_wh.insert (r.source_wh.end(), c.source_wh.begin(), c.source_wh.end());
        r.view.insert (r.view.end(), c.view.begin(), c.view.end());
        r.index.insert (r.index.end(), c.index.begin(), c.index.end());
        r.colour.insert (r.colour.end(), c.colour.begin(), c.colour.end());
        if (sha) take_digests (c, r, (int)k);
        if (fields) take_fields (c, r);
      }
    } else {
      run_parallel ((int)rd.chains.size(), threads, [&] (int k) {
        RoundChain& c = rd.chains[k];
        if (c.s->stopped) return;
        lh264_decoded_t& r = *out[c.s->i];
        if (!device_out && !no_pictures) r.bytes.insert (r.bytes.end(), hb + c.at, hb + c.at + c.bytes);
        r.pics.insert (r.pics.end(), c.pics.begin(), c.pics.end());
        r.concealed.insert (r.concealed.end(), c.concealed.begin(), c.concealed.end());
        r.source_wh.insert (r.source_wh.end(), c.source_wh.begin(), c.source_wh.end());
        r.view.insert (r.view.end(), c.view.begin(), c.view.end());
        r.index.insert (r.index.end(), c.index.begin(), c.index.end());
        r.colour.insert (r.colour.end(), c.colour.begin(), c.colour.end());
        if (sha) take_digests (c, r, k);
        if (fields) take_fields (c, r);
      });
    }
    t_deliver += now_s() - t1;
  };

  for (;;) {
    // ---- who takes part: streams that are through leave, new ones are admitted while the round has room
    for (size_t k = 0; k < active.size(); ) {
      DStream& s = *active[k];
      if (s.stopped || s.ending) { finish (s); retired.push_back (std::move (active[k])); active.erase (active.begin() + (long)k); } else k++;
    }
    if (device_failed) break;
    {
      size_t known = 0, known_mbs = 0;
      for (auto& s : active) if (s->pic_mbs) { known++; known_mbs += s->pic_mbs; }
      const size_t avg = known ? std::max<size_t> (1, known_mbs / known) : 396;
      size_t used = 0;
      for (auto& s : active) used += (s->pic_mbs ? s->pic_mbs : avg) * R;
      int admitted = 0;
      while (next_stream < n && (active.empty() || used + avg * R <= group_mbs) && (known || admitted < kWave)) {
        std::unique_ptr<DStream> s (new DStream());
        s->i = next_stream++;
        s->parser.reset (new Parser());
        s->parser->set_sparse_coeffs (true);
        s->parser->set_sparse_levels (true);       // (the parser has no mode without levels: their list is the cheapest form)
        s->parser->set_conceal (conceal);
        s->dev_route = parse_dev;
        s->parser->set_defer_slice_data (parse_dev || picking);
        s->parser->set_defer_cabac (parse_cabac || picking);
        s->parser->begin_file (data[s->i], data[s->i] ? len[s->i] : 0);
        active.push_back (std::move (s));
        used += avg * R; admitted++;
      }
    }
    if (active.empty()) break;
    const double t_a = now_s();
    run_parallel ((int)active.size(), threads, [&] (int k) { fill_and_select (*active[k], true, parse_dev || picking); });
    if (parse_dev || picking) {
      // ---- the round's CAVLC slice data on the device: payloads and tasks up, slice_parse_kernel, 12 bytes per slice down; then the
      // round's pictures are picked as ever.  On the run stream, behind the round before (whose kernels still read the parse arena),
      // and waited for: the results decide what the round holds
      const double t_p0 = now_s();
      struct TRef { DStream* s; FrameOut* f; size_t def, bytes_at; };
      std::vector<TRef> refs;
      size_t pm = 0, pb = 0;
      for (auto& sp : active) {
        DStream& s = *sp;
        s.dev_at.clear();
        for (auto& fp : s.sel) {
          FrameOut& f = *fp;
          if (f.deferred.empty()) {
            // a picture of CABAC slices (parsed on the spot): the stream stays with the host parser from here on
            if (!f.slices.empty() && s.dev_route) { s.dev_route = false; s.parser->set_defer_slice_data (false); }
            continue;
          }
          // (opts->pick defers every slice, whoever parses it: without LH264_PARSE_FLAG_CABAC a CABAC picture is the host's all the same)
          if (picking && !parse_cabac && f.deferred[0].cabac) { s.dev_route = false; continue; }
          if (!s.dev_route) continue;
          s.dev_at[&f] = {pm};
          pm += (size_t)f.mb_w * f.mb_h;
          for (size_t d = 0; d < f.deferred.size(); d++) refs.push_back ({&s, &f, d, 0});
        }
      }
      std::stable_sort (refs.begin(), refs.end(), [] (const TRef& a, const TRef& b) { return a.f->deferred[a.def].rbsp.size() > b.f->deferred[b.def].rbsp.size(); });
      // (the CAVLC tasks in front of the CABAC ones, longest first within each: one launch per kernel)
      const size_t n_cavlc = (size_t) (std::stable_partition (refs.begin(), refs.end(), [] (const TRef& a) { return !a.f->deferred[a.def].cabac; }) - refs.begin());
      auto line_bytes = [] (const TRef& r) { return (size_t)r.f->mb_w * (r.f->deferred[r.def].cabac ? (size_t)lh264slice::kCabacLineBytes : 4); };
      for (TRef& r : refs) {
        r.bytes_at = pb;
        pb += ((r.f->deferred[r.def].rbsp.size() + 15) & ~ (size_t)15) + 224 + (r.f->mb_w > lh264slice::kLdsLineMbs ? ((line_bytes (r) + 15) & ~ (size_t)15) : 0);
      }
      const size_t nt = refs.size();
      bool ok = true;
      if (nt) {
        ok = A.d_pbytes.alloc (pb) && A.h_pbytes.alloc (pb) && A.d_ptasks.alloc (nt * sizeof (lh264host::SliceTask)) && A.h_ptasks.alloc (nt * sizeof (lh264host::SliceTask)) &&
             A.d_pres.alloc (nt * sizeof (lh264host::SliceResult)) && A.h_pres.alloc (nt * sizeof (lh264host::SliceResult)) &&
             A.d_pmbs.alloc (pm * sizeof (lh264_mb_t)) && A.d_pcoef.alloc (pm * 768);
        if (ok) {
          uint8_t* hb = A.h_pbytes.as<uint8_t>(); uint8_t* db = A.d_pbytes.as<uint8_t>();
          lh264host::SliceTask* ht = A.h_ptasks.as<lh264host::SliceTask>();
          run_parallel ((int)nt, threads, [&] (int j) {
            const TRef& r = refs[(size_t)j];
            const FrameOut& f = *r.f;
            const lh264host::DeferredSlice& ds = f.deferred[r.def];
            const DStream::DevAt at = r.s->dev_at.at (r.f);
            const int n = f.mb_w * f.mb_h;
            const size_t sc_at = r.bytes_at + ((ds.rbsp.size() + 15) & ~ (size_t)15);
            if (!ds.rbsp.empty()) memcpy (hb + r.bytes_at, ds.rbsp.data(), ds.rbsp.size());
            memcpy (hb + sc_at, ds.pps.sl4, 96); memcpy (hb + sc_at + 96, ds.pps.sl8, 128);
            lh264host::SliceTask& t = ht[j];
            memset (&t, 0, sizeof (t));
            t.rbsp = db + r.bytes_at; t.rbsp_bytes = (uint32_t)ds.rbsp.size(); t.data_bit = (uint32_t)ds.data_bit;
            t.first_mb = ds.sh.first_mb;
            t.limit_mb = (size_t)ds.sid + 1 < f.slices.size() ? std::min (n, f.slices[(size_t)ds.sid + 1].first_mb) : n;
            t.mb_w = f.mb_w; t.mb_h = f.mb_h; t.slice_index = ds.sid; t.slice_qp = ds.sh.slice_qp;
            t.slice_type = (uint8_t)ds.sh.slice_type; t.num_ref_idx_l0 = (uint8_t)ds.sh.num_ref_idx_l0;
            t.transform_8x8 = ds.pps.transform_8x8; t.constrained_intra_pred = ds.pps.constrained_intra_pred;
            t.use_sl = ds.sps_scaling || ds.pps.scaling_matrix_present;
            t.chroma_qp_offset[0] = (int8_t)ds.pps.chroma_qp_offset[0]; t.chroma_qp_offset[1] = (int8_t)ds.pps.chroma_qp_offset[1];
            if (ds.cabac) t.reserved = (uint8_t) (lh264slice::kTaskCabac | (ds.sh.cabac_init_idc & 3));
            t.scaling = db + sc_at;
            t.mbs = A.d_pmbs.as<lh264_mb_t>() + at.mb; t.coeffs = A.d_pcoef.as<int16_t>() + at.mb * 384;
            t.slice = nullptr;                                  // (the host fills n_mbs in from the result; the table is staged as ever)
            t.line = f.mb_w > lh264slice::kLdsLineMbs ? (int8_t*) (db + sc_at + 224) : nullptr;
          });
          hipStream_t st = A.s_run;
          ok = hipMemcpyAsync (A.d_pbytes.p, hb, pb, hipMemcpyHostToDevice, st) == hipSuccess &&
               hipMemcpyAsync (A.d_ptasks.p, ht, nt * sizeof (lh264host::SliceTask), hipMemcpyHostToDevice, st) == hipSuccess &&
               hipMemsetAsync (A.d_pmbs.p, 0, pm * sizeof (lh264_mb_t), st) == hipSuccess && hipMemsetAsync (A.d_pcoef.p, 0, pm * 768, st) == hipSuccess &&
               lh264host::launch_slice_parse (A.d_ptasks.as<lh264host::SliceTask>(), A.d_pres.as<lh264host::SliceResult>(), (int)n_cavlc, st, force_fail) &&
               lh264host::launch_slice_parse_cabac (A.d_ptasks.as<lh264host::SliceTask>() + n_cavlc, A.d_pres.as<lh264host::SliceResult>() + n_cavlc, (int) (nt - n_cavlc), st, force_fail_cabac) &&
               hipMemcpyAsync (A.h_pres.p, A.d_pres.p, nt * sizeof (lh264host::SliceResult), hipMemcpyDeviceToHost, st) == hipSuccess &&
               hipStreamSynchronize (st) == hipSuccess;
          if (n_cavlc) force_fail = -1;
          if (nt > n_cavlc) force_fail_cabac = -1;
        }
        if (!ok) {
          fail_device ("the slice parse stage failed");
          for (auto& s : active) { s->dev_at.clear(); unselect (*s); }
          deliver (rounds[rb ^ 1], rb ^ 1);
          continue;
        }
      }
      if (ok && nt) {
        const lh264host::SliceResult* res = A.h_pres.as<lh264host::SliceResult>();
        // a status anywhere in a stream's round: the whole round of that stream goes back to the host parser, and the stream stays there
        for (size_t j = 0; j < nt; j++) if (res[j].status != lh264slice::SLICE_OK && refs[j].s->dev_route) {
          DStream& s = *refs[j].s;
          s.dev_route = false; s.dev_at.clear();
          if (!picking) s.parser->set_defer_slice_data (false);
          out[s.i]->parse_path = LH264_PARSE_PATH_FALLBACK;
        }
        for (size_t j = 0; j < nt; j++) {
          const TRef& r = refs[j];
          if (!r.s->dev_route) continue;
          FrameOut& f = *r.f;
          lh264host::DeferredSlice& ds = f.deferred[r.def];
          if (!ds.counted) { ds.counted = true; out[r.s->i]->parsed_slices++; }
          if (out[r.s->i]->parse_path == LH264_PARSE_PATH_HOST) out[r.s->i]->parse_path = LH264_PARSE_PATH_DEVICE;
          out[r.s->i]->device_slices++;
          if (ds.cabac) out[r.s->i]->device_cabac_slices++;
          // what parse_slice_data_cavlc / _cabac leaves with the picture: n_mbs, coverage, the slice's syntax entry
          f.slices[(size_t)ds.sid].n_mbs = res[j].n_mbs;
          for (int k = 0; k < res[j].n_mbs; k++) f.covered[(size_t) (ds.sh.first_mb + k)] = 1;
          lh264host::SliceSyn ss;
          const size_t stop = (size_t)res[j].stop_bit;
          ss.pad_bits = 7 - (int) (stop & 7);
          ss.pad_value = (ss.pad_bits && (stop >> 3) < ds.rbsp.size()) ? (ds.rbsp[stop >> 3] & ((1 << ss.pad_bits) - 1)) : 0;
          ss.transform8x8_pps = ds.pps.transform_8x8 ? 1 : 0;
          ss.flags = ds.pps.constrained_intra_pred ? 2 : 0;
          if (ds.cabac) { ss.pad_bits = 7; ss.pad_value = ds.rbsp.empty() ? 0 : ds.rbsp.back() & 0x7f; ss.flags |= 1; }
          if (f.slice_syn.size() <= (size_t)ds.sid) f.slice_syn.resize ((size_t)ds.sid + 1);
          f.slice_syn[(size_t)ds.sid] = ss;
        }
      }
      if (parse_dev) { t_dev_parse += now_s() - t_p0; n_dev_slices += (double)nt; }
      // whatever was deferred and did not stay on the device is parsed by the host parser now (a fallback, the pictures behind a CABAC
      // picture); then the round's pictures are picked with everything known
      run_parallel ((int)active.size(), threads, [&] (int k) {
        DStream& s = *active[k];
        auto resolve = [&] (FrameOut& f) {
          if (s.dev_at.count (&f)) return;
          for (size_t d = 0; d < f.deferred.size(); d++) {
            lh264host::DeferredSlice& ds = f.deferred[d];
            if (!ds.resolved && !ds.counted) { ds.counted = true; out[s.i]->parsed_slices++; }
            s.parser->parse_deferred (f, d);
          }
        };
        for (auto& f : s.sel) resolve (*f);
        if (!s.dev_route) for (auto& f : s.pending) resolve (*f);
        unselect (s);
        fill_and_select (s, false, false);
      });
    }
    const double t_b = now_s();
    t_parse += t_b - t_a;

    // ---- the round: which streams fit, where their records and bytes go, which picture slots they take
    // (the buffers `rb` were last used by the round before the one that is on the device now: it has been delivered)
    Round& rd = rounds[rb];
    rd.chains.clear(); rd.out_bytes = 0; rd.mot_bytes = 0; rd.mbi_bytes = 0; rd.timed = false;
    size_t n_mjobs = 0; int max_units = 1;      // fields: the round's motion jobs (its delivered pictures), the most chunks of one of them
    struct Place { size_t mb0, sl0, sp0, job0; };
    std::vector<Place> place;
    size_t n_mbs = 0, n_hmbs = 0, n_sl = 0, n_sp = 0, n_jobs = 0, n_out = 0;      // n_hmbs: the macroblocks whose records the host stages (not those in the parse arena)
    int max_w = 1, max_h = 1, max_bands = 1;
    bool alloc_ok = true, offsets_ok = true;
    for (auto& sp : active) {
      DStream& s = *sp;
      if (s.sel.empty()) continue;
      size_t m = 0, mh = 0, sl = 0, ents = 0, bytes = 0, shown = 0;
      for (auto& f : s.sel) { m += (size_t)f->mb_w * f->mb_h; if (!s.dev_at.count (f.get())) mh += (size_t)f->mb_w * f->mb_h; sl += f->slices.size(); ents += f->sparse_coeffs.size(); if (!f->frozen) { int ow, oh; delivered (s, *f, &ow, &oh); bytes += colour ? (size_t)ow * oh * 3 * es : (size_t)ow * oh * 3 / 2; shown++; } }
      if (!rd.chains.empty() && n_mbs + m > group_mbs) { unselect (s); continue; }
      const FrameOut& f0 = *s.sel[0];
      if (f0.mb_w != s.geo.mb_w || f0.mb_h != s.geo.mb_h) {
        release_pool (s);                           // (the kernels that still read the old pictures are in front of whatever takes them next)
        s.geo.mb_w = f0.mb_w; s.geo.mb_h = f0.mb_h;
        s.geo.bytes = (lh264_pic_bytes (f0.mb_w, f0.mb_h, &s.geo.stride_y, &s.geo.stride_c, &s.geo.off[0], &s.geo.off[1], &s.geo.off[2]) + 255) & ~ (size_t)255;
      }
      RoundChain c;
      c.s = &s; c.first_picture = (int)s.delivered; c.at = rd.out_bytes; c.bytes = bytes; c.n_out = shown; c.dig0 = n_out;
      n_out += shown;
      if (fields) {
        size_t shown_mbs = 0;
        for (auto& f : s.sel) if (!f->frozen) { shown_mbs += (size_t)f->mb_w * f->mb_h; max_units = std::max (max_units, f->mb_h * lh264pack::motion_chunks (f->mb_w)); }
        c.mjob0 = n_mjobs; n_mjobs += shown;
        c.mot_at = rd.mot_bytes; c.mot_bytes = shown_mbs * 96; rd.mot_bytes += (c.mot_bytes + 15) & ~ (size_t)15;
        c.mbi_at = rd.mbi_bytes; c.mbi_bytes = shown_mbs * 8; rd.mbi_bytes += (c.mbi_bytes + 15) & ~ (size_t)15;
      }
      place.push_back ({n_hmbs, n_sl, n_sp, n_jobs});
      n_mbs += m; n_hmbs += mh; n_sl += sl; n_sp += ents; n_jobs += s.sel.size();
      // a float type: every picture, and so every row, begins at a multiple of 4 bytes - the chain at one of 16, a picture 3*ow*oh*es
      // bytes behind the one before (decode_pack_sample_kernel stores nothing narrower)
      if (stype) for (auto& f : s.sel) if (!f->frozen) { int ow, oh; delivered (s, *f, &ow, &oh); if (((size_t)ow * oh * 3 * es | rd.out_bytes) & 3) offsets_ok = false; }
      rd.out_bytes += (bytes + 15) & ~ (size_t)15;
      max_w = std::max (max_w, f0.mb_w); max_h = std::max (max_h, f0.mb_h);
      rd.chains.push_back (std::move (c));
    }
    if (rd.chains.empty()) {
      // nothing to reconstruct (streams that ended without a picture): the round on the device is still owed
      deliver (rounds[rb ^ 1], rb ^ 1);
      continue;
    }
    const int n_chains = (int)rd.chains.size();
    // the chains of the launch: a stream's pictures of the round one behind the other - or, with opts->pick, every picture on its own:
    // it references nothing, so the stream spreads over as many workgroups as it has pictures in the round.  (Delivery and the
    // stream's digest follow rd.chains, the streams, in both cases)
    const int n_launch = picking ? (int)n_jobs : n_chains;
    alloc_ok = A.d_mbs.alloc (n_hmbs * sizeof (lh264_mb_t)) && (motion_only || (A.d_coef.alloc (n_hmbs * 768) && A.d_sparse.alloc (n_sp * 8))) && A.d_sl.alloc (n_sl * sizeof (lh264_slice_t)) &&
               A.d_jobs.alloc (n_jobs * sizeof (lh264_frame_job_t)) && A.d_first.alloc ((size_t) (n_launch + 1) * 4) && A.d_pack.alloc (n_jobs * sizeof (lh264_pack_job_t)) &&
               (motion_only || A.d_out[rb].alloc (rd.out_bytes)) && (device_out || no_pictures || A.h_out[rb].alloc (rd.out_bytes)) &&
               A.h_mbs[rb].alloc (n_hmbs * sizeof (lh264_mb_t)) && A.h_sparse[rb].alloc (n_sp * 8) && A.h_sl[rb].alloc (n_sl * sizeof (lh264_slice_t)) &&
               A.h_jobs[rb].alloc (n_jobs * sizeof (lh264_frame_job_t)) && A.h_first[rb].alloc ((size_t) (n_launch + 1) * 4) && A.h_pack[rb].alloc (n_jobs * sizeof (lh264_pack_job_t)) &&
               (!colour || (A.d_std.alloc (n_jobs) && A.h_std[rb].alloc (n_jobs))) &&
               (!placed || (A.d_place.alloc (n_jobs * sizeof (lh264_pack_place_t)) && A.h_place[rb].alloc (n_jobs * sizeof (lh264_pack_place_t))));
    if (fields) alloc_ok = alloc_ok && A.d_mjobs.alloc (n_mjobs * sizeof (lh264_motion_job_t)) && A.h_mjobs[rb].alloc (n_mjobs * sizeof (lh264_motion_job_t)) &&
                             A.d_mot[rb].alloc (rd.mot_bytes) && A.d_mbi[rb].alloc (rd.mbi_bytes) && (device_out || (A.h_mot[rb].alloc (rd.mot_bytes) && A.h_mbi[rb].alloc (rd.mbi_bytes)));
    for (int k = 0; k < 2 && fields && alloc_ok; k++) if (!A.e_mot[rb][k]) alloc_ok = hipEventCreate (&A.e_mot[rb][k]) == hipSuccess;
    const size_t n_sjobs = (sha_pics ? n_out : 0) + (sha_stream ? (size_t)n_chains : 0);
    rd.dig_states_at = (n_out * 20 + 15) & ~ (size_t)15;
    const size_t dig_bytes = rd.dig_states_at + (size_t)n_chains * sizeof (lh264_sha1_state_t);
    if (sha) alloc_ok = alloc_ok && A.d_sjobs.alloc (n_sjobs * sizeof (lh264_sha1_job_t)) && A.h_sjobs[rb].alloc (n_sjobs * sizeof (lh264_sha1_job_t)) && A.d_dig.alloc (dig_bytes) &&
                          A.h_dig[rb].alloc (dig_bytes) && A.d_rec.alloc (n_out * sizeof (lh264_sha1_state_t)) && A.d_state.alloc ((size_t)n * sizeof (lh264_sha1_state_t));
    // picture slots (serial: the cache is shared).  A picture takes a slot that was free when the round began; a slot becomes free
    // behind the round when its picture is in no DPB any more - the round's pictures are all packed by then
    std::vector<std::vector<int>> slot_of (n_chains);
    for (int c = 0; c < n_chains && alloc_ok && offsets_ok && !motion_only; c++) {
      DStream& s = *rd.chains[c].s;
      s.grey = A.pics.grey (s.geo.bytes, A.s_run);
      if (!s.grey) { alloc_ok = false; break; }
      for (auto& f : s.sel) {
        int at = -1;
        for (size_t q = 0; q < s.pool.size(); q++) if (s.pool[q].pic_id < 0) { at = (int)q; break; }
        if (at < 0) {
          uint8_t* p = A.pics.get (s.geo.bytes, A.s_run);
          if (!p) { alloc_ok = false; break; }
          s.pool.push_back ({p, -1});
          at = (int)s.pool.size() - 1;
        }
        s.pool[at].pic_id = f->id;
        slot_of[c].push_back (at);
      }
    }
    if (!alloc_ok || !offsets_ok) { fail_device (offsets_ok ? "device allocation failed" : "a float picture would not begin at a multiple of 4 bytes"); for (auto& s : active) s->sel.clear(); deliver (rounds[rb ^ 1], rb ^ 1); continue; }
    // ---- staging (host threads): records to the page-locked buffers, the job tables
    lh264_mb_t* h_mbs = A.h_mbs[rb].as<lh264_mb_t>(); uint64_t* h_sparse = A.h_sparse[rb].as<uint64_t>(); lh264_slice_t* h_sl = A.h_sl[rb].as<lh264_slice_t>();
    lh264_frame_job_t* h_jobs = A.h_jobs[rb].as<lh264_frame_job_t>(); int32_t* h_first = A.h_first[rb].as<int32_t>(); lh264_pack_job_t* h_pack = A.h_pack[rb].as<lh264_pack_job_t>();
    uint8_t* h_std = colour ? A.h_std[rb].as<uint8_t>() : nullptr;
    lh264_pack_place_t* h_place = placed ? A.h_place[rb].as<lh264_pack_place_t>() : nullptr;
    uint8_t* const d_out = A.d_out[rb].as<uint8_t>();
    lh264_motion_job_t* h_mjobs = fields ? A.h_mjobs[rb].as<lh264_motion_job_t>() : nullptr;
    run_parallel (n_chains, threads, [&] (int c) {
      RoundChain& rc = rd.chains[c];
      DStream& s = *rc.s;
      size_t mo = place[c].mb0, so = place[c].sl0, po = place[c].sp0, j = place[c].job0, at = rc.at;
      if (!picking) h_first[c] = (int32_t)j;
      uint64_t off = s.out_off;
      for (size_t q = 0; q < s.sel.size(); q++) {
        FrameOut& f = *s.sel[q];
        const size_t nm = (size_t)f.mb_w * f.mb_h;
        const auto dev_it = s.dev_at.find (&f);                  // the picture's records and coefficients lie in the parse arena
        const bool on_dev = dev_it != s.dev_at.end();
        if (!on_dev) memcpy (&h_mbs[mo], f.mbs.data(), nm * sizeof (lh264_mb_t));
        memcpy (&h_sl[so], f.slices.data(), f.slices.size() * sizeof (lh264_slice_t));
        if (!motion_only) { const uint64_t add = (uint64_t) (mo * 384) << 16; const size_t ns = f.sparse_coeffs.size(); for (size_t e = 0; e < ns; e++) h_sparse[po + e] = f.sparse_coeffs[e] + add; po += ns; }
        const Slot me = motion_only ? Slot {nullptr, -1} : s.pool[slot_of[c][q]];
        auto pic_at = [&] (const uint8_t* base) { lh264_pic_t p; p.y_dev = (uint8_t*)base + s.geo.off[0]; p.u_dev = (uint8_t*)base + s.geo.off[1]; p.v_dev = (uint8_t*)base + s.geo.off[2]; return p; };
        lh264_frame_job_t& jb = h_jobs[j];
        memset (&jb, 0, sizeof (jb));
        jb.mbs_dev = on_dev ? A.d_pmbs.as<lh264_mb_t>() + dev_it->second.mb : A.d_mbs.as<lh264_mb_t>() + mo;
        jb.coeffs_dev = on_dev ? A.d_pcoef.as<int16_t>() + dev_it->second.mb * 384 : A.d_coef.as<int16_t>() + mo * 384; jb.slices_dev = A.d_sl.as<lh264_slice_t>() + so;
        if (!motion_only) jb.dst = pic_at (me.base);
        // fields: back[slot], how many pictures back the picture behind job reference `slot` lies (-1: none, or one no longer held)
        int16_t back[LH264_MAX_REFS];
        if (fields) {
          for (size_t k = 0; k < LH264_MAX_REFS; k++) {
            back[k] = -1;
            if (picking || k >= f.ref_ids.size() || f.ref_ids[k] == f.id) continue;
            const auto it = s.held.find (f.ref_ids[k]);
            if (it != s.held.end() && f.index - it->second <= 32767) back[k] = (int16_t) (f.index - it->second);
          }
          s.held[f.id] = f.index;
        }
        for (size_t k = 0; k < LH264_MAX_REFS && !motion_only; k++) {
          // A slot the picture does not fill, or whose picture is not held, points at the 128 picture.  recon_chain_kernel reads job slot
          // 0 for a partition whose slice has no reference list entry (a P picture whose references are lost); the oracle predicts nothing
          // there and leaves its fresh picture's 128: the same samples.  The picture itself in that slot (what the ISVC object does) would
          // be read while it is being written, in wavefront order: not the oracle's result, and not a defined one.
          const uint8_t* base = s.grey;
          if (!picking && k < f.ref_ids.size()) for (const Slot& sl : s.pool) if (sl.pic_id == f.ref_ids[k] && sl.base != me.base) { base = sl.base; break; }
          jb.ref[k] = pic_at (base);
        }
        jb.mb_w = f.mb_w; jb.mb_h = f.mb_h; jb.stride_y = s.geo.stride_y; jb.stride_c = s.geo.stride_c;
        jb.n_slices = (int32_t)f.slices.size();
        jb.flags = f.is_ref && !picking ? 0 : LH264_JOB_NO_EXPAND;      // (opts->pick: nothing will read the picture's borders)
        lh264_pack_job_t& pj = h_pack[j];
        memset (&pj, 0, sizeof (pj));
        if (placed) memset (&h_place[j], 0, sizeof (lh264_pack_place_t));
        pj.reserved = scale;
        const uint8_t std_byte = colour ? picture_standard (f, ext_matrix, ext_range) : 0;      // (a picture select() let through: its standard is defined)
        if (colour) h_std[j] = std_byte & 3;
        if (f.frozen) { if (!on_dev) mo += nm; so += f.slices.size(); j++; continue; }      // withheld: a reference like any other, but no window to pack (crop_h 0)
        pj.y = jb.dst.y_dev; pj.u = jb.dst.u_dev; pj.v = jb.dst.v_dev;
        pj.dst = d_out + at;
        pj.stride_y = s.geo.stride_y; pj.stride_c = s.geo.stride_c;
        // the picture's view: the source rectangle takes the window's place in the job, the destination goes to the job's place
        lh264_rect_t vs, vd;
        int ow, oh;                                                                         // what is delivered
        view_of (f.crop_w, f.crop_h, crops[s.i], fit, scale, out_w, out_h, &vs, &vd, &ow, &oh);
        pj.crop_x = f.crop_x + vs.x; pj.crop_y = f.crop_y + vs.y; pj.crop_w = vs.w; pj.crop_h = vs.h; pj.format = format;
        if (placed) { h_place[j].x = vd.x; h_place[j].y = vd.y; h_place[j].w = vd.w; h_place[j].h = vd.h; h_place[j].fill = fill; }
        for (const lh264_rect_t* r : {&vs, &vd}) { rc.view.push_back (r->x); rc.view.push_back (r->y); rc.view.push_back (r->w); rc.view.push_back (r->h); }
        const size_t bytes = colour ? (size_t)ow * oh * 3 * es : (size_t)ow * oh * 3 / 2;
        lh264_decoded_pic_t dp;
        dp.width = ow; dp.height = oh; dp.frame_num = f.frame_num; dp.idr = f.idr ? 1 : 0; dp.offset = off; dp.bytes = bytes;
        rc.pics.push_back (dp);
        rc.concealed.push_back (f.concealed);
        rc.source_wh.push_back (f.crop_w); rc.source_wh.push_back (f.crop_h);
        rc.index.push_back ((int32_t)f.index);
        if (colour) rc.colour.push_back (std_byte);
        if (fields) {
          size_t mot_off = 0, mbi_off = 0;
          for (const lh264_decoded_motion_t& g : rc.motion_geo) { mot_off += (size_t)g.mb_w * g.mb_h * 96; mbi_off += (size_t)g.mb_w * g.mb_h * 8; }
          lh264_motion_job_t& mj = h_mjobs[rc.mjob0 + rc.motion_geo.size()];
          memset (&mj, 0, sizeof (mj));
          mj.mbs = jb.mbs_dev; mj.slices = jb.slices_dev;
          mj.motion = (int16_t*) (A.d_mot[rb].as<uint8_t>() + rc.mot_at + mot_off); mj.info = A.d_mbi[rb].as<uint8_t>() + rc.mbi_at + mbi_off;
          mj.mb_w = f.mb_w; mj.mb_h = f.mb_h; mj.n_slices = (int32_t)f.slices.size();
          memcpy (mj.back, back, sizeof (back));
          rc.motion_geo.push_back ({f.mb_w, f.mb_h, f.crop_x, f.crop_y, s.mot_off + mot_off, s.mbi_off + mbi_off});
        }
        at += bytes; off += bytes;
        if (!on_dev) mo += nm;
        so += f.slices.size(); j++;
      }
    });
    if (picking) for (size_t j = 0; j < n_jobs; j++) h_first[j] = (int32_t)j;
    h_first[n_launch] = (int32_t)n_jobs;
    if (sha) {
      // the span jobs: a picture is a message of its own (its record is scratch), a chain's bytes are the next span of its stream's
      // message, whose record stays on the device from round to round; a copy of it comes down with the round
      lh264_sha1_job_t* sj = A.h_sjobs[rb].as<lh264_sha1_job_t>();
      size_t q = 0;
      for (int c = 0; c < n_chains; c++) {
        RoundChain& rc = rd.chains[c];
        size_t at = rc.at;
        if (sha_pics) for (size_t k = 0; k < rc.pics.size(); k++) {
          sj[q++] = {d_out + at, rc.pics[k].bytes, A.d_rec.as<lh264_sha1_state_t>() + rc.dig0 + k, A.d_dig.as<uint8_t>() + (rc.dig0 + k) * 20, LH264_SHA1_FRESH | LH264_SHA1_FINAL, 0};
          at += rc.pics[k].bytes;
        }
        if (sha_stream) {
          sj[q++] = {d_out + rc.at, rc.bytes, A.d_state.as<lh264_sha1_state_t>() + rc.s->i, A.d_dig.as<uint8_t>() + rd.dig_states_at + (size_t)c * sizeof (lh264_sha1_state_t), rc.s->sha_started ? 0u : (uint32_t)LH264_SHA1_FRESH, 0};
          rc.s->sha_started = true;
        }
      }
      std::stable_sort (sj, sj + q, [] (const lh264_sha1_job_t& a, const lh264_sha1_job_t& b) { return a.len > b.len; });
    }
    for (int c = 0; c < n_chains; c++) {
      DStream& s = *rd.chains[c].s;
      for (auto& f : s.sel) { int ow, oh; delivered (s, *f, &ow, &oh); max_bands = std::max (max_bands, (oh + lh264pack::kBandRows - 1) / lh264pack::kBandRows); }
      // the slots the round leaves free: pictures the DPB behind the round's last picture does not hold
      const std::vector<int>& dpb = s.sel.back()->dpb_ids;
      for (Slot& sl : s.pool) if (sl.pic_id >= 0 && (picking || std::find (dpb.begin(), dpb.end(), sl.pic_id) == dpb.end())) sl.pic_id = -1;      // (opts->pick: a slot is needed for its round only)
      s.next_picture += (long)s.sel.size();
      s.delivered += (long)rd.chains[c].pics.size();
      s.out_off += rd.chains[c].bytes;
      s.mot_off += rd.chains[c].mot_bytes; s.mbi_off += rd.chains[c].mbi_bytes;
      // (fields: the pictures whose slots are free now are no reference any more)
      if (fields) for (auto it = s.held.begin(); it != s.held.end(); ) { if (picking || std::find (dpb.begin(), dpb.end(), it->first) == dpb.end()) it = s.held.erase (it); else ++it; }
      s.sel.clear();                                  // the pictures' records are staged: their memory goes back
    }
    const double t_c = now_s();
    t_stage += t_c - t_b;
    // ---- the device stage, asynchronous: upload, clear + expand the coefficients, reconstruct, pack; the download behind an event
    {
      hipStream_t st = A.s_run;
      auto up = [&] (DevBuf& d, const void* s, size_t bytes) { return bytes == 0 || hipMemcpyAsync (d.p, s, bytes, hipMemcpyHostToDevice, st) == hipSuccess; };
      // (motion only: the records and the slice tables are all the gather reads)
      bool ok = motion_only ? up (A.d_mbs, h_mbs, n_hmbs * sizeof (lh264_mb_t)) && up (A.d_sl, h_sl, n_sl * sizeof (lh264_slice_t)) :
                up (A.d_mbs, h_mbs, n_hmbs * sizeof (lh264_mb_t)) && up (A.d_sparse, h_sparse, n_sp * 8) && up (A.d_sl, h_sl, n_sl * sizeof (lh264_slice_t)) &&
                up (A.d_jobs, h_jobs, n_jobs * sizeof (lh264_frame_job_t)) && up (A.d_first, h_first, (size_t) (n_launch + 1) * 4) && up (A.d_pack, h_pack, n_jobs * sizeof (lh264_pack_job_t)) && (!colour || up (A.d_std, h_std, n_jobs)) && (!placed || up (A.d_place, h_place, n_jobs * sizeof (lh264_pack_place_t))) &&
                (n_hmbs == 0 || hipMemsetAsync (A.d_coef.p, 0, n_hmbs * 768, st) == hipSuccess);
      // the fields need the records only: the gather goes in front of the reconstruct launch
      if (ok && n_mjobs) {
        ok = up (A.d_mjobs, h_mjobs, n_mjobs * sizeof (lh264_motion_job_t)) && hipEventRecord (A.e_mot[rb][0], st) == hipSuccess;
        if (ok) {
          hipLaunchKernelGGL (decode_pack_motion_kernel, dim3 ((unsigned)n_mjobs, (unsigned)max_units), dim3 (256), 0, st, A.d_mjobs.as<lh264_motion_job_t>());
          ok = hipGetLastError() == hipSuccess && hipEventRecord (A.e_mot[rb][1], st) == hipSuccess;
          rd.timed = ok;
        }
      }
      if (ok && n_sp && !motion_only) { lh264host::expand_sparse (A.d_sparse.as<uint64_t>(), n_sp, A.d_coef.as<int16_t>(), st); ok = hipGetLastError() == hipSuccess; }
      if (ok && !motion_only) ok = lh264_recon_chains (A.d_jobs.as<lh264_frame_job_t>(), A.d_first.as<int32_t>(), n_launch, max_w, max_h, st) == LH264_OK;
      if (ok && !motion_only) { n_rounds++; n_launched += n_launch; n_launched_jobs += (long long)n_jobs; }
      if (ok && !motion_only) {
        if (placed) {
          const lh264_pack_place_t* d_place = A.d_place.as<lh264_pack_place_t>();
          if (stype) hipLaunchKernelGGL (decode_pack_sample_placed_kernel, dim3 ((unsigned)n_jobs, (unsigned)max_bands), dim3 (256), 0, st, A.d_pack.as<lh264_pack_job_t>(), d_place, A.d_std.as<uint8_t>(), out_w, out_h, colour, sample_arg);
          else if (colour) hipLaunchKernelGGL (decode_pack_rgb_placed_kernel, dim3 ((unsigned)n_jobs, (unsigned)max_bands), dim3 (256), 0, st, A.d_pack.as<lh264_pack_job_t>(), d_place, A.d_std.as<uint8_t>(), out_w, out_h, colour);
          else hipLaunchKernelGGL (decode_pack_placed_kernel, dim3 ((unsigned)n_jobs, (unsigned)max_bands), dim3 (256), 0, st, A.d_pack.as<lh264_pack_job_t>(), d_place, out_w, out_h);
        }
        else if (stype) hipLaunchKernelGGL (decode_pack_sample_kernel, dim3 ((unsigned)n_jobs, (unsigned)max_bands), dim3 (256), 0, st, A.d_pack.as<lh264_pack_job_t>(), A.d_std.as<uint8_t>(), out_w, out_h, colour, sample_arg);
        else if (colour) hipLaunchKernelGGL (decode_pack_rgb_kernel, dim3 ((unsigned)n_jobs, (unsigned)max_bands), dim3 (256), 0, st, A.d_pack.as<lh264_pack_job_t>(), A.d_std.as<uint8_t>(), out_w, out_h, colour);
        else if (out_w) hipLaunchKernelGGL (decode_pack_resized_kernel, dim3 ((unsigned)n_jobs, (unsigned)max_bands), dim3 (256), 0, st, A.d_pack.as<lh264_pack_job_t>(), out_w, out_h);
        else if (scale) hipLaunchKernelGGL (decode_pack_scaled_kernel, dim3 ((unsigned)n_jobs, (unsigned)max_bands), dim3 (256), 0, st, A.d_pack.as<lh264_pack_job_t>());
        else hipLaunchKernelGGL (decode_pack_kernel, dim3 ((unsigned)n_jobs, (unsigned)max_bands), dim3 (256), 0, st, A.d_pack.as<lh264_pack_job_t>());
        ok = hipGetLastError() == hipSuccess;
      }
      if (ok && sha) {
        ok = up (A.d_sjobs, A.h_sjobs[rb].p, n_sjobs * sizeof (lh264_sha1_job_t));
        if (ok && n_sjobs) { hipLaunchKernelGGL (sha1_spans_kernel, dim3 ((unsigned) ((n_sjobs + 63) / 64)), dim3 (64), 0, st, A.d_sjobs.as<lh264_sha1_job_t>(), (int)n_sjobs); ok = hipGetLastError() == hipSuccess; }
        ok = ok && hipMemcpyAsync (A.h_dig[rb].p, A.d_dig.p, dig_bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
      }
      // bytes that stay on the device go behind what the handle holds (the buffer grows by doubling)
      auto keep_dev = [&] (uint8_t*& dev, size_t& dev_len, size_t& dev_cap, const uint8_t* src, size_t bytes) {
        if (dev_len + bytes > dev_cap) {
          const size_t cap = std::max<size_t> (4 * (dev_len + bytes), (size_t)1 << 16);
          uint8_t* p = nullptr;
          if (hipMalloc ((void**)&p, cap) != hipSuccess) return false;
          if (dev_len && hipMemcpyAsync (p, dev, dev_len, hipMemcpyDeviceToDevice, st) != hipSuccess) { hipFree (p); return false; }
          if (dev) { hipStreamSynchronize (st); hipFree (dev); }
          dev = p; dev_cap = cap;
        }
        if (hipMemcpyAsync (dev + dev_len, src, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
        dev_len += bytes;
        return true;
      };
      if (ok && device_out && fields) for (RoundChain& c : rd.chains) {
        lh264_decoded_t& r = *out[c.s->i];
        if (!c.mot_bytes) continue;
        if (!keep_dev (r.mot_dev, r.mot_len, r.mot_cap, A.d_mot[rb].as<uint8_t>() + c.mot_at, c.mot_bytes) ||
            !keep_dev (r.mbi_dev, r.mbi_len, r.mbi_cap, A.d_mbi[rb].as<uint8_t>() + c.mbi_at, c.mbi_bytes)) { ok = false; break; }
      }
      if (ok && device_out && !no_pictures) {
        // the pictures stay on the device: every stream's run goes behind what its handle holds
        for (RoundChain& c : rd.chains) {
          lh264_decoded_t& r = *out[c.s->i];
          if (!c.bytes) continue;                   // (every picture of the chain withheld)
          if (!keep_dev (r.dev, r.dev_len, r.dev_cap, d_out + c.at, c.bytes)) { ok = false; break; }
        }
      }
      ok = ok && hipEventRecord (A.e_run[rb], st) == hipSuccess;
      if (ok && down) ok = hipStreamWaitEvent (A.s_down, A.e_run[rb], 0) == hipSuccess &&
                                  (no_pictures || !rd.out_bytes || hipMemcpyAsync (A.h_out[rb].p, d_out, rd.out_bytes, hipMemcpyDeviceToHost, A.s_down) == hipSuccess) &&
                                  (!fields || !rd.mot_bytes || (hipMemcpyAsync (A.h_mot[rb].p, A.d_mot[rb].p, rd.mot_bytes, hipMemcpyDeviceToHost, A.s_down) == hipSuccess &&
                                                                hipMemcpyAsync (A.h_mbi[rb].p, A.d_mbi[rb].p, rd.mbi_bytes, hipMemcpyDeviceToHost, A.s_down) == hipSuccess)) &&
                                  hipEventRecord (A.e_down[rb], A.s_down) == hipSuccess;
      if (!ok) { const char* le = lh264_last_error(); fail_device (std::string ("launching the device stage failed") + (le && *le ? std::string (": ") + le : std::string())); for (RoundChain& c : rd.chains) c.s->stopped = true; }
      else rd.live = true;
    }
    t_enqueue += now_s() - t_c;
    // ---- the round before: its bytes arrive while this one reconstructs
    deliver (rounds[rb ^ 1], rb ^ 1);
    rb ^= 1;
  }
  deliver (rounds[0], 0);
  deliver (rounds[1], 1);
  hipStreamSynchronize (A.s_run);
  hipStreamSynchronize (A.s_down);
  for (auto& s : active) finish (*s);
  active.clear(); retired.clear();
  if (sha_stream) for (int i = 0; i < n; i++) { lh264_sha1_state_t fin = out[i]->stream_state; lh264sha1::finish (&fin, out[i]->stream_sha); }
  // (streams that were complete before a failure of the device stage keep their result; the others carry the error)
  if (device_failed) for (int i = next_stream; i < n; i++) { out[i]->status = LH264_E_HIP; out[i]->error = device_error; }
  g_timing[0] = (now_s() - t_call) * 1e3; g_timing[1] = t_parse * 1e3; g_timing[2] = t_stage * 1e3; g_timing[3] = t_enqueue * 1e3; g_timing[4] = t_wait * 1e3; g_timing[5] = t_deliver * 1e3;
  g_parse_timing[0] = t_dev_parse * 1e3; g_parse_timing[1] = n_dev_slices;
  g_motion_ms = motion_ms; g_motion_bytes = motion_bytes;
  g_chains[0] = n_rounds; g_chains[1] = n_launched; g_chains[2] = n_launched_jobs;
  if (trace_on()) fprintf (stderr, "[lh264 decode] %d streams: %.3f s (parse %.3f, staging %.3f, enqueue %.3f, waiting for the device %.3f, delivery %.3f); arena %.1f MB device, %.1f MB pinned\n",
                           n, g_timing[0] / 1e3, t_parse, t_stage, t_enqueue, t_wait, t_deliver, A.device_bytes() / 1e6, A.pinned_bytes() / 1e6);
  return LH264_OK;
}

int lh264_decode_last_timing (double* ms) {
  if (!ms) return LH264_E_ARG;
  for (int k = 0; k < 6; k++) ms[k] = g_timing[k];
  return LH264_OK;
}
int lh264_decode_last_parse_timing (double* out) {
  if (!out) return LH264_E_ARG;
  out[0] = g_parse_timing[0]; out[1] = g_parse_timing[1];
  return LH264_OK;
}
int lh264_decode_last_chains (long long v[3]) {
  if (!v) return LH264_E_ARG;
  for (int k = 0; k < 3; k++) v[k] = g_chains[k];
  return LH264_OK;
}
// the header walk of lh264_decode_batch under opts->pick, and its choice: every slice deferred, none resolved
int lh264_parser_pick (const uint8_t* data, size_t len, uint32_t pick, int32_t* idx, int cap, int* n) {
  if (!n || cap < 0 || (cap && !idx) || pick > LH264_PICK_IDR || (!data && len)) return LH264_E_ARG;
  Parser P;
  P.set_sparse_coeffs (true); P.set_sparse_levels (true);
  P.set_defer_slice_data (true); P.set_defer_cabac (true);
  P.begin_file (data, data ? len : 0);
  int count = 0;
  while (!P.file_finished()) {
    P.feed_file_some (0);
    const long limit = P.error().empty() ? 0x7fffffffffffffffl : P.error_pictures();
    for (auto& f : P.frames()) if (f->index < limit && picture_selected (*f, pick)) { if (count < cap) idx[count] = (int32_t)f->index; count++; }
    P.frames().clear();
  }
  *n = count;
  return LH264_OK;
}
int lh264_parser_colour (const uint8_t* data, size_t len, int32_t* matrix_coefficients, int32_t* full_range, int32_t* present) {
  if (!data) return LH264_E_ARG;
  int mc = 2, fr = 0, pr = 0;
  if (!Parser::first_sps_colour (data, len, &mc, &fr, &pr)) return LH264_E_UNSUPPORTED;
  if (matrix_coefficients) *matrix_coefficients = mc;
  if (full_range) *full_range = fr;
  if (present) *present = pr;
  return LH264_OK;
}
int lh264_decoded_picture_colour (const lh264_decoded_t* d, int idx, uint32_t* matrix, int32_t* full_range) {
  if (!d || idx < 0 || (size_t)idx >= d->pics.size() || d->colour.size() != d->pics.size()) return LH264_E_ARG;
  if (matrix) *matrix = (d->colour[idx] & 1) ? LH264_MATRIX_BT709 : LH264_MATRIX_BT601;
  if (full_range) *full_range = d->colour[idx] >> 1 & 1;
  return LH264_OK;
}
int lh264_decoded_sample_type (const lh264_decoded_t* d) { return d ? d->sample_type : LH264_E_ARG; }
long long lh264_decoded_parsed_slices (const lh264_decoded_t* d) { return d ? (long long)d->parsed_slices : 0; }
int lh264_decoded_picture_index (const lh264_decoded_t* d, int idx) {
  if (!d || idx < 0 || (size_t)idx >= d->pics.size() || d->index.size() != d->pics.size()) return LH264_E_ARG;
  return d->index[idx];
}
int lh264_decoded_status (const lh264_decoded_t* d) { return d ? d->status : LH264_E_ARG; }
int lh264_decoded_parse_path (const lh264_decoded_t* d) { return d ? d->parse_path : LH264_E_ARG; }
long long lh264_decoded_device_slices (const lh264_decoded_t* d) { return d ? (long long)d->device_slices : 0; }
long long lh264_decoded_device_cabac_slices (const lh264_decoded_t* d) { return d ? (long long)d->device_cabac_slices : 0; }
const char* lh264_decoded_error (const lh264_decoded_t* d) { return d ? d->error.c_str() : ""; }
int lh264_decoded_pictures (const lh264_decoded_t* d) { return d ? (int)d->pics.size() : 0; }
int lh264_decoded_picture (const lh264_decoded_t* d, int idx, lh264_decoded_pic_t* o) {
  if (!d || !o || idx < 0 || (size_t)idx >= d->pics.size()) return LH264_E_ARG;
  *o = d->pics[idx];
  return LH264_OK;
}
const uint8_t* lh264_decoded_bytes (const lh264_decoded_t* d, size_t* len) {
  if (len) *len = d ? d->bytes.size() : 0;
  return d && !d->bytes.empty() ? d->bytes.data() : nullptr;
}
const uint8_t* lh264_decoded_bytes_dev (const lh264_decoded_t* d, size_t* len) {
  if (len) *len = d ? d->dev_len : 0;
  return d ? d->dev : nullptr;
}
int lh264_decoded_copy_dev (const lh264_decoded_t* d, void* dst_dev, size_t cap) {
  if (!d || !dst_dev || cap < d->dev_len) return LH264_E_ARG;
  if (d->dev_len && hipMemcpy (dst_dev, d->dev, d->dev_len, hipMemcpyDeviceToDevice) != hipSuccess) return LH264_E_HIP;
  return LH264_OK;
}
int lh264_decoded_picture_sha1 (const lh264_decoded_t* d, int idx, uint8_t out[20]) {
  if (!d || !out) return LH264_E_ARG;
  if (d->status == LH264_E_HIP) return d->status;
  if (!(d->sha & LH264_DECODE_SHA1_PICTURES) || idx < 0 || (size_t)idx >= d->pics.size() || d->pic_sha.size() != d->pics.size() * 20) return LH264_E_ARG;
  memcpy (out, &d->pic_sha[(size_t)idx * 20], 20);
  return LH264_OK;
}
int lh264_decoded_stream_sha1 (const lh264_decoded_t* d, uint8_t out[20]) {
  if (!d || !out) return LH264_E_ARG;
  if (d->status == LH264_E_HIP) return d->status;
  if (!(d->sha & LH264_DECODE_SHA1_STREAM)) return LH264_E_ARG;
  memcpy (out, d->stream_sha, 20);
  return LH264_OK;
}
int lh264_decoded_picture_source_size (const lh264_decoded_t* d, int idx, int32_t* width, int32_t* height) {
  if (!d || idx < 0 || (size_t)idx >= d->pics.size() || d->source_wh.size() != d->pics.size() * 2) return LH264_E_ARG;
  if (width) *width = d->source_wh[(size_t)idx * 2];
  if (height) *height = d->source_wh[(size_t)idx * 2 + 1];
  return LH264_OK;
}
int lh264_decoded_picture_view (const lh264_decoded_t* d, int idx, lh264_rect_t* src, lh264_rect_t* dst) {
  if (!d || idx < 0 || (size_t)idx >= d->pics.size() || d->view.size() != d->pics.size() * 8) return LH264_E_ARG;
  const int32_t* v = &d->view[(size_t)idx * 8];
  if (src) *src = {v[0], v[1], v[2], v[3]};
  if (dst) *dst = {v[4], v[5], v[6], v[7]};
  return LH264_OK;
}
int lh264_view_rects (int32_t w, int32_t h, const lh264_rect_t* crop, uint32_t fit, int32_t out_w, int32_t out_h, lh264_rect_t* src, lh264_rect_t* dst) {
  if (w < 2 || h < 2 || w > 16384 || h > 16384 || ((w | h) & 1) || fit > LH264_FIT_CONTAIN) return LH264_E_ARG;
  if ((out_w || out_h) ? !lh264pack::size_ok (out_w, out_h) : fit != LH264_FIT_STRETCH) return LH264_E_ARG;
  const lh264_rect_t c = crop ? *crop : lh264_rect_t {0, 0, 0, 0};
  if (!crop_ok (c) || (c.w && !crop_fits (c, w, h))) return LH264_E_ARG;
  lh264_rect_t vs, vd;
  int ow, oh;
  view_of (w, h, c, fit, 0, out_w, out_h, &vs, &vd, &ow, &oh);
  if (src) *src = vs;
  if (dst) *dst = vd;
  return LH264_OK;
}
int lh264_parser_window (const uint8_t* data, size_t len, int32_t* width, int32_t* height) {
  if (!data) return LH264_E_ARG;
  int w = 0, h = 0;
  if (!Parser::first_sps_window (data, len, &w, &h)) return LH264_E_UNSUPPORTED;
  if (width) *width = w;
  if (height) *height = h;
  return LH264_OK;
}
int lh264_decoded_picture_motion (const lh264_decoded_t* d, int idx, lh264_decoded_motion_t* o) {
  if (!d || !o || !d->fields || idx < 0 || (size_t)idx >= d->pics.size() || d->motion_geo.size() != d->pics.size()) return LH264_E_ARG;
  *o = d->motion_geo[idx];
  return LH264_OK;
}
int lh264_decoded_motion (const lh264_decoded_t* d, const int16_t** motion, size_t* motion_bytes, const uint8_t** info, size_t* info_bytes) {
  if (!d || !d->fields) return LH264_E_ARG;
  if (motion) *motion = d->mot.empty() ? nullptr : (const int16_t*)d->mot.data();
  if (motion_bytes) *motion_bytes = d->mot.size();
  if (info) *info = d->mbi.empty() ? nullptr : d->mbi.data();
  if (info_bytes) *info_bytes = d->mbi.size();
  return LH264_OK;
}
int lh264_decoded_motion_dev (const lh264_decoded_t* d, const int16_t** motion, size_t* motion_bytes, const uint8_t** info, size_t* info_bytes) {
  if (!d || !d->fields) return LH264_E_ARG;
  if (motion) *motion = (const int16_t*)d->mot_dev;
  if (motion_bytes) *motion_bytes = d->mot_len;
  if (info) *info = d->mbi_dev;
  if (info_bytes) *info_bytes = d->mbi_len;
  return LH264_OK;
}
int lh264_decoded_motion_copy_dev (const lh264_decoded_t* d, void* motion_dst_dev, size_t motion_cap, void* info_dst_dev, size_t info_cap) {
  if (!d || !d->fields || (motion_dst_dev && motion_cap < d->mot_len) || (info_dst_dev && info_cap < d->mbi_len)) return LH264_E_ARG;
  if (motion_dst_dev && d->mot_len && hipMemcpy (motion_dst_dev, d->mot_dev, d->mot_len, hipMemcpyDeviceToDevice) != hipSuccess) return LH264_E_HIP;
  if (info_dst_dev && d->mbi_len && hipMemcpy (info_dst_dev, d->mbi_dev, d->mbi_len, hipMemcpyDeviceToDevice) != hipSuccess) return LH264_E_HIP;
  return LH264_OK;
}
int lh264_decode_last_motion (double* ms, unsigned long long* bytes) {
  if (ms) *ms = g_motion_ms;
  if (bytes) *bytes = g_motion_bytes;
  return LH264_OK;
}
int lh264_decoded_concealed (const lh264_decoded_t* d, int idx) {
  if (!d || idx < 0 || (size_t)idx >= d->pics.size() || d->concealed.size() != d->pics.size()) return LH264_E_ARG;
  return d->concealed[idx];
}
void lh264_decoded_free (lh264_decoded_t* d) { delete d; }
int lh264_decode_arena_bytes (size_t* device, size_t* pinned) {
  const bool ok = lh264_device_count() > 0 && g_arena.read_current ([&] (const Arena* a) {
    if (device) *device = a ? a->device_bytes() : 0;
    if (pinned) *pinned = a ? a->pinned_bytes() : 0;
  });
  return ok ? LH264_OK : LH264_E_NODEVICE;
}
void lh264_decode_release (void) {
  if (lh264_device_count() <= 0) return;
  g_arena.release_all();
}

}
