// lh264_pack.h - what the pack kernels of lh264_decode.hip and the lh264_debug_*_cpu entry points step, host and device from one
// source: crop and pack, scaled means, resampling, colour, float samples, their placed forms, and the gather of the motion fields.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lh264.h"
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
// one axis of a filter table (lh264_decode_batch_ex6: bilinear, bicubic), built on the host and only read here: ent[3 * X] .. [3 * X + 2]
// are the first tap of delivered coordinate X, the number of its taps and where their weights begin in k.  The weights of one X sum to
// 2^14; every tap lies inside the window
struct FilterAxis { const int32_t* ent; const int16_t* k; };
// the four tables of one pack job: luma columns, luma rows, chroma columns, chroma rows
struct FilterJob { FilterAxis lx, ly, cx, cy; };
// one plane as the resize step sees it: the window's first sample, its size, the delivered size (fx, fy: the filtered step's tables)
struct ResizePlane { const uint8_t* p; int stride; uint32_t w, h, ow, oh; FilterAxis fx = {nullptr, nullptr}, fy = {nullptr, nullptr}; };
__host__ __device__ inline uint32_t filtered_sample (const ResizePlane& pl, int X, int Y);      // (behind clip8, below)
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
// k - b0 of plane a (interleaved: sample (k - b0) / 2 of a or b, b0 even); every other byte is fa (k even) or fb (k odd).
// M = 4: the area means; M = 6: the planes' filter tables (filtered_sample)
template <int M = 4>
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
  const Span sy = M == 4 ? span_of ((uint32_t) (Y - y0), a.h, a.oh) : Span();
  uint32_t o = 0;
  for (int k = k0; k < k1; k++) {
    uint8_t v;
    if (k < b0 || k >= b1) v = (uint8_t) ((k & 1) ? fb : fa);
    else if constexpr (M == 4) { const int x = k - b0; v = interleaved ? resized_sample ((x & 1) ? b : a, sy, x >> 1) : resized_sample (a, sy, x); }
    else { const int x = k - b0; v = (uint8_t) (interleaved ? filtered_sample ((x & 1) ? b : a, x >> 1, Y - y0) : filtered_sample (a, x, Y - y0)); }
    if (whole) o |= (uint32_t)v << (8 * (k - k0));
    else d[k] = v;
  }
  if (whole) * (uint32_t*) (d + k0) = o;
}
// band `band` (16 delivered luma rows, 8 chroma rows) of one job delivered as ow x oh with its window placed by pl, worked on by item
// t of nt (the host steps it with t = 0, nt = 1).  M = 6: resampled by the job's filter tables fj
template <int M = 4>
__host__ __device__ inline void pack_band_placed (const lh264_pack_job_t& j, const lh264_pack_place_t& pl, int ow, int oh, int band, int t, int nt, const FilterJob* fj = nullptr) {
  const FilterAxis none = {nullptr, nullptr};
  const int w = j.crop_w, h = j.crop_h, ocw = ow >> 1, och = oh >> 1;
  const uint32_t fy = pl.fill & 0xffu, fcb = pl.fill >> 8 & 0xffu, fcr = pl.fill >> 16 & 0xffu;
  const int r0 = band * kBandRows, r1 = r0 + kBandRows < oh ? r0 + kBandRows : oh;
  if (r1 > r0) {
    const ResizePlane y = {j.y + (size_t)j.crop_y * j.stride_y + j.crop_x, j.stride_y, (uint32_t)w, (uint32_t)h, (uint32_t)pl.w, (uint32_t)pl.h, M == 6 ? fj->lx : none, M == 6 ? fj->ly : none};
    const int pieces = (ow + 6) >> 2, items = (r1 - r0) * pieces;
    for (int it = t; it < items; it += nt) {
      const int r = r0 + it / pieces, p = it % pieces;
      piece_placed<M> (j.dst + (size_t)r * ow, ow, r, p, y, y, false, pl.x, pl.x + pl.w, pl.y, fy, fy);
    }
  }
  const int c0 = band * (kBandRows / 2), c1 = c0 + kBandRows / 2 < och ? c0 + kBandRows / 2 : och;
  if (c1 <= c0) return;
  const size_t co = (size_t) (j.crop_y >> 1) * j.stride_c + (j.crop_x >> 1);
  const ResizePlane u = {j.u + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pl.w >> 1), (uint32_t) (pl.h >> 1), M == 6 ? fj->cx : none, M == 6 ? fj->cy : none};
  const ResizePlane v = {j.v + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pl.w >> 1), (uint32_t) (pl.h >> 1), M == 6 ? fj->cx : none, M == 6 ? fj->cy : none};
  uint8_t* dc = j.dst + (size_t)ow * oh;
  if (j.format == LH264_FMT_NV12) {
    const int pieces = (ow + 6) >> 2, items = (c1 - c0) * pieces;
    for (int it = t; it < items; it += nt) {
      const int r = c0 + it / pieces, p = it % pieces;
      piece_placed<M> (dc + (size_t)r * ow, ow, r, p, u, v, true, pl.x, pl.x + pl.w, pl.y >> 1, fcb, fcr);
    }
  } else {
    const int pieces = (ocw + 6) >> 2, per_plane = (c1 - c0) * pieces;
    for (int it = t; it < 2 * per_plane; it += nt) {
      const int plane = it >= per_plane, q = it - plane * per_plane;
      const int r = c0 + q / pieces, p = q % pieces;
      const uint32_t f = plane ? fcr : fcb;
      piece_placed<M> (dc + (size_t)plane * ocw * och + (size_t)r * ocw, ocw, r, p, plane ? v : u, u, false, pl.x >> 1, (pl.x + pl.w) >> 1, pl.y >> 1, f, f);
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

// delivered sample (X, Y) of a plane resampled by its filter tables (the definition: include/lh264.h at lh264_decode_batch_ex6): the row
// sums H by the column weights in 32 bits, their sum by the row weights in 64, one rounding and the clamp at the end.  Every tap lies
// inside the window: no byte outside it is read
__host__ __device__ inline uint32_t filtered_sample (const ResizePlane& pl, int X, int Y) {
  const int32_t* ex = pl.fx.ent + 3 * X;
  const int32_t* ey = pl.fy.ent + 3 * Y;
  const int16_t* kx = pl.fx.k + ex[2];
  const int16_t* ky = pl.fy.k + ey[2];
  const int nx = ex[1], ny = ey[1];
  const uint8_t* row = pl.p + (size_t)ey[0] * pl.stride + ex[0];
  int64_t S = 0;
  for (int y = 0; y < ny; y++, row += pl.stride) {
    int32_t H = 0;
    for (int x = 0; x < nx; x++) H += (int32_t)kx[x] * (int32_t)row[x];
    S += (int64_t)ky[y] * H;
  }
  return clip8 ((int32_t) ((S + ((int64_t)1 << 27)) >> 28));
}

// delivered sample (X, Y) of one plane under sizing M: 0 the window, 1..3 the means of scale_log2, 4 the given size (sy: the rows of Y),
// 6 the given size by the plane's filter tables
template <int M>
__host__ __device__ inline int plane_sample (const ResizePlane& pl, const Span& sy, int X, int Y) {
  if constexpr (M == 0) return pl.p[(size_t)Y * pl.stride + X];
  else if constexpr (M <= 3) return mean_clamped<M> (pl.p, pl.stride, (int)pl.w, (int)pl.h, X, Y);
  else if constexpr (M == 6) return (int)filtered_sample (pl, X, Y);
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
// Sizing M = 7 is M = 5 with the rectangle's samples from quad_rgb<6>: the planes' filter tables in the area means' place
struct Placed { int x, y; uint32_t fill; };
constexpr bool placed_sizing (int M) { return M == 5 || M == 7; }
constexpr int placed_inner (int M) { return M == 5 ? 4 : 6; }
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
  if constexpr (placed_sizing (M)) {
    bar_rgb (pc.fill, f, y0, bar);
    rows_in = 2 * R >= pc.y && 2 * R < pc.y + (int)py.oh;
    if (M == 5 && rows_in) { sy[0] = span_of ((uint32_t) (2 * R - pc.y), py.h, py.oh); sy[1] = span_of ((uint32_t) (2 * R + 1 - pc.y), py.h, py.oh); sc = span_of ((uint32_t) (R - (pc.y >> 1)), pu.h, pu.oh); }
  }
  // the 12 pixels of both rows as byte streams: RGB24 one stream of 36 bytes, RGBP three of 12
  uint32_t W[2][NP][NW + 1];
  for (int rr = 0; rr < 2; rr++) for (int c = 0; c < NP; c++) for (int k = 0; k <= NW; k++) W[rr][c][k] = 0;
  _Pragma ("unroll")
  for (int q = 0; q < kRgbQuads; q++) {
    const int X = x0 + 2 * q;
    if (X < 0 || X >= ow) continue;
    uint32_t px[2][2][3];
    if constexpr (placed_sizing (M)) {
      if (rows_in && X >= pc.x && X < pc.x + (int)py.ow) quad_rgb<placed_inner (M)> (py, pu, pv, sy, sc, f, y0, X - pc.x, R - (pc.y >> 1), px);
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
__host__ __device__ inline void pack_band_rgb_as (const lh264_pack_job_t& j, int ow, int oh, int std_byte, int band, int t, int nt, const lh264_pack_place_t* pl = nullptr, const FilterJob* fj = nullptr) {
  const int w = j.crop_w, h = j.crop_h;
  const int R0 = band * (kBandRows / 2), R1 = R0 + kBandRows / 2 < (oh >> 1) ? R0 + kBandRows / 2 : (oh >> 1);
  if (R1 <= R0) return;
  const size_t co = (size_t) (j.crop_y >> 1) * j.stride_c + (j.crop_x >> 1);
  const int pw = placed_sizing (M) ? pl->w : ow, ph = placed_sizing (M) ? pl->h : oh;
  const Placed pc = placed_sizing (M) ? Placed {pl->x, pl->y, pl->fill} : Placed {0, 0, 0u};
  const FilterAxis none = {nullptr, nullptr};
  const ResizePlane py = {j.y + (size_t)j.crop_y * j.stride_y + j.crop_x, j.stride_y, (uint32_t)w, (uint32_t)h, (uint32_t)pw, (uint32_t)ph, M == 7 ? fj->lx : none, M == 7 ? fj->ly : none};
  const ResizePlane pu = {j.u + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pw >> 1), (uint32_t) (ph >> 1), M == 7 ? fj->cx : none, M == 7 ? fj->cy : none};
  const ResizePlane pv = {j.v + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pw >> 1), (uint32_t) (ph >> 1), M == 7 ? fj->cx : none, M == 7 ? fj->cy : none};
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
  if constexpr (placed_sizing (M)) {
    uint32_t bar[3];
    bar_rgb (pc.fill, f, y0, bar);
    for (int c = 0; c < 3; c++) barv[c] = __builtin_fmaf ((float)bar[c], mul[c], add[c]);
    rows_in = 2 * R >= pc.y && 2 * R < pc.y + (int)py.oh;
    if (M == 5 && rows_in) { sy[0] = span_of ((uint32_t) (2 * R - pc.y), py.h, py.oh); sy[1] = span_of ((uint32_t) (2 * R + 1 - pc.y), py.h, py.oh); sc = span_of ((uint32_t) (R - (pc.y >> 1)), pu.h, pu.oh); }
  }
  uint32_t W[2][NP][NW];                                                             // the item's words, per row and plane
  for (int rr = 0; rr < 2; rr++) for (int c = 0; c < NP; c++) for (int k = 0; k < NW; k++) W[rr][c][k] = 0;
  _Pragma ("unroll")
  for (int q = 0; q < 4; q++) {
    if (q >= nq) continue;
    uint32_t px[2][2][3];
    bool in_bar = false;
    if constexpr (placed_sizing (M)) {
      const int X = X0 + 2 * q;
      in_bar = !(rows_in && X >= pc.x && X < pc.x + (int)py.ow);
      if (!in_bar) quad_rgb<placed_inner (M)> (py, pu, pv, sy, sc, f, y0, X - pc.x, R - (pc.y >> 1), px);
      else for (int rr = 0; rr < 2; rr++) for (int i = 0; i < 2; i++) for (int c = 0; c < 3; c++) px[rr][i][c] = 0;
    } else quad_rgb<M> (py, pu, pv, sy, sc, f, y0, X0 + 2 * q, R, px);
    _Pragma ("unroll")
    for (int rr = 0; rr < 2; rr++) {
      float v[2][3];
      _Pragma ("unroll")
      for (int i = 0; i < 2; i++) {
        _Pragma ("unroll")
        for (int c = 0; c < 3; c++) v[i][c] = (placed_sizing (M) && in_bar) ? barv[c] : __builtin_fmaf ((float)px[rr][i][c], mul[c], add[c]);      // one fused multiply-add: the definition's
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
__host__ __device__ LH264_SAMPLE_INLINE void pack_band_sample_as (const lh264_pack_job_t& j, int ow, int oh, int std_byte, const float* mul, const float* add, int band, int t, int nt, const lh264_pack_place_t* pl = nullptr, const FilterJob* fj = nullptr) {
  const int w = j.crop_w, h = j.crop_h;
  const int R0 = band * (kBandRows / 2), R1 = R0 + kBandRows / 2 < (oh >> 1) ? R0 + kBandRows / 2 : (oh >> 1);
  if (R1 <= R0) return;
  const size_t co = (size_t) (j.crop_y >> 1) * j.stride_c + (j.crop_x >> 1);
  const int pw = placed_sizing (M) ? pl->w : ow, ph = placed_sizing (M) ? pl->h : oh;      // (pl: the job's place, read under M = 5 and 7 only)
  const Placed pc = placed_sizing (M) ? Placed {pl->x, pl->y, pl->fill} : Placed {0, 0, 0u};
  const FilterAxis none = {nullptr, nullptr};
  const ResizePlane py = {j.y + (size_t)j.crop_y * j.stride_y + j.crop_x, j.stride_y, (uint32_t)w, (uint32_t)h, (uint32_t)pw, (uint32_t)ph, M == 7 ? fj->lx : none, M == 7 ? fj->ly : none};
  const ResizePlane pu = {j.u + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pw >> 1), (uint32_t) (ph >> 1), M == 7 ? fj->cx : none, M == 7 ? fj->cy : none};
  const ResizePlane pv = {j.v + co, j.stride_c, (uint32_t) (w >> 1), (uint32_t) (h >> 1), (uint32_t) (pw >> 1), (uint32_t) (ph >> 1), M == 7 ? fj->cx : none, M == 7 ? fj->cy : none};
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

// ---- the filtered pack step: lh264_decode_batch_ex6 with LH264_FILTER_BILINEAR / _BICUBIC (the definition: include/lh264.h there) ------
// The placed steps above with filtered_sample in resized_sample's place: the window is resampled to pl.w x pl.h by the job's four
// tables and lies at (pl.x, pl.y) of the out_w x out_h picture (a job that is not placed: the whole picture, no bar).  Bands, pieces,
// stores and bars are the placed steps'; a sample costs taps_y * taps_x multiply-adds, each tap read from the window once per sample.
__host__ __device__ inline void pack_band_filtered (const lh264_pack_job_t& j, const FilterJob& fj, const lh264_pack_place_t& pl, int out_w, int out_h, int band, int t, int nt) {
  if (j.crop_w <= 0 || j.crop_h <= 0 || j.reserved) return;
  pack_band_placed<6> (j, pl, out_w, out_h, band, t, nt, &fj);
}
__host__ __device__ inline void pack_band_rgb_filtered (const lh264_pack_job_t& j, const FilterJob& fj, const lh264_pack_place_t& pl, int out_w, int out_h, int layout, int std_byte, int band, int t, int nt) {
  if (j.crop_w <= 0 || j.crop_h <= 0 || j.reserved) return;
  if (layout == (int)LH264_COLOUR_RGB24) pack_band_rgb_as<7, (int)LH264_COLOUR_RGB24> (j, out_w, out_h, std_byte, band, t, nt, &pl, &fj);
  else if (layout == (int)LH264_COLOUR_RGBP) pack_band_rgb_as<7, (int)LH264_COLOUR_RGBP> (j, out_w, out_h, std_byte, band, t, nt, &pl, &fj);
}
template <int L>
__host__ __device__ LH264_SAMPLE_INLINE void pack_band_sample_filtered_in (const lh264_pack_job_t& j, const FilterJob& fj, const lh264_pack_place_t& pl, int ow, int oh, int type, int std_byte, const float* mul, const float* add, int band, int t, int nt) {
  if (type == (int)LH264_SAMPLE_F32) pack_band_sample_as<7, L, (int)LH264_SAMPLE_F32> (j, ow, oh, std_byte, mul, add, band, t, nt, &pl, &fj);
  else if (type == (int)LH264_SAMPLE_F16) pack_band_sample_as<7, L, (int)LH264_SAMPLE_F16> (j, ow, oh, std_byte, mul, add, band, t, nt, &pl, &fj);
  else if (type == (int)LH264_SAMPLE_BF16) pack_band_sample_as<7, L, (int)LH264_SAMPLE_BF16> (j, ow, oh, std_byte, mul, add, band, t, nt, &pl, &fj);
}
__host__ __device__ LH264_SAMPLE_INLINE void pack_band_sample_filtered (const lh264_pack_job_t& j, const FilterJob& fj, const lh264_pack_place_t& pl, int out_w, int out_h, int layout, int std_byte, const lh264_decode_sample_t& sm, int band, int t, int nt) {
  if (j.crop_w <= 0 || j.crop_h <= 0 || j.reserved || ((uintptr_t)j.dst & 3u)) return;
  if (layout == (int)LH264_COLOUR_RGB24) pack_band_sample_filtered_in<(int)LH264_COLOUR_RGB24> (j, fj, pl, out_w, out_h, (int)sm.type, std_byte, sm.mul, sm.add, band, t, nt);
  else if (layout == (int)LH264_COLOUR_RGBP) pack_band_sample_filtered_in<(int)LH264_COLOUR_RGBP> (j, fj, pl, out_w, out_h, (int)sm.type, std_byte, sm.mul, sm.add, band, t, nt);
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
