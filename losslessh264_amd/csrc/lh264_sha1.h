// lh264_sha1.h - SHA-1 (FIPS 180-4) for the digests of decoded pictures, host and device from one source: the compression function
// over one 64-byte block, and around it update / finalise on a state record that lies in memory (a stream's record stays in device
// memory between the rounds of a decode call; the host finalises a downloaded copy with the same function).  sha1_spans_kernel
// (lh264_decode.hip) runs one lane per job of a table the host fills.  Plain C++: the rotates become v_alignbit_b32, the big-endian
// word load a byte permute.
#pragma once
#include <stdint.h>
#include <string.h>

// {h[5], the message's length so far in bytes as 64 bits, the bytes of the block that is not full yet}: 92 bytes, padded to 96
struct lh264_sha1_state_t {
  uint32_t h[5];
  uint32_t len_lo, len_hi;
  uint8_t buf[64];
  uint32_t reserved;
};
static_assert (sizeof (lh264_sha1_state_t) == 96, "the state record is 96 bytes");

enum { LH264_SHA1_FRESH = 1, LH264_SHA1_FINAL = 2 };
// one span of one message: `len` bytes at `src` go into the message whose record is `state` (FRESH: the record is initialised
// first).  FINAL: the message ends behind the span and its 20-byte digest goes to `out`; otherwise a non-null `out` takes a copy of
// the record as the span leaves it (96 bytes).  No record may be named by two jobs of one launch.
struct lh264_sha1_job_t {
  const uint8_t* src;
  uint64_t len;
  lh264_sha1_state_t* state;
  uint8_t* out;
  uint32_t flags, reserved;
};
static_assert (sizeof (lh264_sha1_job_t) == 40, "the span job is 40 bytes");

namespace lh264sha1 {

__host__ __device__ inline uint32_t rol (uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

// FIPS 180-4 section 6.1.2 over one block; w: its 16 words, big-endian already.  The schedule is a ring of 16 words: with the loop
// unrolled every index is a constant and the ring stays in registers.
__host__ __device__ inline void block (uint32_t h[5], uint32_t w[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
  for (int t = 0; t < 80; t++) {
    uint32_t x;
    if (t < 16) x = w[t];
    else x = w[t & 15] = rol (w[(t + 13) & 15] ^ w[(t + 8) & 15] ^ w[(t + 2) & 15] ^ w[t & 15], 1);
    uint32_t f, k;
    if (t < 20)      { f = d ^ (b & (c ^ d));       k = 0x5a827999u; }
    else if (t < 40) { f = b ^ c ^ d;               k = 0x6ed9eba1u; }
    else if (t < 60) { f = (b & c) | (d & (b | c)); k = 0x8f1bbcdcu; }
    else             { f = b ^ c ^ d;               k = 0xca62c1d6u; }
    const uint32_t tmp = rol (a, 5) + f + e + k + x;
    e = d; d = c; c = rol (b, 30); b = a; a = tmp;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}

// the 16 big-endian words of the 64 bytes at p, p at any byte address.  On the device in two steps, so that the next block's loads
// can be in flight while this one is worked on: raw() fetches the aligned dwords that hold the block (16, and a 17th where p is not
// 4-byte aligned: it holds bytes of the block, so it lies in memory the block lies in) as dwordx4 loads, words() moves them into
// place in registers (v_alignbyte_b32; a shift of 0 leaves the word as it is) and swaps the bytes.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline void raw (const uint8_t* p, uint32_t d[17]) {
  struct __attribute__ ((aligned (4))) Quad { uint32_t v[4]; };
  const uint32_t r = (uint32_t) ((uintptr_t)p & 3u);
  const uint8_t* q = p - r;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    Quad x;
    __builtin_memcpy (&x, q + 16 * k, 16);
    d[4 * k] = x.v[0]; d[4 * k + 1] = x.v[1]; d[4 * k + 2] = x.v[2]; d[4 * k + 3] = x.v[3];
  }
  d[16] = 0;
  if (r) d[16] = * (const uint32_t*) (q + 64);
}
__device__ inline void words (const uint32_t d[17], uint32_t r, uint32_t w[16]) {
#pragma unroll
  for (int k = 0; k < 16; k++) w[k] = __builtin_bswap32 (__builtin_amdgcn_alignbyte (d[k + 1], d[k], r));
}
#endif
__host__ __device__ inline void load_block (const uint8_t* p, uint32_t w[16]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t d[17];
  raw (p, d);
  words (d, (uint32_t) ((uintptr_t)p & 3u), w);
#else
  for (int k = 0; k < 16; k++) w[k] = (uint32_t)p[4 * k] << 24 | (uint32_t)p[4 * k + 1] << 16 | (uint32_t)p[4 * k + 2] << 8 | (uint32_t)p[4 * k + 3];
#endif
}

__host__ __device__ inline void init (lh264_sha1_state_t* s) {
  s->h[0] = 0x67452301u; s->h[1] = 0xefcdab89u; s->h[2] = 0x98badcfeu; s->h[3] = 0x10325476u; s->h[4] = 0xc3d2e1f0u;
  s->len_lo = 0; s->len_hi = 0; s->reserved = 0;
  for (int k = 0; k < 64; k++) s->buf[k] = 0;
}

// n more bytes of the message.  Bytes that complete the record's partial block and the bytes behind the last whole block go byte by
// byte through the record; the whole blocks between them are read where they lie.
__host__ __device__ inline void update (lh264_sha1_state_t* s, const uint8_t* p, uint64_t n) {
  uint32_t h[5], w[16];
  for (int k = 0; k < 5; k++) h[k] = s->h[k];
  const uint64_t total = ((uint64_t)s->len_hi << 32 | s->len_lo) + n;
  uint32_t fill = s->len_lo & 63u;
  if (fill) {
    while (fill < 64 && n) { s->buf[fill++] = *p++; n--; }
    if (fill == 64) { load_block (s->buf, w); block (h, w); fill = 0; }
  }
#if defined(__HIP_DEVICE_COMPILE__)
  if (n >= 64) {
    const uint32_t r = (uint32_t) ((uintptr_t)p & 3u);
    uint32_t d[17];
    raw (p, d);
    for (;;) {
      words (d, r, w);
      p += 64; n -= 64;
      const bool more = n >= 64;
      if (more) raw (p, d);                 // in flight during the 80 rounds below
      block (h, w);
      if (!more) break;
    }
  }
#else
  for (; n >= 64; n -= 64, p += 64) { load_block (p, w); block (h, w); }
#endif
  for (uint32_t k = 0; k < (uint32_t)n; k++) s->buf[fill + k] = p[k];       // (n > 0 only where fill is 0 here)
  for (int k = 0; k < 5; k++) s->h[k] = h[k];
  s->len_lo = (uint32_t)total; s->len_hi = (uint32_t) (total >> 32);
}

// padding (a 1 bit, zeros, the length in bits as 64 bits, big-endian) and the digest's 20 bytes.  The record is used up.
__host__ __device__ inline void finish (lh264_sha1_state_t* s, uint8_t out[20]) {
  uint32_t h[5], w[16];
  for (int k = 0; k < 5; k++) h[k] = s->h[k];
  const uint64_t bits = ((uint64_t)s->len_hi << 32 | s->len_lo) << 3;
  uint32_t fill = s->len_lo & 63u;
  s->buf[fill++] = 0x80;
  if (fill > 56) {
    while (fill < 64) s->buf[fill++] = 0;
    load_block (s->buf, w); block (h, w);
    fill = 0;
  }
  while (fill < 56) s->buf[fill++] = 0;
  for (int k = 0; k < 8; k++) s->buf[56 + k] = (uint8_t) (bits >> (56 - 8 * k));
  load_block (s->buf, w); block (h, w);
  for (int k = 0; k < 5; k++) { out[4 * k] = (uint8_t) (h[k] >> 24); out[4 * k + 1] = (uint8_t) (h[k] >> 16); out[4 * k + 2] = (uint8_t) (h[k] >> 8); out[4 * k + 3] = (uint8_t)h[k]; }
}

// one job, as a lane of sha1_spans_kernel runs it and as the host steps it
__host__ __device__ inline void run_job (const lh264_sha1_job_t& j) {
  if (j.flags & LH264_SHA1_FRESH) init (j.state);
  update (j.state, j.src, j.len);
  if (j.flags & LH264_SHA1_FINAL) finish (j.state, j.out);
  else if (j.out) { const uint32_t* a = (const uint32_t*)j.state; uint32_t* o = (uint32_t*)j.out; for (int k = 0; k < 24; k++) o[k] = a[k]; }
}

}  // namespace lh264sha1
