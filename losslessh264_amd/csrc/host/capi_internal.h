// capi_internal.h - what the C ABI's opaque handles are, for the translation units of the library that share them
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <atomic>
#include <thread>
#include <vector>
#include "h264_parser.h"
struct lh264_parser { lh264host::Parser p; mutable std::vector<uint8_t> escapes; };      // escapes: what lh264_parser_escapes handed out last
static inline lh264host::Parser* lh264_parser_impl (lh264_parser* h) { return h ? &h->p : nullptr; }

// n independent pieces of work on `threads` host threads (0 = one per hardware thread)
template <typename F> static void run_parallel (int n, int threads, F&& fn) {
  if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
  if (threads < 1) threads = 1;
  if (threads > n) threads = n;
  std::atomic<int> next (0);
  auto worker = [&] () { for (;;) { const int i = next.fetch_add (1); if (i >= n) break; fn (i); } };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; t++) pool.emplace_back (worker);
  worker();
  for (auto& t : pool) t.join();
}

// n entries of (index << 16 | 16-bit value) in device memory written into the dense planes (lh264_capi.hip: expand_sparse_kernel, one
// thread per entry, enqueued on `stream`); n > 0.  The caller asks hipGetLastError() if it wants to know
namespace lh264host { void expand_sparse (const uint64_t* ents_dev, size_t n, int16_t* dense_dev, void* stream); }
