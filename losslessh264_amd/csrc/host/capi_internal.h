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

// One slice whose macroblock layer is parsed apart from its header (CAVLC: lh264_slice.h, on the device by slice_parse_kernel; CABAC:
// lh264_slice_cabac.h, by slice_parse_cabac_kernel; on the host by the same code).  The pointers are the walker's own: device addresses for the kernel, host addresses for the CPU form.
namespace lh264host {
struct SliceTask {
  const uint8_t* rbsp;              // the slice NAL's unescaped payload ...
  uint32_t rbsp_bytes, data_bit;    // ... its length, and the bit at which slice_data() begins
  int32_t first_mb, limit_mb;       // the slice may write macroblocks [first_mb, limit_mb): limit_mb is the next slice's first_mb, or mb_w * mb_h
  int32_t mb_w, mb_h;
  int32_t slice_index;              // in its picture's lh264_slice_t table (the records' slice_id)
  int32_t slice_qp;
  uint8_t slice_type, num_ref_idx_l0, transform_8x8, constrained_intra_pred, use_sl;
  int8_t chroma_qp_offset[2];
  uint8_t reserved;                 // 0: CAVLC.  CABAC: lh264slice::kTaskCabac | cabac_init_idc.  Checked by task_ok since the CABAC walk
                                    // exists: a CAVLC task with any other value here is SLICE_BAD_TASK (the byte used to be ignored)
  const uint8_t* scaling;           // use_sl: the PPS's resolved lists, 6 x 16 then 2 x 64 entries in raster order
  lh264_mb_t* mbs;                  // the picture's records, 16-byte aligned
  int16_t* coeffs;                  // the picture's coefficient plane, cleared by the caller
  lh264_slice_t* slice;             // the slice's table entry: n_mbs is written (may be null: the result carries it too)
  int8_t* line;                     // 4 * mb_w bytes of scratch (CABAC: lh264slice::kCabacLineBytes * mb_w); the kernels need it only for pictures wider than their LDS line
};
static_assert (sizeof (SliceTask) == 88, "SliceTask is fixed-width: the host fills what the kernel reads");
struct SliceResult { int32_t status, n_mbs, stop_bit; };
// lh264_slice.hip: n tasks in device memory through slice_parse_kernel, enqueued on `stream`; force_fail: -1, or the task that is to
// report a status unwalked
bool launch_slice_parse (const SliceTask* tasks_dev, SliceResult* results_dev, int n, void* stream, int force_fail);
// ... and n CABAC tasks through slice_parse_cabac_kernel
bool launch_slice_parse_cabac (const SliceTask* tasks_dev, SliceResult* results_dev, int n, void* stream, int force_fail);
}

// n entries of (index << 16 | 16-bit value) in device memory written into the dense planes (lh264_capi.hip: expand_sparse_kernel, one
// thread per entry, enqueued on `stream`); n > 0.  The caller asks hipGetLastError() if it wants to know
namespace lh264host { void expand_sparse (const uint64_t* ents_dev, size_t n, int16_t* dense_dev, void* stream); }
