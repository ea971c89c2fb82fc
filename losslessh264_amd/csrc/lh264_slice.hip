// lh264_slice.hip - slice_parse_kernel and slice_parse_cabac_kernel: the CAVLC macroblock layer of lh264_slice.h and the CABAC one of
// lh264_slice_cabac.h on the device, one wave64 per slice, and lh264_debug_slice_parse_opts, which runs one stream's deferred slices
// through that code on the host or through the kernels and hands back what it wrote, with guard bytes behind every buffer.  DESIGN.md
// section 4.4.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/lh264.h"
#include "host/h264_parser.h"
#include "host/capi_internal.h"
#include "host/device_mem.h"
#include "lh264_slice.h"
#include "lh264_slice_cabac.h"

using lh264host::SliceResult;
using lh264host::SliceTask;

// One wave per task.  The lanes copy the table record and - up to kLdsRbspBytes - the slice's payload into LDS together; lane 0 walks
// the slice: a slice is one serial chain of variable-length codes, the width comes from the batch.  The record in hand and (for
// pictures up to kLdsLineMbs macroblocks wide) the line of intra modes lie in LDS; records of neighbours are read back from where the
// lane wrote them.
enum { kLdsRbspBytes = 4096 };
__global__ void __launch_bounds__ (64) slice_parse_kernel (const SliceTask* __restrict__ tasks, SliceResult* __restrict__ results, int n,
                                                           const lh264slice::Tables* __restrict__ tables, int force_fail) {
  __shared__ lh264slice::Tables T;
  __shared__ alignas (16) lh264_mb_t rec;
  __shared__ int8_t line[lh264slice::kLdsLineMbs * 4];
  __shared__ uint8_t payload[kLdsRbspBytes];
  const int i = (int)blockIdx.x;
  if (i >= n) return;
  SliceTask t = tasks[i];
  // (the same for every lane: an inconsistent task - or the one a test asks to fail - gets its status before anything it names is read)
  if (i == force_fail || !lh264slice::task_ok (t)) {
    if (threadIdx.x == 0) { SliceResult r = {i == force_fail ? lh264slice::SLICE_SYNTAX : lh264slice::SLICE_BAD_TASK, 0, 0}; results[i] = r; }
    return;
  }
  const bool staged = t.rbsp_bytes <= (uint32_t)kLdsRbspBytes;
  if (staged) for (uint32_t q = threadIdx.x; q < t.rbsp_bytes; q += 64) payload[q] = t.rbsp[q];
  {
    const uint4* s = (const uint4*)tables; uint4* d = (uint4*)&T;
    for (int q = (int)threadIdx.x; q < (int) (sizeof (lh264slice::Tables) / 16); q += 64) d[q] = s[q];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (staged) t.rbsp = payload;
  results[i] = lh264slice::parse_slice (T, t, &rec, t.mb_w > lh264slice::kLdsLineMbs ? t.line : line);
}

// The CABAC form, a kernel of its own (slice_parse_kernel's registers, scratch and LDS stay what they are).  One wave per task again:
// the lanes copy the table record and the payload as above and initialise the slice's 460 context bytes from its column of the
// (m, n) table (`init`, [460][4][2], read once from global memory); lane 0 walks the slice with the record in hand, the context bytes
// and (for pictures up to kLdsLineMbs macroblocks wide) the line in LDS.
__global__ void __launch_bounds__ (64) slice_parse_cabac_kernel (const SliceTask* __restrict__ tasks, SliceResult* __restrict__ results, int n,
                                                                 const lh264slice::CabacTables* __restrict__ tables, const int8_t* __restrict__ init, int force_fail) {
  __shared__ lh264slice::CabacTables T;
  __shared__ alignas (16) lh264_mb_t rec;
  __shared__ alignas (16) uint8_t line[lh264slice::kLdsLineMbs * lh264slice::kCabacLineBytes];
  __shared__ uint8_t payload[kLdsRbspBytes];
  __shared__ uint8_t state[lh264slice::kCabacContexts];
  const int i = (int)blockIdx.x;
  if (i >= n) return;
  SliceTask t = tasks[i];
  if (i == force_fail || !lh264slice::cabac_task_ok (t)) {
    if (threadIdx.x == 0) { SliceResult r = {i == force_fail ? lh264slice::SLICE_SYNTAX : lh264slice::SLICE_BAD_TASK, 0, 0}; results[i] = r; }
    return;
  }
  const bool staged = t.rbsp_bytes <= (uint32_t)kLdsRbspBytes;
  if (staged) for (uint32_t q = threadIdx.x; q < t.rbsp_bytes; q += 64) payload[q] = t.rbsp[q];
  {
    const uint4* s = (const uint4*)tables; uint4* d = (uint4*)&T;
    for (int q = (int)threadIdx.x; q < (int) (sizeof (lh264slice::CabacTables) / 16); q += 64) d[q] = s[q];
  }
  {
    const int col = lh264slice::cabac_init_column (t);      // 0..3: task_ok has checked cabac_init_idc
    for (int q = (int)threadIdx.x; q < lh264slice::kCabacContexts; q += 64) state[q] = lh264slice::cabac_init_state (init[(q * 4 + col) * 2], init[(q * 4 + col) * 2 + 1], t.slice_qp);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (staged) t.rbsp = payload;
  results[i] = lh264slice::parse_slice_cabac (T, t, &rec, t.mb_w > lh264slice::kLdsLineMbs ? (uint8_t*)t.line : line, state);
}

namespace lh264host {

namespace {
struct TablesDev { DevBuf buf; bool up = false; };
PerDevice<TablesDev> g_tables, g_cabac_tables;
const size_t kCabacInitAt = (sizeof (lh264slice::CabacTables) + 15) & ~ (size_t)15;      // the (m, n) table lies behind the record
}

const lh264slice::CabacTables& slice_cabac_tables_host() {
  static const lh264slice::CabacTables* t = [] { lh264slice::CabacTables* p = new lh264slice::CabacTables(); lh264slice::fill_cabac_tables (*p); return p; }();
  return *t;
}

// the same for CABAC tasks through slice_parse_cabac_kernel
bool launch_slice_parse_cabac (const SliceTask* tasks_dev, SliceResult* results_dev, int n, void* stream, int force_fail) {
  if (n <= 0) return true;
  int device = 0;
  if (hipGetDevice (&device) != hipSuccess || device < 0 || device >= kMaxDevices) return false;
  const uint8_t* td = nullptr;
  {
    auto ref = g_cabac_tables.lock (device);
    TablesDev& t = ref.get();
    if (!t.up) {
      static_assert (sizeof (kCabacInit) == lh264slice::kCabacContexts * 8, "kCabacInit");
      if (!t.buf.alloc (kCabacInitAt + sizeof (kCabacInit)) || hipMemcpy (t.buf.p, &slice_cabac_tables_host(), sizeof (lh264slice::CabacTables), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy ((uint8_t*)t.buf.p + kCabacInitAt, kCabacInit, sizeof (kCabacInit), hipMemcpyHostToDevice) != hipSuccess) return false;
      t.up = true;
    }
    td = t.buf.as<uint8_t>();
  }
  hipLaunchKernelGGL (slice_parse_cabac_kernel, dim3 ((unsigned)n), dim3 (64), 0, (hipStream_t)stream, tasks_dev, results_dev, n,
                      (const lh264slice::CabacTables*)td, (const int8_t*) (td + kCabacInitAt), force_fail);
  return hipGetLastError() == hipSuccess;
}

const lh264slice::Tables& slice_tables_host() {
  static const lh264slice::Tables* t = [] { lh264slice::Tables* p = new lh264slice::Tables(); lh264slice::fill_tables (*p); return p; }();
  return *t;
}

// n tasks in device memory (longest first pays: a wave ends with its slice), one result each; enqueued on `stream`.  force_fail >= 0:
// that task reports SLICE_SYNTAX without being walked (the tests' forced fallback).  false: the table record could not be put on the
// device, or the launch failed
bool launch_slice_parse (const SliceTask* tasks_dev, SliceResult* results_dev, int n, void* stream, int force_fail) {
  if (n <= 0) return true;
  int device = 0;
  if (hipGetDevice (&device) != hipSuccess || device < 0 || device >= kMaxDevices) return false;
  const lh264slice::Tables* td = nullptr;
  {
    auto ref = g_tables.lock (device);
    TablesDev& t = ref.get();
    if (!t.up) {
      if (!t.buf.alloc (sizeof (lh264slice::Tables)) || hipMemcpy (t.buf.p, &slice_tables_host(), sizeof (lh264slice::Tables), hipMemcpyHostToDevice) != hipSuccess) return false;
      t.up = true;
    }
    td = t.buf.as<lh264slice::Tables>();
  }
  hipLaunchKernelGGL (slice_parse_kernel, dim3 ((unsigned)n), dim3 (64), 0, (hipStream_t)stream, tasks_dev, results_dev, n, td, force_fail);
  return hipGetLastError() == hipSuccess;
}

}  // namespace lh264host

// ---- lh264_debug_slice_parse ---------------------------------------------------------------------------------------------------------
struct lh264_slice_dump {
  struct Pic { int mb_w = 0, mb_h = 0, n_slices = 0, n_deferred = 0; size_t mbs = 0, coeffs = 0, slices = 0; std::vector<int32_t> results; };
  std::vector<Pic> pics;
  uint8_t* arena = nullptr; size_t arena_bytes = 0;
  std::vector<std::pair<size_t, size_t>> guards;      // (offset, bytes) of every guard zone
  bool guards_ok = false;
  std::string error;
  ~lh264_slice_dump() { free (arena); }
};

namespace {
const size_t kGuard = 64;
const uint8_t kGuardByte = 0xA5;
}

extern "C" {

int lh264_debug_slice_parse (const uint8_t* data, size_t len, int on_device, int threads, const int32_t* tweak, lh264_slice_dump_t** out) {
  int32_t tw[4] = {tweak ? tweak[0] : -1, tweak ? tweak[1] : -1, tweak ? tweak[2] : 0, -1};
  return lh264_debug_slice_parse_opts (data, len, on_device ? LH264_SLICE_PARSE_ON_DEVICE : 0, threads, tweak ? tw : nullptr, out);
}

int lh264_debug_slice_parse_opts (const uint8_t* data, size_t len, uint32_t flags, int threads, const int32_t* tweak, lh264_slice_dump_t** out) {
  if (!out || (!data && len) || (flags & ~ (uint32_t) (LH264_SLICE_PARSE_ON_DEVICE | LH264_SLICE_PARSE_CABAC))) return LH264_E_ARG;
  *out = nullptr;
  const bool on_device = (flags & LH264_SLICE_PARSE_ON_DEVICE) != 0;
  if (on_device && lh264_device_count() <= 0) return LH264_E_NODEVICE;
  using namespace lh264host;
  Parser P;
  P.set_defer_slice_data (true);
  P.set_defer_cabac ((flags & LH264_SLICE_PARSE_CABAC) != 0);
  P.set_sparse_levels (true);
  P.feed_file (data, len);
  std::unique_ptr<lh264_slice_dump> D (new lh264_slice_dump());
  D->error = P.error();
  auto& frames = P.frames();
  // the arena: every buffer 16-byte aligned with a guard zone behind it; tasks name offsets until the base is known
  size_t at = 0;
  auto take = [&] (size_t bytes) { const size_t o = at; at += (bytes + 15) & ~ (size_t)15; D->guards.push_back ({at, kGuard}); at += kGuard; return o; };
  struct Job { size_t pic, def; size_t rbsp, scaling, line; };
  std::vector<Job> jobs;
  for (size_t p = 0; p < frames.size(); p++) {
    FrameOut& f = *frames[p];
    const size_t n = (size_t)f.mb_w * f.mb_h;
    lh264_slice_dump::Pic pc;
    pc.mb_w = f.mb_w; pc.mb_h = f.mb_h; pc.n_slices = (int)f.slices.size(); pc.n_deferred = (int)f.deferred.size();
    pc.mbs = take (n * sizeof (lh264_mb_t)); pc.coeffs = take (n * 768); pc.slices = take (f.slices.size() * sizeof (lh264_slice_t));
    pc.results.assign (f.slices.size() * 4, 0);
    for (size_t d = 0; d < f.deferred.size(); d++) {
      const DeferredSlice& ds = f.deferred[d];
      jobs.push_back ({p, d, take (ds.rbsp.size()), take (224), take ((size_t)f.mb_w * (ds.cabac ? (size_t)lh264slice::kCabacLineBytes : 4))});
    }
    D->pics.push_back (std::move (pc));
  }
  const size_t tasks_at = take (jobs.size() * sizeof (SliceTask)), results_at = take (jobs.size() * sizeof (SliceResult));
  D->arena_bytes = at;
  if (posix_memalign ((void**)&D->arena, 64, at ? at : 64) != 0) { D->arena = nullptr; return LH264_E_ARG; }
  uint8_t* const A = D->arena;
  memset (A, 0, at);
  for (auto& g : D->guards) memset (A + g.first, kGuardByte, g.second);
  uint8_t* dev = nullptr;
  if (on_device && hipMalloc ((void**)&dev, at ? at : 64) != hipSuccess) return LH264_E_HIP;
  uint8_t* const B = on_device ? dev : A;               // the base the tasks' pointers are made from
  // longest first, as the restore kernel takes its streams; the CAVLC tasks in front of the CABAC ones: one launch each
  std::stable_sort (jobs.begin(), jobs.end(), [&] (const Job& a, const Job& b) { return frames[a.pic]->deferred[a.def].rbsp.size() > frames[b.pic]->deferred[b.def].rbsp.size(); });
  const size_t n_cavlc = (size_t) (std::stable_partition (jobs.begin(), jobs.end(), [&] (const Job& a) { return !frames[a.pic]->deferred[a.def].cabac; }) - jobs.begin());
  SliceTask* tasks = (SliceTask*) (A + tasks_at);
  for (size_t p = 0; p < frames.size(); p++) {
    FrameOut& f = *frames[p];
    const lh264_slice_dump::Pic& pc = D->pics[p];
    // what the deferred parser holds already: the records and coefficients of slices parsed on the spot (CABAC), the slice table
    memcpy (A + pc.mbs, f.mbs.data(), f.mbs.size() * sizeof (lh264_mb_t));
    if (f.coeffs.size()) memcpy (A + pc.coeffs, f.coeffs.data(), f.coeffs.size() * 2);
    memcpy (A + pc.slices, f.slices.data(), f.slices.size() * sizeof (lh264_slice_t));
  }
  for (size_t j = 0; j < jobs.size(); j++) {
    const Job& jb = jobs[j];
    FrameOut& f = *frames[jb.pic];
    const DeferredSlice& ds = f.deferred[jb.def];
    const lh264_slice_dump::Pic& pc = D->pics[jb.pic];
    const int n = f.mb_w * f.mb_h;
    SliceTask& t = tasks[j];
    memset (&t, 0, sizeof (t));
    if (!ds.rbsp.empty()) memcpy (A + jb.rbsp, ds.rbsp.data(), ds.rbsp.size());
    memcpy (A + jb.scaling, ds.pps.sl4, 96); memcpy (A + jb.scaling + 96, ds.pps.sl8, 128);
    t.rbsp = B + jb.rbsp; t.rbsp_bytes = (uint32_t)ds.rbsp.size(); t.data_bit = (uint32_t)ds.data_bit;
    t.first_mb = ds.sh.first_mb;
    t.limit_mb = (size_t)ds.sid + 1 < f.slices.size() ? std::min (n, f.slices[(size_t)ds.sid + 1].first_mb) : n;
    if (ds.cabac) t.reserved = (uint8_t) (lh264slice::kTaskCabac | (ds.sh.cabac_init_idc & 3));
    if (tweak && tweak[0] == (int32_t)jb.pic && tweak[1] == ds.sid) { t.limit_mb = tweak[2]; if (tweak[3] >= 0) t.reserved = (uint8_t)tweak[3]; }
    t.mb_w = f.mb_w; t.mb_h = f.mb_h; t.slice_index = ds.sid; t.slice_qp = ds.sh.slice_qp;
    t.slice_type = (uint8_t)ds.sh.slice_type; t.num_ref_idx_l0 = (uint8_t)ds.sh.num_ref_idx_l0;
    t.transform_8x8 = ds.pps.transform_8x8; t.constrained_intra_pred = ds.pps.constrained_intra_pred;
    t.use_sl = ds.sps_scaling || ds.pps.scaling_matrix_present;
    t.chroma_qp_offset[0] = (int8_t)ds.pps.chroma_qp_offset[0]; t.chroma_qp_offset[1] = (int8_t)ds.pps.chroma_qp_offset[1];
    t.scaling = B + jb.scaling;
    t.mbs = (lh264_mb_t*) (B + pc.mbs); t.coeffs = (int16_t*) (B + pc.coeffs);
    t.slice = (lh264_slice_t*) (B + pc.slices) + ds.sid;
    t.line = (int8_t*) (B + jb.line);
  }
  SliceResult* results = (SliceResult*) (A + results_at);
  int rc = LH264_OK;
  if (!on_device) {
    // slices of one picture may run side by side: no two of them write one record
    const lh264slice::Tables& T = slice_tables_host();
    const lh264slice::CabacTables& TC = slice_cabac_tables_host();
    run_parallel ((int)jobs.size(), threads, [&] (int j) {
      alignas (16) lh264_mb_t rec;
      if ((size_t)j < n_cavlc) { results[j] = lh264slice::parse_slice (T, tasks[j], &rec, tasks[j].line); return; }
      uint8_t state[lh264slice::kCabacContexts];
      lh264slice::cabac_init_states (tasks[j], state);
      results[j] = lh264slice::parse_slice_cabac (TC, tasks[j], &rec, (uint8_t*)tasks[j].line, state);
    });
  } else {
    bool ok = hipMemcpy (dev, A, at, hipMemcpyHostToDevice) == hipSuccess &&
              launch_slice_parse ((const SliceTask*) (dev + tasks_at), (SliceResult*) (dev + results_at), (int)n_cavlc, nullptr, -1) &&
              launch_slice_parse_cabac ((const SliceTask*) (dev + tasks_at) + n_cavlc, (SliceResult*) (dev + results_at) + n_cavlc, (int) (jobs.size() - n_cavlc), nullptr, -1) &&
              hipStreamSynchronize (nullptr) == hipSuccess && hipMemcpy (A, dev, at, hipMemcpyDeviceToHost) == hipSuccess;
    hipFree (dev);
    if (!ok) rc = LH264_E_HIP;
  }
  if (rc != LH264_OK) return rc;
  D->guards_ok = true;
  for (auto& g : D->guards) for (size_t q = 0; q < g.second; q++) if (A[g.first + q] != kGuardByte) D->guards_ok = false;
  for (size_t j = 0; j < jobs.size(); j++) {
    const Job& jb = jobs[j];
    int32_t* r = &D->pics[jb.pic].results[(size_t)frames[jb.pic]->deferred[jb.def].sid * 4];
    r[0] = 1; r[1] = results[j].status; r[2] = results[j].n_mbs; r[3] = results[j].stop_bit;
  }
  *out = D.release();
  return LH264_OK;
}
int lh264_slice_dump_pictures (const lh264_slice_dump_t* d) { return d ? (int)d->pics.size() : 0; }
int lh264_slice_dump_picture (const lh264_slice_dump_t* d, int idx, int32_t info[4]) {
  if (!d || !info || idx < 0 || (size_t)idx >= d->pics.size()) return LH264_E_ARG;
  const auto& p = d->pics[(size_t)idx];
  info[0] = p.mb_w; info[1] = p.mb_h; info[2] = p.n_slices; info[3] = p.n_deferred;
  return LH264_OK;
}
const lh264_mb_t* lh264_slice_dump_mbs (const lh264_slice_dump_t* d, int idx) { return d && idx >= 0 && (size_t)idx < d->pics.size() ? (const lh264_mb_t*) (d->arena + d->pics[(size_t)idx].mbs) : nullptr; }
const int16_t* lh264_slice_dump_coeffs (const lh264_slice_dump_t* d, int idx) { return d && idx >= 0 && (size_t)idx < d->pics.size() ? (const int16_t*) (d->arena + d->pics[(size_t)idx].coeffs) : nullptr; }
const lh264_slice_t* lh264_slice_dump_slices (const lh264_slice_dump_t* d, int idx) { return d && idx >= 0 && (size_t)idx < d->pics.size() ? (const lh264_slice_t*) (d->arena + d->pics[(size_t)idx].slices) : nullptr; }
const int32_t* lh264_slice_dump_results (const lh264_slice_dump_t* d, int idx) { return d && idx >= 0 && (size_t)idx < d->pics.size() ? d->pics[(size_t)idx].results.data() : nullptr; }
int lh264_slice_dump_guards_ok (const lh264_slice_dump_t* d) { return d && d->guards_ok ? 1 : 0; }
const char* lh264_slice_dump_error (const lh264_slice_dump_t* d) { return d ? d->error.c_str() : ""; }
void lh264_slice_dump_free (lh264_slice_dump_t* d) { delete d; }

}  // extern "C"
