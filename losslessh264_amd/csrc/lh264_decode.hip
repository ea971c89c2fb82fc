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
#include "lh264_pack.h"

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

// lh264_decode_batch_ex6 with a bilinear or bicubic filter: the planes, RGB and float RGB resampled by the tables filt[job] names.
// places may be null: every window then goes to the whole out_w x out_h picture.  Kernels of their own: every launch above stays as it was
__device__ inline lh264_pack_place_t place_of (const lh264_pack_place_t* places, int out_w, int out_h) {
  return places ? places[blockIdx.x] : lh264_pack_place_t {0, 0, out_w, out_h, 0u, 0u};
}
__global__ void __launch_bounds__ (256) decode_pack_filtered_kernel (const lh264_pack_job_t* __restrict__ jobs, const lh264_pack_place_t* __restrict__ places, const lh264pack::FilterJob* __restrict__ filt, int out_w, int out_h) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  if (j.crop_w <= 0 || j.crop_h <= 0 || (int)blockIdx.y * lh264pack::kBandRows >= out_h) return;
  const lh264pack::FilterJob fj = filt[blockIdx.x];
  lh264pack::pack_band_filtered (j, fj, place_of (places, out_w, out_h), out_w, out_h, (int)blockIdx.y, (int)threadIdx.x, 256);
}
__global__ void __launch_bounds__ (256) decode_pack_rgb_filtered_kernel (const lh264_pack_job_t* __restrict__ jobs, const lh264_pack_place_t* __restrict__ places, const lh264pack::FilterJob* __restrict__ filt, const uint8_t* __restrict__ std, int out_w, int out_h, int layout) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  if (j.crop_w <= 0 || j.crop_h <= 0 || (int)blockIdx.y * lh264pack::kBandRows >= out_h) return;
  const lh264pack::FilterJob fj = filt[blockIdx.x];
  lh264pack::pack_band_rgb_filtered (j, fj, place_of (places, out_w, out_h), out_w, out_h, layout, (int)std[blockIdx.x], (int)blockIdx.y, (int)threadIdx.x, 256);
}
__global__ void __launch_bounds__ (256) decode_pack_sample_filtered_kernel (const lh264_pack_job_t* __restrict__ jobs, const lh264_pack_place_t* __restrict__ places, const lh264pack::FilterJob* __restrict__ filt, const uint8_t* __restrict__ std, int out_w, int out_h, int layout, lh264_decode_sample_t sample) {
  const lh264_pack_job_t j = jobs[blockIdx.x];
  if (j.crop_w <= 0 || j.crop_h <= 0 || (int)blockIdx.y * lh264pack::kBandRows >= out_h) return;
  const lh264pack::FilterJob fj = filt[blockIdx.x];
  lh264pack::pack_band_sample_filtered (j, fj, place_of (places, out_w, out_h), out_w, out_h, layout, (int)std[blockIdx.x], sample, (int)blockIdx.y, (int)threadIdx.x, 256);
}

// ---- the digests: SHA-1 of packed pictures where they lie ---------------------------------------------------------------------------
// One lane per span job, 64 jobs per wave (a message is serial; the width comes from the batch).  The host orders a launch's jobs by
// descending length, so the lanes of a wave end near one another.  No LDS, no wave waits for another; every bound is the job's.
__global__ void __launch_bounds__ (64) sha1_spans_kernel (const lh264_sha1_job_t* __restrict__ jobs, int n) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= n) return;
  lh264sha1::run_job (jobs[i]);
}

// bytes a handle keeps on the device: a run goes behind what is held, on stream st (the buffer grows by doubling)
struct DevGrow {
  uint8_t* p = nullptr; size_t len = 0, cap = 0;
  bool append (const uint8_t* src, size_t bytes, hipStream_t st) {
    if (len + bytes > cap) {
      const size_t want = std::max<size_t> (4 * (len + bytes), (size_t)1 << 16);
      uint8_t* q = nullptr;
      if (hipMalloc ((void**)&q, want) != hipSuccess) return false;
      if (len && hipMemcpyAsync (q, p, len, hipMemcpyDeviceToDevice, st) != hipSuccess) { hipFree (q); return false; }
      if (p) { hipStreamSynchronize (st); hipFree (p); }
      p = q; cap = want;
    }
    if (hipMemcpyAsync (p + len, src, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
    len += bytes;
    return true;
  }
};

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
  long chain_pictures = 0;                      // pictures of the stream that were reconstructed, delivered or not
  std::vector<int32_t> index;                   // per delivered picture: its number among the stream's pictures in decode order
  std::vector<uint8_t> colour;                  // lh264_decode_batch_ex with colour: per delivered picture the standard byte that was applied
  int sample_type = (int)LH264_SAMPLE_U8;       // lh264_decode_batch_ex2: the LH264_SAMPLE_* of the call
  int filter = (int)LH264_FILTER_AREA;          // lh264_decode_batch_ex6: the LH264_FILTER_* of the call
  std::vector<uint8_t> bytes;                  // host mode
  DevGrow dev; int device = 0;                  // LH264_DECODE_DEVICE_OUT
  uint32_t sha = 0;                             // the LH264_DECODE_SHA1_* bits of the call
  std::vector<uint8_t> pic_sha;                 // 20 bytes per delivered picture
  lh264_sha1_state_t stream_state;              // the stream's message behind the last round delivered
  uint8_t stream_sha[20];
  // lh264_decode_batch_ex4 with fields: per delivered picture its geometry and offsets, the stream's motion blocks and macroblock
  // blocks in host memory, or in device memory (LH264_DECODE_DEVICE_OUT)
  uint32_t fields = 0;
  std::vector<lh264_decoded_motion_t> motion_geo;
  std::vector<uint8_t> mot, mbi;
  DevGrow mot_dev, mbi_dev;
  lh264_decoded() { lh264sha1::init (&stream_state); memset (stream_sha, 0, 20); }
  ~lh264_decoded() {
    if (!dev.p && !mot_dev.p && !mbi_dev.p) return;
    int cur = 0;
    hipGetDevice (&cur);
    if (cur != device) hipSetDevice (device);
    for (DevGrow* g : {&dev, &mot_dev, &mbi_dev}) if (g->p) hipFree (g->p);
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
  DevBuf d_filter; PinBuf h_filter[2];  // lh264_decode_batch_ex6 with a filter: a FilterJob per pack job, behind them the weight tables they name
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
  // every buffer of the arena, once: dev (a DevBuf), pin (a PinBuf).  A buffer that is declared above is named here, and nowhere else
  template <typename FD, typename FP> void each_buffer (FD dev, FP pin) const {
    for (const DevBuf* b : {&d_mbs, &d_coef, &d_sparse, &d_sl, &d_jobs, &d_first, &d_pack, &d_out[0], &d_out[1], &d_std, &d_place, &d_filter, &d_mjobs, &d_mot[0], &d_mot[1], &d_mbi[0], &d_mbi[1],
                            &d_sjobs, &d_dig, &d_rec, &d_state, &d_pbytes, &d_ptasks, &d_pres, &d_pmbs, &d_pcoef}) dev (*b);
    for (const PinBuf* two : {h_mbs, h_sparse, h_sl, h_jobs, h_first, h_pack, h_out, h_std, h_place, h_filter, h_mjobs, h_mot, h_mbi, h_sjobs, h_dig}) { pin (two[0]); pin (two[1]); }
    for (const PinBuf* b : {&h_pbytes, &h_ptasks, &h_pres}) pin (*b);
  }
  size_t device_bytes() const { size_t n = pics.bytes; each_buffer ([&] (const DevBuf& b) { n += b.cap; }, [] (const PinBuf&) {}); return n; }
  size_t pinned_bytes() const { size_t n = 0; each_buffer ([] (const DevBuf&) {}, [&] (const PinBuf& b) { n += b.cap; }); return n; }
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
  // lh264_decode_batch_ex5: the walked pictures of the current run that no requested picture has made needed yet (their slices deferred);
  // the walk is over (the last requested picture, or a failure of the header walk, is behind it)
  std::vector<std::unique_ptr<FrameOut>> run_held;
  bool walk_over = false;
  // parse = LH264_PARSE_DEVICE: the stream's CAVLC slices go to slice_parse_kernel (until a CABAC picture or a fallback ends that), and
  // where in the parse arena the records / the slice table of the pictures parsed there in this round lie
  bool dev_route = false;
  struct DevAt { size_t mb; };
  std::map<const FrameOut*, DevAt> dev_at;
};

// what the call delivers for a picture: the source rectangle in its window, the destination rectangle in the ow x oh picture, its bytes
struct PicPlan { lh264_rect_t src, dst; int ow, oh; size_t bytes; };
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
  std::vector<PicPlan> plan;                         // per picture of the round, withheld ones included (plan_round: staging reads it)
};
struct Round { std::vector<RoundChain> chains; size_t out_bytes = 0, dig_states_at = 0, mot_bytes = 0, mbi_bytes = 0; bool live = false, timed = false; };

// lh264_decode_batch_ex5: one stream's entry (the rule: include/lh264.h at that call)
struct Selection {
  const int32_t* list = nullptr; uint32_t n_list = 0, first = 0, count = 0, step = 1;
  explicit Selection (const lh264_select_t& e) : list (e.list), n_list (e.n_list), first (e.first), count (e.count), step (e.step) {}
  bool requested (long k) const {
    if (list) return k <= 0x7fffffffl && std::binary_search (list, list + n_list, (int32_t)k);
    return k >= (long)first && (k - (long)first) % (long)step == 0 && (count == 0 || (k - (long)first) / (long)step < (long)count);
  }
  // the last requested number: -1 for none, the largest long for "to the stream's end"
  long last() const {
    if (list) return n_list ? (long)list[n_list - 1] : -1;
    return count ? (long)first + (long) (count - 1) * (long)step : 0x7fffffffffffffffl;
  }
};
bool select_entry_ok (const lh264_select_t& e) {
  if (!e.list) return e.n_list == 0 && e.step >= 1;
  for (uint32_t k = 0; k < e.n_list; k++) if (e.list[k] < 0 || (k && e.list[k] <= e.list[k - 1])) return false;
  return true;
}

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

// ---- the pack launch: one descriptor, one ladder over the eleven kernels -----------------------------------------------------------
// what every entry point asks of a pack job: planes and a destination, an even window of up to max_side a side at an even place, I420
// or NV12, reserved (the job's scale) in 0..max_reserved.  A caller's stricter conditions stand beside its call
struct PackLimits { int max_side, max_reserved; };
const int kAnySide = 0x7fffffff, kFrontEndSide = 16384;      // lh264_debug_pack_*: no cap; the others: what the front end can deliver
bool pack_job_ok (const lh264_pack_job_t& j, PackLimits lim) {
  return j.y && j.u && j.v && j.dst && j.crop_w > 0 && j.crop_h > 0 && j.crop_w <= lim.max_side && j.crop_h <= lim.max_side && !((j.crop_w | j.crop_h | j.crop_x | j.crop_y) & 1) &&
         j.crop_x >= 0 && j.crop_y >= 0 && (j.format == LH264_FMT_I420 || j.format == LH264_FMT_NV12) && j.reserved >= 0 && j.reserved <= lim.max_reserved;
}
int bands_of (int rows) { return (rows + lh264pack::kBandRows - 1) / lh264pack::kBandRows; }

// one launch of a pack kernel over n jobs: the tables (places: LH264_FIT_CONTAIN, else null; std: with a colour), the grid's bands, the
// given size or 0, 0, the colour layout or 0, the scale all jobs share, and the sample struct of a float type or null
struct PackLaunch {
  const lh264_pack_job_t* jobs; const lh264_pack_place_t* places; const uint8_t* std;
  int n, max_bands, out_w, out_h, colour, scale;
  const lh264_decode_sample_t* sample;
  const lh264pack::FilterJob* filt;     // lh264_decode_batch_ex6 with a bilinear or bicubic filter: the jobs' tables; else null
};
bool launch_pack (const PackLaunch& p, hipStream_t st) {
  const dim3 grid ((unsigned)p.n, (unsigned)p.max_bands), wg (256);
  if (p.filt && p.sample) hipLaunchKernelGGL (decode_pack_sample_filtered_kernel, grid, wg, 0, st, p.jobs, p.places, p.filt, p.std, p.out_w, p.out_h, p.colour, *p.sample);
  else if (p.filt && p.colour) hipLaunchKernelGGL (decode_pack_rgb_filtered_kernel, grid, wg, 0, st, p.jobs, p.places, p.filt, p.std, p.out_w, p.out_h, p.colour);
  else if (p.filt) hipLaunchKernelGGL (decode_pack_filtered_kernel, grid, wg, 0, st, p.jobs, p.places, p.filt, p.out_w, p.out_h);
  else if (p.places && p.sample) hipLaunchKernelGGL (decode_pack_sample_placed_kernel, grid, wg, 0, st, p.jobs, p.places, p.std, p.out_w, p.out_h, p.colour, *p.sample);
  else if (p.places && p.colour) hipLaunchKernelGGL (decode_pack_rgb_placed_kernel, grid, wg, 0, st, p.jobs, p.places, p.std, p.out_w, p.out_h, p.colour);
  else if (p.places) hipLaunchKernelGGL (decode_pack_placed_kernel, grid, wg, 0, st, p.jobs, p.places, p.out_w, p.out_h);
  else if (p.sample) hipLaunchKernelGGL (decode_pack_sample_kernel, grid, wg, 0, st, p.jobs, p.std, p.out_w, p.out_h, p.colour, *p.sample);
  else if (p.colour) hipLaunchKernelGGL (decode_pack_rgb_kernel, grid, wg, 0, st, p.jobs, p.std, p.out_w, p.out_h, p.colour);
  else if (p.out_w) hipLaunchKernelGGL (decode_pack_resized_kernel, grid, wg, 0, st, p.jobs, p.out_w, p.out_h);
  else if (p.scale) hipLaunchKernelGGL (decode_pack_scaled_kernel, grid, wg, 0, st, p.jobs);
  else hipLaunchKernelGGL (decode_pack_kernel, grid, wg, 0, st, p.jobs);
  return hipGetLastError() == hipSuccess;
}
// ... and of decode_pack_motion_kernel: units, the most (row, chunk) pairs of one job
bool launch_motion (const lh264_motion_job_t* jobs, int n, int units, hipStream_t st) {
  hipLaunchKernelGGL (decode_pack_motion_kernel, dim3 ((unsigned)n, (unsigned)units), dim3 (256), 0, st, jobs);
  return hipGetLastError() == hipSuccess;
}
// ---- the filter tables: lh264_decode_batch_ex6 (the definition: include/lh264.h at that call) -----------------------------------------
// One axis: src_len source samples delivered as dst_len, every delivered coordinate's taps by the definition.  The raw weights reach
// 2^48 and their scaled quotients need more than 64 bits: 128-bit integers, here and nowhere on the device.  ent gets {first, count,
// offset into k} per coordinate, k the weights, zero weights at a row's ends trimmed.  false: a property the kernels rely on does not
// hold (a weight outside int16, a row whose absolute weights times 255 leave int32) - no shape in range is known to do that
bool filter_axis (uint32_t filter, int src_len, int dst_len, std::vector<int32_t>* ent, std::vector<int16_t>* k) {
  typedef __int128 wide;
  const int64_t w = src_len, ow = dst_len, m = 2 * std::max (w, ow), support = filter == LH264_FILTER_BILINEAR ? m : 2 * m;
  auto floor_div = [] (int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && (a < 0)) ? q - 1 : q; };      // (b > 0)
  std::vector<int64_t> r;
  std::vector<int32_t> kk;
  for (int64_t X = 0; X < ow; X++) {
    const int64_t c = (2 * X + 1) * w - ow;                                   // n (x) = |2*ow*x - c|
    const int64_t x0 = std::max<int64_t> (0, floor_div (c - support, 2 * ow) + 1), x1 = std::min<int64_t> (w - 1, floor_div (c + support - 1, 2 * ow));
    if (x1 < x0) return false;
    r.clear();
    wide R = 0;
    size_t best = 0;
    for (int64_t x = x0; x <= x1; x++) {
      const int64_t d = 2 * ow * x - c, n = d < 0 ? -d : d;
      int64_t v;
      if (filter == LH264_FILTER_BILINEAR) v = n < m ? m - n : 0;
      else v = n < m ? 3 * n * n * n - 5 * n * n * m + 2 * m * m * m : n < 2 * m ? -n * n * n + 5 * n * n * m - 8 * n * m * m + 4 * m * m * m : 0;
      if (!r.empty() && v > r[best]) best = r.size();                         // (the largest, the lowest x among equals)
      r.push_back (v);
      R += v;
    }
    if (R <= 0) return false;
    kk.assign (r.size(), 0);
    int64_t sum = 0;
    for (size_t i = 0; i < r.size(); i++) {
      const wide num = ((wide)r[i] << 15) + R, den = 2 * R;
      wide q = num / den;
      if (num % den != 0 && num < 0) q--;                                     // floor, toward minus infinity
      kk[i] = (int32_t)q;
      sum += kk[i];
    }
    kk[best] += (int32_t) (16384 - sum);
    size_t a = 0, b = kk.size();
    while (a < b && kk[a] == 0) a++;
    while (b > a && kk[b - 1] == 0) b--;
    int64_t mag = 0;
    for (size_t i = a; i < b; i++) { if (kk[i] < -32768 || kk[i] > 32767) return false; mag += kk[i] < 0 ? -kk[i] : kk[i]; }
    if (a == b || mag * 255 > 0x7fffffff) return false;
    ent->push_back ((int32_t) (x0 + (int64_t)a)); ent->push_back ((int32_t) (b - a)); ent->push_back ((int32_t)k->size());
    for (size_t i = a; i < b; i++) k->push_back ((int16_t)kk[i]);
  }
  return true;
}
// the tables of one call: one per distinct (src_len, dst_len), laid out one behind the other as the device reads them - 3 * dst_len
// int32 entries, then the int16 weights, padded to 4 bytes
struct FilterPlan {
  uint32_t filter = LH264_FILTER_AREA;
  std::map<std::pair<int, int>, size_t> at;     // where the table of a geometry begins in blob
  std::vector<uint8_t> blob;
  bool add (int src_len, int dst_len) {
    if (at.count ({src_len, dst_len})) return true;
    std::vector<int32_t> ent; std::vector<int16_t> k;
    if (!filter_axis (filter, src_len, dst_len, &ent, &k)) return false;
    if (k.size() & 1) k.push_back (0);
    const size_t off = blob.size();
    blob.resize (off + ent.size() * 4 + k.size() * 2);
    memcpy (&blob[off], ent.data(), ent.size() * 4);
    memcpy (&blob[off + ent.size() * 4], k.data(), k.size() * 2);
    at[{src_len, dst_len}] = off;
    return true;
  }
  // the four tables of a job whose w x h window is resampled to pw x ph (all even)
  bool add_job (int w, int h, int pw, int ph) { return add (w, pw) && add (h, ph) && add (w >> 1, pw >> 1) && add (h >> 1, ph >> 1); }
  lh264pack::FilterAxis axis (const uint8_t* base, int src_len, int dst_len) const {
    const uint8_t* t = base + at.at ({src_len, dst_len});
    return {(const int32_t*)t, (const int16_t*) (t + (size_t)dst_len * 12)};
  }
  // ... as the job's record, the blob lying (or going to lie) at base
  lh264pack::FilterJob job (const uint8_t* base, int w, int h, int pw, int ph) const {
    return {axis (base, w, pw), axis (base, h, ph), axis (base, w >> 1, pw >> 1), axis (base, h >> 1, ph >> 1)};
  }
};

// the lh264_debug_*_dev entry points: the host tables p names go up, one launch on the null stream is waited for, the tables go
// (fp: the filter tables of a filtered launch, whose job records p.filt were written for a blob at address 0)
bool upload (DevBuf& d, const void* src, size_t bytes) { return d.alloc (bytes) && hipMemcpy (d.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess; }
int debug_launch (PackLaunch p, const FilterPlan* fp = nullptr) {
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  if (!p.n) return LH264_OK;
  DevBuf d_jobs, d_places, d_std, d_blob, d_filt;
  bool ok = upload (d_jobs, p.jobs, (size_t)p.n * sizeof (lh264_pack_job_t)) && (!p.places || upload (d_places, p.places, (size_t)p.n * sizeof (lh264_pack_place_t))) && (!p.std || upload (d_std, p.std, (size_t)p.n));
  if (ok && fp) {
    ok = upload (d_blob, fp->blob.data(), fp->blob.size());
    std::vector<lh264pack::FilterJob> rec (p.filt, p.filt + p.n);
    const uintptr_t base = (uintptr_t)d_blob.p;
    for (lh264pack::FilterJob& f : rec) for (lh264pack::FilterAxis* a : {&f.lx, &f.ly, &f.cx, &f.cy}) { a->ent = (const int32_t*) ((uintptr_t)a->ent + base); a->k = (const int16_t*) ((uintptr_t)a->k + base); }
    ok = ok && upload (d_filt, rec.data(), rec.size() * sizeof (lh264pack::FilterJob));
    p.filt = d_filt.as<lh264pack::FilterJob>();
  }
  p.jobs = d_jobs.as<lh264_pack_job_t>(); p.places = d_places.as<lh264_pack_place_t>(); p.std = d_std.as<uint8_t>();      // (null where none went up)
  ok = ok && launch_pack (p, nullptr) && hipStreamSynchronize (nullptr) == hipSuccess;
  return ok ? LH264_OK : LH264_E_HIP;
}

// a sample struct the call takes: 32 bytes, a type that is defined, with LH264_SAMPLE_U8 six floats whose bits are all clear, with a
// float type six finite floats
bool sample_ok (const lh264_decode_sample_t* s) {
  if (s->struct_bytes != sizeof (lh264_decode_sample_t) || s->type > LH264_SAMPLE_BF16) return false;
  for (int k = 0; k < 6; k++) {
    uint32_t x;
    memcpy (&x, k < 3 ? &s->mul[k] : &s->add[k - 3], 4);
    if (s->type == LH264_SAMPLE_U8 ? x != 0 : (x & 0x7f800000u) == 0x7f800000u) return false;
  }
  return true;
}

// ---- the call's configuration: every argument check and every derived value, once; no device is touched -----------------------------
struct DecodeConfig {
  int format, conceal;
  uint32_t parse; bool parse_dev, parse_cabac;      // slice data goes to slice_parse_kernel (not with concealment, which builds records on the host); CABAC slices too
  int scale;                                        // 0: decode_pack_kernel; 1..3: decode_pack_scaled_kernel
  uint32_t pick; bool picking;                      // unselected pictures are walked by their headers only, every selected one is a chain
  std::vector<Selection> selects; bool selecting;   // lh264_decode_batch_ex5: every stream's entry; only needed pictures are decoded, a run is a chain
  bool sparse;                                      // picking or selecting: every slice is deferred, pictures leave the stream unparsed
  int out_w, out_h;                                 // 0, 0: the window (or its scale); else decode_pack_resized_kernel
  uint32_t fit, fill; std::vector<lh264_rect_t> crops;      // the view: the fit, the bars' fill, and every stream's crop (w = 0: none)
  bool placed;                                      // LH264_FIT_CONTAIN: the placed kernels and a place per pack job
  uint32_t filter;                                  // LH264_FILTER_AREA: the kernels above; else the filtered kernels and a FilterJob per pack job
  int colour; uint32_t matrix, range;               // 0: the planes; else decode_pack_rgb_kernel, 3 bytes per delivered luma sample
  int stype; size_t es; lh264_decode_sample_t sample;       // 0: bytes; else decode_pack_sample_kernel in decode_pack_rgb_kernel's place, es bytes per element
  uint32_t fields, sha_bits;                        // fields 0: the call is lh264_decode_batch_ex3; else decode_pack_motion_kernel gathers the round's records
  bool device_out, no_pictures, sha_pics, sha_stream, sha;
  bool motion_only, down;                           // no pool, no reconstruct, pack or digest kernel; the round has bytes to bring down on the second stream
  lh264_decode_sink_fn sink; void* user;
  size_t R, group_mbs;
  // what the call delivers for a picture of stream i whose window is w x h (a picture select let through: the crop fits)
  PicPlan plan (int w, int h, int i) const {
    PicPlan v;
    view_of (w, h, crops[i], fit, scale, out_w, out_h, &v.src, &v.dst, &v.ow, &v.oh);
    v.bytes = colour ? (size_t)v.ow * v.oh * 3 * es : (size_t)v.ow * v.oh * 3 / 2;
    return v;
  }
  // the picture's standard byte (0 without a colour), and whether it is defined: if not, the stream stops at the picture
  uint8_t standard (const FrameOut& f) const { return colour ? picture_standard (f, matrix, range) : 0; }
  bool standard_defined (const FrameOut& f) const { return standard (f) <= 3; }
};

// LH264_OK, or LH264_E_ARG for arguments the call does not take
int decode_config (const lh264_decode_opts_t* opts, const lh264_decode_ext_t* ext, const lh264_decode_sample_t* sample, const lh264_decode_view_t* view, const lh264_decode_motion_t* motion, const lh264_decode_select_t* select, const lh264_decode_filter_t* filter, int n, DecodeConfig* cfg) {
  DecodeConfig& c = *cfg;
  if (filter && (filter->struct_bytes != sizeof (lh264_decode_filter_t) || filter->filter > LH264_FILTER_BICUBIC || filter->reserved0 != 0 || filter->reserved1 != 0)) return LH264_E_ARG;
  c.filter = filter ? filter->filter : LH264_FILTER_AREA;
  if (select && (select->struct_bytes != sizeof (lh264_decode_select_t) || select->reserved != 0 || (select->n_selects != 0 && select->n_selects != 1 && select->n_selects != (uint32_t)n) ||
                 (select->n_selects != 0 && !select->selects))) return LH264_E_ARG;
  if (select) for (uint32_t k = 0; k < select->n_selects; k++) if (!select_entry_ok (select->selects[k])) return LH264_E_ARG;
  c.selecting = select && select->n_selects;
  c.selects.clear();
  if (c.selecting) for (int i = 0; i < n; i++) c.selects.push_back (Selection (select->selects[select->n_selects == 1 ? 0 : i]));
  if (motion && (motion->struct_bytes != sizeof (lh264_decode_motion_t) || motion->fields > LH264_MOTION_FIELDS || motion->reserved0 != 0 || motion->reserved1 != 0)) return LH264_E_ARG;
  c.fields = motion ? motion->fields : 0;
  if (view && (view->struct_bytes != sizeof (lh264_decode_view_t) || view->fit > LH264_FIT_CONTAIN || view->reserved0 != 0 || view->reserved1 != 0 ||
               (view->fill && (view->fit != LH264_FIT_CONTAIN || view->fill >> 24)) || (view->n_crops != 0 && view->n_crops != 1 && view->n_crops != (uint32_t)n) ||
               (view->n_crops != 0 && !view->crops))) return LH264_E_ARG;
  if (view) for (uint32_t k = 0; k < view->n_crops; k++) if (!crop_ok (view->crops[k])) return LH264_E_ARG;
  c.fit = view ? view->fit : LH264_FIT_STRETCH; c.fill = view ? view->fill : 0;
  c.crops.assign ((size_t)n, lh264_rect_t {0, 0, 0, 0});
  if (view && view->n_crops) for (int i = 0; i < n; i++) c.crops[i] = view->crops[view->n_crops == 1 ? 0 : i];
  if (ext && ext->struct_bytes != sizeof (lh264_decode_ext_t)) return LH264_E_ARG;      // (before ext->colour is read below)
  if (sample && (!sample_ok (sample) || (sample->type != LH264_SAMPLE_U8 && (!ext || ext->colour == LH264_COLOUR_YUV)))) return LH264_E_ARG;
  c.stype = sample ? (int)sample->type : (int)LH264_SAMPLE_U8;
  c.es = c.stype == (int)LH264_SAMPLE_U8 ? 1 : c.stype == (int)LH264_SAMPLE_F32 ? 4 : 2;
  memset (&c.sample, 0, sizeof (c.sample));
  if (sample) c.sample = *sample;
  if (ext && (ext->colour > LH264_COLOUR_RGBP || ext->matrix > LH264_MATRIX_BT709 || ext->range > LH264_RANGE_FULL ||
              ext->reserved0 != 0 || ext->reserved1 != 0 || (ext->colour == LH264_COLOUR_YUV && (ext->matrix != LH264_MATRIX_AUTO || ext->range != LH264_RANGE_AUTO)) ||
              (ext->colour != LH264_COLOUR_YUV && opts && opts->format != LH264_FMT_I420))) return LH264_E_ARG;
  c.colour = ext ? (int)ext->colour : 0;
  c.matrix = ext ? ext->matrix : LH264_MATRIX_AUTO; c.range = ext ? ext->range : LH264_RANGE_AUTO;
  const uint32_t flags = opts ? opts->flags : 0, bytes = opts ? opts->struct_bytes : 0;
  c.sha_bits = flags & (LH264_DECODE_SHA1_PICTURES | LH264_DECODE_SHA1_STREAM);
  if (opts && ((bytes != sizeof (lh264_decode_opts_t) && bytes != LH264_DECODE_OPTS_BYTES_V5 && bytes != LH264_DECODE_OPTS_BYTES_V4 && bytes != LH264_DECODE_OPTS_BYTES_V3 && bytes != LH264_DECODE_OPTS_BYTES_V2 && bytes != LH264_DECODE_OPTS_BYTES_V1) ||
               opts->format > LH264_FMT_NV12 || (flags & ~ (LH264_DECODE_DEVICE_OUT | LH264_DECODE_SHA1_PICTURES | LH264_DECODE_SHA1_STREAM | LH264_DECODE_NO_PICTURES)) ||
               (opts->sink && (flags & LH264_DECODE_DEVICE_OUT)) ||
               ((flags & LH264_DECODE_NO_PICTURES) && ((!c.fields && (!c.sha_bits || (flags & LH264_DECODE_DEVICE_OUT))) || opts->sink)))) return LH264_E_ARG;
  c.conceal = bytes >= LH264_DECODE_OPTS_BYTES_V2 ? (int)opts->conceal : 0;
  c.parse = bytes >= LH264_DECODE_OPTS_BYTES_V3 ? opts->parse : LH264_PARSE_HOST;
  if (c.parse != LH264_PARSE_HOST && c.parse != LH264_PARSE_DEVICE) return LH264_E_ARG;
  const uint32_t parse_flags = bytes >= LH264_DECODE_OPTS_BYTES_V3 ? opts->parse_flags : 0;
  if ((parse_flags & ~LH264_PARSE_FLAG_CABAC) || (parse_flags && c.parse != LH264_PARSE_DEVICE)) return LH264_E_ARG;
  c.parse_dev = c.parse == LH264_PARSE_DEVICE && c.conceal == 0;
  c.parse_cabac = c.parse_dev && (parse_flags & LH264_PARSE_FLAG_CABAC);
  const bool v4 = bytes >= LH264_DECODE_OPTS_BYTES_V4, v5 = bytes >= LH264_DECODE_OPTS_BYTES_V5, v6 = bytes == sizeof (lh264_decode_opts_t);
  if (v4 && (opts->scale_log2 > 3 || opts->reserved2 != 0)) return LH264_E_ARG;
  c.scale = v4 ? (int)opts->scale_log2 : 0;
  if (v5 && (opts->pick > LH264_PICK_IDR || opts->reserved3 != 0 || (opts->pick != LH264_PICK_ALL && c.conceal != 0))) return LH264_E_ARG;
  c.pick = v5 ? opts->pick : LH264_PICK_ALL;
  c.picking = c.pick != LH264_PICK_ALL;
  if (c.selecting && (c.picking || c.conceal != 0)) return LH264_E_ARG;
  c.sparse = c.picking || c.selecting;
  const bool sized = v6 && (opts->out_width || opts->out_height);
  if (v6 && (opts->reserved4 != 0 || opts->reserved5 != 0 || (sized && (!lh264pack::size_ok (opts->out_width, opts->out_height) || c.scale != 0)))) return LH264_E_ARG;
  c.out_w = sized ? (int)opts->out_width : 0; c.out_h = sized ? (int)opts->out_height : 0;
  if (c.fit != LH264_FIT_STRETCH && !c.out_w) return LH264_E_ARG;
  if (c.filter != LH264_FILTER_AREA && !c.out_w) return LH264_E_ARG;
  c.placed = c.fit == LH264_FIT_CONTAIN;
  if (!Parser::conceal_method_ok (c.conceal)) return LH264_E_ARG;           // a method that is not provided (FRAME_COPY), or no method at all
  c.format = opts ? (int)opts->format : LH264_FMT_I420;
  c.device_out = flags & LH264_DECODE_DEVICE_OUT;
  c.no_pictures = flags & LH264_DECODE_NO_PICTURES;                       // digests or fields only: no picture is downloaded or kept
  c.sha_pics = flags & LH264_DECODE_SHA1_PICTURES; c.sha_stream = flags & LH264_DECODE_SHA1_STREAM;
  c.sha = c.sha_pics || c.sha_stream;
  c.motion_only = c.fields && c.no_pictures && !c.sha;
  c.down = !c.device_out && (!c.no_pictures || c.fields);
  c.sink = opts ? opts->sink : nullptr; c.user = opts ? opts->user : nullptr;
  c.R = opts && opts->round_pictures ? opts->round_pictures : kDefaultRoundPictures;
  c.group_mbs = opts && opts->group_mbs ? (size_t)opts->group_mbs : (size_t)kDefaultGroupMbs;
  return LH264_OK;
}

// ---- the call: rounds of admit -> fill_and_select (-> device_parse) -> plan_round -> stage_round -> enqueue_round -> deliver ----------
struct DecodeCall {
  const DecodeConfig& cfg;
  Arena& A;
  const uint8_t* const* data; const size_t* len; const int n, threads;
  lh264_decoded_t** out;
  std::vector<std::unique_ptr<DStream>> active, retired;      // retired: streams that are through (a round on the device still names them)
  int next_stream = 0;
  const int kWave = std::max (8, 4 * threads);
  Round rounds[2];
  int rb = 0;                                       // the buffers the next round takes
  bool device_failed = false;
  std::string device_error;
  // LH264_SLICE_PARSE_FAIL=k (tests): task k of the call's first parse launch reports a status unwalked, which forces the fallback;
  // LH264_SLICE_PARSE_FAIL_CABAC=k: the same for task k of the call's first CABAC launch
  int force_fail = cfg.parse_dev && getenv ("LH264_SLICE_PARSE_FAIL") ? atoi (getenv ("LH264_SLICE_PARSE_FAIL")) : -1;
  int force_fail_cabac = cfg.parse_cabac && getenv ("LH264_SLICE_PARSE_FAIL_CABAC") ? atoi (getenv ("LH264_SLICE_PARSE_FAIL_CABAC")) : -1;
  const double t_call = now_s();
  double t_parse = 0, t_stage = 0, t_enqueue = 0, t_wait = 0, t_deliver = 0, t_dev_parse = 0, n_dev_slices = 0;
  double motion_ms = 0; unsigned long long motion_bytes = 0;        // lh264_decode_last_motion
  long long n_rounds = 0, n_launched = 0, n_launched_jobs = 0;      // lh264_decode_last_chains
  // the round in preparation, plan_round to enqueue_round: where each chain's records, slices, entries and jobs begin, its pictures'
  // slots, the round's counts.  n_hmbs: the macroblocks whose records the host stages (not those in the parse arena); n_mjobs,
  // max_units: the round's motion jobs (its delivered pictures), the most chunks of one of them
  struct Place { size_t mb0, sl0, sp0, job0; };
  std::vector<Place> place;
  std::vector<std::vector<int>> slot_of;
  FilterPlan filters {cfg.filter, {}, {}};                            // a filter: the tables of every geometry the call has met so far
  size_t n_hmbs = 0, n_sl = 0, n_sp = 0, n_jobs = 0, n_out = 0, n_mjobs = 0, n_sjobs = 0, dig_bytes = 0;
  int n_launch = 0, max_units = 1, max_w = 1, max_h = 1, max_bands = 1;
  std::vector<int32_t> chain_first;                // the round's jobs that begin a chain of the lh264_recon_chains launch

  void release_pool (DStream& s) {
    for (Slot& sl : s.pool) A.pics.put (s.geo.bytes, sl.base);
    s.pool.clear();
  }
  void retire (DStream& s) {                        // the stream leaves: its result stands, its memory goes back
    lh264_decoded_t& r = *out[s.i];
    if (r.status == LH264_OK && device_failed) { r.status = LH264_E_HIP; r.error = device_error; }
    if (r.status == LH264_OK && s.end_code != LH264_OK) { r.status = s.end_code; r.error = s.end_text; }
    release_pool (s);
    s.parser.reset(); s.pending.clear(); s.sel.clear();
  }
  void unselect (DStream& s) {                      // the round was full: the pictures wait for the next one
    for (size_t q = s.sel.size(); q-- > 0; ) s.pending.push_front (std::move (s.sel[q]));
    s.sel.clear(); s.ending = false;
  }
  void fail_device (const std::string& what) {
    device_failed = true; device_error = what;
    const char* he = hipGetErrorString (hipGetLastError());
    if (he && *he) device_error += std::string (" (") + he + ")";
  }

  // who takes part: streams that are through leave, new ones are admitted while the round has room.  false: the call is over
  bool admit() {
    for (size_t k = 0; k < active.size(); ) {
      DStream& s = *active[k];
      if (s.stopped || s.ending) { retire (s); retired.push_back (std::move (active[k])); active.erase (active.begin() + (long)k); } else k++;
    }
    if (device_failed) return false;
    size_t known = 0, known_mbs = 0;
    for (auto& s : active) if (s->pic_mbs) { known++; known_mbs += s->pic_mbs; }
    const size_t avg = known ? std::max<size_t> (1, known_mbs / known) : 396;
    size_t used = 0;
    for (auto& s : active) used += (s->pic_mbs ? s->pic_mbs : avg) * cfg.R;
    int admitted = 0;
    while (next_stream < n && (active.empty() || used + avg * cfg.R <= cfg.group_mbs) && (known || admitted < kWave)) {
      std::unique_ptr<DStream> s (new DStream());
      s->i = next_stream++;
      s->dev_route = cfg.parse_dev;
      s->walk_over = cfg.selecting && cfg.selects[s->i].last() < 0;      // (an empty list: nothing of the stream is read)
      Parser& P = * (s->parser = std::make_unique<Parser>());
      P.set_sparse_coeffs (true); P.set_sparse_levels (true);       // (the parser has no mode without levels: their list is the cheapest form)
      P.set_conceal (cfg.conceal);
      P.set_defer_slice_data (cfg.parse_dev || cfg.sparse); P.set_defer_cabac (cfg.parse_cabac || cfg.sparse);
      P.begin_file (data[s->i], data[s->i] ? len[s->i] : 0);
      active.push_back (std::move (s));
      used += avg * cfg.R; admitted++;
    }
    return !active.empty();
  }

  // lh264_decode_batch_ex5, a walked picture: an entry (an IDR picture; picture 0 has nothing in front of it) drops what is held, a
  // requested picture makes everything held needed - the others of them reconstructed only - and behind the last requested picture,
  // or at a failure of the header walk, the walk is over
  void hold_or_promote (DStream& s, std::unique_ptr<FrameOut> f) {
    const Selection& q = cfg.selects[s.i];
    const Parser& P = *s.parser;
    if (s.walk_over) return;
    if (!P.error().empty() && f->index >= P.error_pictures()) { s.walk_over = true; s.run_held.clear(); return; }
    if (f->idr) s.run_held.clear();
    const long k = f->index;
    s.run_held.push_back (std::move (f));
    if (q.requested (k)) {
      for (auto& h : s.run_held) { h->frozen = h->index != k; s.pending.push_back (std::move (h)); }
      s.run_held.clear();
    }
    if (k >= q.last()) { s.walk_over = true; s.run_held.clear(); }
  }

  // host threads: parse until the stream has a round's pictures (or ends), then pick the round's pictures
  // tentative (a stream on the device route): the round's candidates, before their slice data is parsed - nothing is refused yet
  void fill_and_select (DStream& s, bool fill, bool tentative) {
    Parser& P = *s.parser;
    const size_t R = cfg.R;
    while (fill && s.pending.size() < R && !P.file_finished() && !s.walk_over) {
      const size_t want = s.pic_mbs ? (R - s.pending.size()) * s.pic_mbs - 1 : 0;
      P.feed_file_some (want);
      for (auto& f : P.frames()) {
        s.pic_mbs = (size_t)f->mb_w * f->mb_h;
        s.seen = f->index + 1;
        // (slices parsed on the spot; the deferred ones are counted where they are resolved)
        out[s.i]->parsed_slices += (long) (f->slices.size() - f->deferred.size());
        // opts->pick: an unselected picture leaves here, its slice data unseen
        if (cfg.picking && !picture_selected (*f, cfg.pick)) continue;
        if (cfg.selecting) { hold_or_promote (s, std::move (f)); continue; }
        s.pending.push_back (std::move (f));
      }
      P.frames().clear();
      if (cfg.selecting && !P.error().empty()) { s.walk_over = true; s.run_held.clear(); }      // (what the failure means is decided below)
    }
    s.ending = false; s.end_code = LH264_OK; s.end_text.clear();
    // (lh264_decode_batch_ex5: a failure behind the last requested picture is not the call's)
    const bool has_err = !tentative && !P.error().empty() && (!cfg.selecting || P.error_pictures() <= cfg.selects[s.i].last());
    const long limit = has_err ? P.error_pictures() : 0x7fffffffffffffffl;
    while (s.sel.size() < R) {
      // the picture's number in the stream: with opts->pick the next selected picture's own, or where the pictures seen so far end
      const long idx = !cfg.sparse ? s.next_picture + (long)s.sel.size() : !s.pending.empty() ? s.pending.front()->index : has_err ? limit : s.seen;
      if (idx >= limit) { s.ending = true; s.end_code = LH264_E_UNSUPPORTED; s.end_text = "picture " + std::to_string (cfg.sparse ? limit : idx) + ": " + P.error(); break; }
      if (s.pending.empty()) {
        if (P.file_finished() || s.walk_over) { s.ending = true; if (has_err) { s.end_code = LH264_E_UNSUPPORTED; s.end_text = P.error(); } }
        break;
      }
      FrameOut& f = *s.pending.front();
      // a change of resolution ends the round: the next one starts with a new pool.  (Asked first: on the device route the tentative
      // pass stopped here too, so the picture's slice data is not parsed yet and there is nothing to refuse it by)
      if (!s.sel.empty() && (f.mb_w != s.sel[0]->mb_w || f.mb_h != s.sel[0]->mb_h)) break;
      std::string why = tentative ? std::string() : refuse_picture (f);
      if (!tentative && why.empty() && !cfg.standard_defined (f)) why = "matrix_coefficients " + std::to_string (f.matrix_coefficients) + " has no conversion here (BT.601: 5, 6, 2 or none; BT.709: 1): name a matrix";
      if (!why.empty()) { s.ending = true; s.end_code = LH264_E_UNSUPPORTED; s.end_text = "picture " + std::to_string (idx) + ": " + why; break; }
      // the caller's crop against this picture's window (a stream may change size): the stream stops here, as for the matrix
      const lh264_rect_t& cr = cfg.crops[s.i];
      if (!tentative && cr.w && !crop_fits (cr, f.crop_w, f.crop_h)) {
        s.ending = true; s.end_code = LH264_E_ARG;
        s.end_text = "picture " + std::to_string (idx) + ": the crop {" + std::to_string (cr.x) + ", " + std::to_string (cr.y) + ", " + std::to_string (cr.w) + ", " + std::to_string (cr.h) +
                     "} does not fit the picture's " + std::to_string (f.crop_w) + " x " + std::to_string (f.crop_h) + " window";
        break;
      }
      s.sel.push_back (std::move (s.pending.front())); s.pending.pop_front();
    }
  }

  // ---- the round's deferred slice data on the device: payloads and tasks up, slice_parse_kernel (and its CABAC sibling), 12 bytes per
  // slice down; then the round's pictures are picked as ever.  On the run stream, behind the round before (whose kernels still read the
  // parse arena), and waited for: the results decide what the round holds.  false: the stage failed, nothing is selected
  struct TRef { DStream* s; FrameOut* f; size_t def, bytes_at; };
  bool device_parse() {
    const double t_p0 = now_s();
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
        if (cfg.sparse && !cfg.parse_cabac && f.deferred[0].cabac) { s.dev_route = false; continue; }
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
    if (nt) {
      bool ok = A.d_pbytes.alloc (pb) && A.h_pbytes.alloc (pb) && A.d_ptasks.alloc (nt * sizeof (lh264host::SliceTask)) && A.h_ptasks.alloc (nt * sizeof (lh264host::SliceTask)) &&
                A.d_pres.alloc (nt * sizeof (lh264host::SliceResult)) && A.h_pres.alloc (nt * sizeof (lh264host::SliceResult)) &&
                A.d_pmbs.alloc (pm * sizeof (lh264_mb_t)) && A.d_pcoef.alloc (pm * 768);
      if (ok) {
        lh264host::SliceTask* ht = A.h_ptasks.as<lh264host::SliceTask>();
        run_parallel ((int)nt, threads, [&] (int j) { slice_task (refs[(size_t)j], ht[j]); });
        hipStream_t st = A.s_run;
        ok = hipMemcpyAsync (A.d_pbytes.p, A.h_pbytes.p, pb, hipMemcpyHostToDevice, st) == hipSuccess &&
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
        return false;
      }
      take_parse_results (refs);
    }
    if (cfg.parse_dev) { t_dev_parse += now_s() - t_p0; n_dev_slices += (double)nt; }
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
    return true;
  }
  // one deferred slice as a task of the parse kernels: its payload and scaling lists into the page-locked bytes, its places on the device
  void slice_task (const TRef& r, lh264host::SliceTask& t) {
    uint8_t* hb = A.h_pbytes.as<uint8_t>(); uint8_t* db = A.d_pbytes.as<uint8_t>();
    const FrameOut& f = *r.f;
    const lh264host::DeferredSlice& ds = f.deferred[r.def];
    const DStream::DevAt at = r.s->dev_at.at (r.f);
    const int n_mb = f.mb_w * f.mb_h;
    const size_t sc_at = r.bytes_at + ((ds.rbsp.size() + 15) & ~ (size_t)15);
    if (!ds.rbsp.empty()) memcpy (hb + r.bytes_at, ds.rbsp.data(), ds.rbsp.size());
    memcpy (hb + sc_at, ds.pps.sl4, 96); memcpy (hb + sc_at + 96, ds.pps.sl8, 128);
    memset (&t, 0, sizeof (t));
    t.rbsp = db + r.bytes_at; t.rbsp_bytes = (uint32_t)ds.rbsp.size(); t.data_bit = (uint32_t)ds.data_bit;
    t.first_mb = ds.sh.first_mb;
    t.limit_mb = (size_t)ds.sid + 1 < f.slices.size() ? std::min (n_mb, f.slices[(size_t)ds.sid + 1].first_mb) : n_mb;
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
  }
  void take_parse_results (const std::vector<TRef>& refs) {
    const lh264host::SliceResult* res = A.h_pres.as<lh264host::SliceResult>();
    const size_t nt = refs.size();
    // a status anywhere in a stream's round: the whole round of that stream goes back to the host parser, and the stream stays there
    for (size_t j = 0; j < nt; j++) if (res[j].status != lh264slice::SLICE_OK && refs[j].s->dev_route) {
      DStream& s = *refs[j].s;
      s.dev_route = false; s.dev_at.clear();
      if (!cfg.sparse) s.parser->set_defer_slice_data (false);
      out[s.i]->parse_path = LH264_PARSE_PATH_FALLBACK;
    }
    for (size_t j = 0; j < nt; j++) {
      const TRef& r = refs[j];
      if (!r.s->dev_route) continue;
      FrameOut& f = *r.f;
      lh264host::DeferredSlice& ds = f.deferred[r.def];
      lh264_decoded_t& o = *out[r.s->i];
      if (!ds.counted) { ds.counted = true; o.parsed_slices++; }
      if (o.parse_path == LH264_PARSE_PATH_HOST) o.parse_path = LH264_PARSE_PATH_DEVICE;
      o.device_slices++;
      if (ds.cabac) o.device_cabac_slices++;
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

  // ---- the round: which streams fit, where their records and bytes go, what each picture delivers, which picture slots they take
  // (the buffers `rb` were last used by the round before the one that is on the device now: it has been delivered).  false: no round
  bool plan_round() {
    Round& rd = rounds[rb];
    rd.chains.clear(); rd.out_bytes = 0; rd.mot_bytes = 0; rd.mbi_bytes = 0; rd.timed = false;
    place.clear(); chain_first.clear();
    size_t n_mbs = 0;
    n_hmbs = n_sl = n_sp = n_jobs = n_out = n_mjobs = 0;
    max_units = max_w = max_h = max_bands = 1;
    bool alloc_ok = true, offsets_ok = true, tables_ok = true;
    for (auto& sp : active) {
      DStream& s = *sp;
      if (s.sel.empty()) continue;
      size_t m = 0, mh = 0, sl = 0, ents = 0, bytes = 0, shown = 0;
      std::vector<PicPlan> plan;
      for (auto& f : s.sel) {
        m += (size_t)f->mb_w * f->mb_h; if (!s.dev_at.count (f.get())) mh += (size_t)f->mb_w * f->mb_h; sl += f->slices.size(); ents += f->sparse_coeffs.size();
        plan.push_back (cfg.plan (f->crop_w, f->crop_h, s.i));
        if (!f->frozen) { bytes += plan.back().bytes; shown++; }
      }
      if (!rd.chains.empty() && n_mbs + m > cfg.group_mbs) { unselect (s); continue; }
      const FrameOut& f0 = *s.sel[0];
      if (f0.mb_w != s.geo.mb_w || f0.mb_h != s.geo.mb_h) {
        release_pool (s);                           // (the kernels that still read the old pictures are in front of whatever takes them next)
        s.geo.mb_w = f0.mb_w; s.geo.mb_h = f0.mb_h;
        s.geo.bytes = (lh264_pic_bytes (f0.mb_w, f0.mb_h, &s.geo.stride_y, &s.geo.stride_c, &s.geo.off[0], &s.geo.off[1], &s.geo.off[2]) + 255) & ~ (size_t)255;
      }
      RoundChain c;
      c.s = &s; c.first_picture = (int)s.delivered; c.at = rd.out_bytes; c.bytes = bytes; c.n_out = shown; c.dig0 = n_out;
      n_out += shown;
      if (cfg.fields) {
        size_t shown_mbs = 0;
        for (auto& f : s.sel) if (!f->frozen) { shown_mbs += (size_t)f->mb_w * f->mb_h; max_units = std::max (max_units, f->mb_h * lh264pack::motion_chunks (f->mb_w)); }
        c.mjob0 = n_mjobs; n_mjobs += shown;
        c.mot_at = rd.mot_bytes; c.mot_bytes = shown_mbs * 96; rd.mot_bytes += (c.mot_bytes + 15) & ~ (size_t)15;
        c.mbi_at = rd.mbi_bytes; c.mbi_bytes = shown_mbs * 8; rd.mbi_bytes += (c.mbi_bytes + 15) & ~ (size_t)15;
      }
      // the chains of the launch: a stream's pictures of the round one behind the other - or, with opts->pick, every picture on its own:
      // it references nothing, so the stream spreads over as many workgroups as it has pictures in the round; with a selection every run
      // that begins at an IDR picture.  (Delivery and the stream's digest follow rd.chains, the streams, in every case)
      for (size_t q = 0; q < s.sel.size(); q++) if (q == 0 || cfg.picking || (cfg.selecting && s.sel[q]->idr)) chain_first.push_back ((int32_t) (n_jobs + q));
      place.push_back ({n_hmbs, n_sl, n_sp, n_jobs});
      n_mbs += m; n_hmbs += mh; n_sl += sl; n_sp += ents; n_jobs += s.sel.size();
      for (size_t q = 0; q < plan.size(); q++) {
        max_bands = std::max (max_bands, bands_of (plan[q].oh));
        if (cfg.filter && !s.sel[q]->frozen && !filters.add_job (plan[q].src.w, plan[q].src.h, plan[q].dst.w, plan[q].dst.h)) tables_ok = false;
        // a float type: every picture, and so every row, begins at a multiple of 4 bytes - the chain at one of 16, a picture 3*ow*oh*es
        // bytes behind the one before (decode_pack_sample_kernel stores nothing narrower)
        if (cfg.stype && !s.sel[q]->frozen && ((plan[q].bytes | rd.out_bytes) & 3)) offsets_ok = false;
      }
      rd.out_bytes += (bytes + 15) & ~ (size_t)15;
      max_w = std::max (max_w, f0.mb_w); max_h = std::max (max_h, f0.mb_h);
      c.plan = std::move (plan);
      rd.chains.push_back (std::move (c));
    }
    if (rd.chains.empty()) return false;            // nothing to reconstruct (streams that ended without a picture)
    const int n_chains = (int)rd.chains.size();
    n_launch = (int)chain_first.size();
    alloc_ok = A.d_mbs.alloc (n_hmbs * sizeof (lh264_mb_t)) && (cfg.motion_only || (A.d_coef.alloc (n_hmbs * 768) && A.d_sparse.alloc (n_sp * 8))) && A.d_sl.alloc (n_sl * sizeof (lh264_slice_t)) &&
               A.d_jobs.alloc (n_jobs * sizeof (lh264_frame_job_t)) && A.d_first.alloc ((size_t) (n_launch + 1) * 4) && A.d_pack.alloc (n_jobs * sizeof (lh264_pack_job_t)) &&
               (cfg.motion_only || A.d_out[rb].alloc (rd.out_bytes)) && (cfg.device_out || cfg.no_pictures || A.h_out[rb].alloc (rd.out_bytes)) &&
               A.h_mbs[rb].alloc (n_hmbs * sizeof (lh264_mb_t)) && A.h_sparse[rb].alloc (n_sp * 8) && A.h_sl[rb].alloc (n_sl * sizeof (lh264_slice_t)) &&
               A.h_jobs[rb].alloc (n_jobs * sizeof (lh264_frame_job_t)) && A.h_first[rb].alloc ((size_t) (n_launch + 1) * 4) && A.h_pack[rb].alloc (n_jobs * sizeof (lh264_pack_job_t)) &&
               (!cfg.colour || (A.d_std.alloc (n_jobs) && A.h_std[rb].alloc (n_jobs))) &&
               (!cfg.placed || (A.d_place.alloc (n_jobs * sizeof (lh264_pack_place_t)) && A.h_place[rb].alloc (n_jobs * sizeof (lh264_pack_place_t)))) &&
               (!cfg.filter || (A.d_filter.alloc (filter_bytes()) && A.h_filter[rb].alloc (filter_bytes())));
    if (cfg.fields) alloc_ok = alloc_ok && A.d_mjobs.alloc (n_mjobs * sizeof (lh264_motion_job_t)) && A.h_mjobs[rb].alloc (n_mjobs * sizeof (lh264_motion_job_t)) &&
                               A.d_mot[rb].alloc (rd.mot_bytes) && A.d_mbi[rb].alloc (rd.mbi_bytes) && (cfg.device_out || (A.h_mot[rb].alloc (rd.mot_bytes) && A.h_mbi[rb].alloc (rd.mbi_bytes)));
    for (int k = 0; k < 2 && cfg.fields && alloc_ok; k++) if (!A.e_mot[rb][k]) alloc_ok = hipEventCreate (&A.e_mot[rb][k]) == hipSuccess;
    n_sjobs = (cfg.sha_pics ? n_out : 0) + (cfg.sha_stream ? (size_t)n_chains : 0);
    rd.dig_states_at = (n_out * 20 + 15) & ~ (size_t)15;
    dig_bytes = rd.dig_states_at + (size_t)n_chains * sizeof (lh264_sha1_state_t);
    if (cfg.sha) alloc_ok = alloc_ok && A.d_sjobs.alloc (n_sjobs * sizeof (lh264_sha1_job_t)) && A.h_sjobs[rb].alloc (n_sjobs * sizeof (lh264_sha1_job_t)) && A.d_dig.alloc (dig_bytes) &&
                            A.h_dig[rb].alloc (dig_bytes) && A.d_rec.alloc (n_out * sizeof (lh264_sha1_state_t)) && A.d_state.alloc ((size_t)n * sizeof (lh264_sha1_state_t));
    // picture slots (serial: the cache is shared).  A picture takes a slot that was free when the round began; a slot becomes free
    // behind the round when its picture is in no DPB any more - the round's pictures are all packed by then
    slot_of.assign ((size_t)n_chains, std::vector<int>());
    for (int c = 0; c < n_chains && alloc_ok && offsets_ok && !cfg.motion_only; c++) {
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
    if (alloc_ok && offsets_ok && tables_ok) return true;
    fail_device (!tables_ok ? "a filter table leaves the range the kernels take" : offsets_ok ? "device allocation failed" : "a float picture would not begin at a multiple of 4 bytes");
    for (auto& s : active) s->sel.clear();
    return false;
  }

  // a filter: the round's FilterJob records, behind them every table the call has built so far
  size_t filter_bytes() const { return n_jobs * sizeof (lh264pack::FilterJob) + filters.blob.size(); }

  // ---- staging (host threads): records to the page-locked buffers, the job tables; then what the round leaves with its streams
  void stage_round() {
    Round& rd = rounds[rb];
    const int n_chains = (int)rd.chains.size();
    run_parallel (n_chains, threads, [&] (int c) { stage_chain (c); });
    if (cfg.filter) memcpy (A.h_filter[rb].as<uint8_t>() + n_jobs * sizeof (lh264pack::FilterJob), filters.blob.data(), filters.blob.size());
    int32_t* h_first = A.h_first[rb].as<int32_t>();
    std::copy (chain_first.begin(), chain_first.end(), h_first);
    h_first[n_launch] = (int32_t)n_jobs;
    if (cfg.sha) {
      // the span jobs: a picture is a message of its own (its record is scratch), a chain's bytes are the next span of its stream's
      // message, whose record stays on the device from round to round; a copy of it comes down with the round
      lh264_sha1_job_t* sj = A.h_sjobs[rb].as<lh264_sha1_job_t>();
      uint8_t* const d_out = A.d_out[rb].as<uint8_t>();
      size_t q = 0;
      for (int c = 0; c < n_chains; c++) {
        RoundChain& rc = rd.chains[c];
        size_t at = rc.at;
        if (cfg.sha_pics) for (size_t k = 0; k < rc.pics.size(); k++) {
          sj[q++] = {d_out + at, rc.pics[k].bytes, A.d_rec.as<lh264_sha1_state_t>() + rc.dig0 + k, A.d_dig.as<uint8_t>() + (rc.dig0 + k) * 20, LH264_SHA1_FRESH | LH264_SHA1_FINAL, 0};
          at += rc.pics[k].bytes;
        }
        if (cfg.sha_stream) {
          sj[q++] = {d_out + rc.at, rc.bytes, A.d_state.as<lh264_sha1_state_t>() + rc.s->i, A.d_dig.as<uint8_t>() + rd.dig_states_at + (size_t)c * sizeof (lh264_sha1_state_t), rc.s->sha_started ? 0u : (uint32_t)LH264_SHA1_FRESH, 0};
          rc.s->sha_started = true;
        }
      }
      std::stable_sort (sj, sj + q, [] (const lh264_sha1_job_t& a, const lh264_sha1_job_t& b) { return a.len > b.len; });
    }
    for (int c = 0; c < n_chains; c++) {
      DStream& s = *rd.chains[c].s;
      // the slots the round leaves free: pictures the DPB behind the round's last picture does not hold
      const std::vector<int>& dpb = s.sel.back()->dpb_ids;
      for (Slot& sl : s.pool) if (sl.pic_id >= 0 && (cfg.picking || std::find (dpb.begin(), dpb.end(), sl.pic_id) == dpb.end())) sl.pic_id = -1;      // (opts->pick: a slot is needed for its round only)
      s.next_picture += (long)s.sel.size();
      if (!cfg.motion_only) out[s.i]->chain_pictures += (long)s.sel.size();
      s.delivered += (long)rd.chains[c].pics.size();
      s.out_off += rd.chains[c].bytes;
      s.mot_off += rd.chains[c].mot_bytes; s.mbi_off += rd.chains[c].mbi_bytes;
      // (fields: the pictures whose slots are free now are no reference any more)
      if (cfg.fields) for (auto it = s.held.begin(); it != s.held.end(); ) { if (cfg.picking || std::find (dpb.begin(), dpb.end(), it->first) == dpb.end()) it = s.held.erase (it); else ++it; }
      s.sel.clear();                                  // the pictures' records are staged: their memory goes back
    }
  }
  // one chain of the round: per picture its records, its reconstruct job, its pack job (by its plan) and what delivery will hand out
  void stage_chain (int c) {
    lh264_mb_t* h_mbs = A.h_mbs[rb].as<lh264_mb_t>(); uint64_t* h_sparse = A.h_sparse[rb].as<uint64_t>(); lh264_slice_t* h_sl = A.h_sl[rb].as<lh264_slice_t>();
    lh264_frame_job_t* h_jobs = A.h_jobs[rb].as<lh264_frame_job_t>(); lh264_pack_job_t* h_pack = A.h_pack[rb].as<lh264_pack_job_t>();
    uint8_t* h_std = cfg.colour ? A.h_std[rb].as<uint8_t>() : nullptr;
    lh264_pack_place_t* h_place = cfg.placed ? A.h_place[rb].as<lh264_pack_place_t>() : nullptr;
    lh264_motion_job_t* h_mjobs = cfg.fields ? A.h_mjobs[rb].as<lh264_motion_job_t>() : nullptr;
    lh264pack::FilterJob* h_filt = cfg.filter ? A.h_filter[rb].as<lh264pack::FilterJob>() : nullptr;
    const uint8_t* d_tables = A.d_filter.as<uint8_t>() + n_jobs * sizeof (lh264pack::FilterJob);      // (where the tables will lie on the device)
    const bool picking = cfg.picking, motion_only = cfg.motion_only;
    RoundChain& rc = rounds[rb].chains[c];
    DStream& s = *rc.s;
    size_t mo = place[c].mb0, so = place[c].sl0, po = place[c].sp0, j = place[c].job0, at = rc.at;
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
      if (cfg.fields) {
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
      if (h_place) memset (&h_place[j], 0, sizeof (lh264_pack_place_t));
      if (h_filt) memset (&h_filt[j], 0, sizeof (lh264pack::FilterJob));
      pj.reserved = cfg.scale;
      const uint8_t std_byte = cfg.standard (f);      // (a picture select let through: its standard is defined)
      if (h_std) h_std[j] = std_byte & 3;
      if (f.frozen) { if (!on_dev) mo += nm; so += f.slices.size(); j++; continue; }      // withheld: a reference like any other, but no window to pack (crop_h 0)
      pj.y = jb.dst.y_dev; pj.u = jb.dst.u_dev; pj.v = jb.dst.v_dev;
      pj.dst = A.d_out[rb].as<uint8_t>() + at;
      pj.stride_y = s.geo.stride_y; pj.stride_c = s.geo.stride_c;
      // the picture's view: the source rectangle takes the window's place in the job, the destination goes to the job's place
      const PicPlan& v = rc.plan[q];
      pj.crop_x = f.crop_x + v.src.x; pj.crop_y = f.crop_y + v.src.y; pj.crop_w = v.src.w; pj.crop_h = v.src.h; pj.format = cfg.format;
      if (h_filt) h_filt[j] = filters.job (d_tables, v.src.w, v.src.h, v.dst.w, v.dst.h);
      if (h_place) { h_place[j].x = v.dst.x; h_place[j].y = v.dst.y; h_place[j].w = v.dst.w; h_place[j].h = v.dst.h; h_place[j].fill = cfg.fill; }
      for (const lh264_rect_t* r : {&v.src, &v.dst}) { rc.view.push_back (r->x); rc.view.push_back (r->y); rc.view.push_back (r->w); rc.view.push_back (r->h); }
      lh264_decoded_pic_t dp;
      dp.width = v.ow; dp.height = v.oh; dp.frame_num = f.frame_num; dp.idr = f.idr ? 1 : 0; dp.offset = off; dp.bytes = v.bytes;
      rc.pics.push_back (dp);
      rc.concealed.push_back (f.concealed);
      rc.source_wh.push_back (f.crop_w); rc.source_wh.push_back (f.crop_h);
      rc.index.push_back ((int32_t)f.index);
      if (cfg.colour) rc.colour.push_back (std_byte);
      if (cfg.fields) {
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
      at += v.bytes; off += v.bytes;
      if (!on_dev) mo += nm;
      so += f.slices.size(); j++;
    }
  }

  // ---- the device stage, asynchronous: upload, clear + expand the coefficients, reconstruct, pack; the download behind an event
  void enqueue_round() {
    Round& rd = rounds[rb];
    const bool motion_only = cfg.motion_only;
    hipStream_t st = A.s_run;
    uint8_t* const d_out = A.d_out[rb].as<uint8_t>();
    auto up = [&] (DevBuf& d, const PinBuf& s, size_t bytes) { return bytes == 0 || hipMemcpyAsync (d.p, s.p, bytes, hipMemcpyHostToDevice, st) == hipSuccess; };
    // (motion only: the records and the slice tables are all the gather reads)
    bool ok = up (A.d_mbs, A.h_mbs[rb], n_hmbs * sizeof (lh264_mb_t)) && (motion_only || up (A.d_sparse, A.h_sparse[rb], n_sp * 8)) && up (A.d_sl, A.h_sl[rb], n_sl * sizeof (lh264_slice_t)) &&
              (motion_only || (up (A.d_jobs, A.h_jobs[rb], n_jobs * sizeof (lh264_frame_job_t)) && up (A.d_first, A.h_first[rb], (size_t) (n_launch + 1) * 4) && up (A.d_pack, A.h_pack[rb], n_jobs * sizeof (lh264_pack_job_t)) &&
                               (!cfg.colour || up (A.d_std, A.h_std[rb], n_jobs)) && (!cfg.placed || up (A.d_place, A.h_place[rb], n_jobs * sizeof (lh264_pack_place_t))) && (!cfg.filter || up (A.d_filter, A.h_filter[rb], filter_bytes())) &&
                               (n_hmbs == 0 || hipMemsetAsync (A.d_coef.p, 0, n_hmbs * 768, st) == hipSuccess)));
    // the fields need the records only: the gather goes in front of the reconstruct launch
    if (ok && n_mjobs) {
      ok = up (A.d_mjobs, A.h_mjobs[rb], n_mjobs * sizeof (lh264_motion_job_t)) && hipEventRecord (A.e_mot[rb][0], st) == hipSuccess &&
           launch_motion (A.d_mjobs.as<lh264_motion_job_t>(), (int)n_mjobs, max_units, st) && hipEventRecord (A.e_mot[rb][1], st) == hipSuccess;
      rd.timed = ok;
    }
    if (ok && n_sp && !motion_only) { lh264host::expand_sparse (A.d_sparse.as<uint64_t>(), n_sp, A.d_coef.as<int16_t>(), st); ok = hipGetLastError() == hipSuccess; }
    if (ok && !motion_only) ok = lh264_recon_chains (A.d_jobs.as<lh264_frame_job_t>(), A.d_first.as<int32_t>(), n_launch, max_w, max_h, st) == LH264_OK;
    if (ok && !motion_only) { n_rounds++; n_launched += n_launch; n_launched_jobs += (long long)n_jobs; }
    if (ok && !motion_only) ok = launch_pack ({A.d_pack.as<lh264_pack_job_t>(), cfg.placed ? A.d_place.as<lh264_pack_place_t>() : nullptr, A.d_std.as<uint8_t>(), (int)n_jobs, max_bands,
                                               cfg.out_w, cfg.out_h, cfg.colour, cfg.scale, cfg.stype ? &cfg.sample : nullptr, cfg.filter ? A.d_filter.as<lh264pack::FilterJob>() : nullptr}, st);
    if (ok && cfg.sha) {
      ok = up (A.d_sjobs, A.h_sjobs[rb], n_sjobs * sizeof (lh264_sha1_job_t));
      if (ok && n_sjobs) { hipLaunchKernelGGL (sha1_spans_kernel, dim3 ((unsigned) ((n_sjobs + 63) / 64)), dim3 (64), 0, st, A.d_sjobs.as<lh264_sha1_job_t>(), (int)n_sjobs); ok = hipGetLastError() == hipSuccess; }
      ok = ok && hipMemcpyAsync (A.h_dig[rb].p, A.d_dig.p, dig_bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
    }
    // bytes that stay on the device: every stream's run goes behind what its handle holds
    if (ok && cfg.device_out && cfg.fields) for (RoundChain& c : rd.chains) {
      lh264_decoded_t& r = *out[c.s->i];
      if (!c.mot_bytes) continue;
      if (!r.mot_dev.append (A.d_mot[rb].as<uint8_t>() + c.mot_at, c.mot_bytes, st) || !r.mbi_dev.append (A.d_mbi[rb].as<uint8_t>() + c.mbi_at, c.mbi_bytes, st)) { ok = false; break; }
    }
    if (ok && cfg.device_out && !cfg.no_pictures) for (RoundChain& c : rd.chains) {
      if (!c.bytes) continue;                   // (every picture of the chain withheld)
      if (!out[c.s->i]->dev.append (d_out + c.at, c.bytes, st)) { ok = false; break; }
    }
    ok = ok && hipEventRecord (A.e_run[rb], st) == hipSuccess;
    if (ok && cfg.down) ok = hipStreamWaitEvent (A.s_down, A.e_run[rb], 0) == hipSuccess &&
                             (cfg.no_pictures || !rd.out_bytes || hipMemcpyAsync (A.h_out[rb].p, d_out, rd.out_bytes, hipMemcpyDeviceToHost, A.s_down) == hipSuccess) &&
                             (!cfg.fields || !rd.mot_bytes || (hipMemcpyAsync (A.h_mot[rb].p, A.d_mot[rb].p, rd.mot_bytes, hipMemcpyDeviceToHost, A.s_down) == hipSuccess &&
                                                               hipMemcpyAsync (A.h_mbi[rb].p, A.d_mbi[rb].p, rd.mbi_bytes, hipMemcpyDeviceToHost, A.s_down) == hipSuccess)) &&
                             hipEventRecord (A.e_down[rb], A.s_down) == hipSuccess;
    if (!ok) { const char* le = lh264_last_error(); fail_device (std::string ("launching the device stage failed") + (le && *le ? std::string (": ") + le : std::string())); for (RoundChain& c : rd.chains) c.s->stopped = true; }
    else rd.live = true;
  }

  // what a delivered chain adds to its stream's handle: the picture records, and the round's digests and fields.  The digests came down
  // on the run stream, in front of the event: the pictures' 20 bytes, and the stream's record as this round leaves it (a stream's
  // digest covers the rounds that were delivered, whatever is on the device behind them)
  void take_chain (const Round& rd, int b, size_t k) {
    const RoundChain& c = rd.chains[k];
    lh264_decoded_t& r = *out[c.s->i];
    auto add = [] (auto& to, const auto& from) { to.insert (to.end(), from.begin(), from.end()); };
    add (r.pics, c.pics); add (r.concealed, c.concealed); add (r.source_wh, c.source_wh); add (r.view, c.view); add (r.index, c.index); add (r.colour, c.colour);
    const uint8_t* hd = A.h_dig[b].as<uint8_t>();
    if (cfg.sha_pics) r.pic_sha.insert (r.pic_sha.end(), hd + c.dig0 * 20, hd + (c.dig0 + c.pics.size()) * 20);
    if (cfg.sha_stream) memcpy (&r.stream_state, hd + rd.dig_states_at + k * sizeof (lh264_sha1_state_t), sizeof (lh264_sha1_state_t));
    // the round's fields: geometry per picture, and in host mode the chain's blocks behind what the handle holds
    if (cfg.fields) add (r.motion_geo, c.motion_geo);
    if (!cfg.fields || cfg.device_out) return;
    const uint8_t* hm = A.h_mot[b].as<uint8_t>() + c.mot_at; const uint8_t* hi = A.h_mbi[b].as<uint8_t>() + c.mbi_at;
    r.mot.insert (r.mot.end(), hm, hm + c.mot_bytes);
    r.mbi.insert (r.mbi.end(), hi, hi + c.mbi_bytes);
  }
  // a round that is on the device: wait for its bytes and hand them on
  void deliver (int b) {
    Round& rd = rounds[b];
    if (!rd.live) return;
    rd.live = false;
    const double t0 = now_s();
    if (!device_failed && hipEventSynchronize (cfg.down ? A.e_down[b] : A.e_run[b]) != hipSuccess) fail_device ("the device stage failed");
    const double t1 = now_s();
    t_wait += t1 - t0;
    if (device_failed) {
      for (RoundChain& c : rd.chains) { c.s->stopped = true; lh264_decoded_t& r = *out[c.s->i]; if (r.status == LH264_OK) { r.status = LH264_E_HIP; r.error = device_error; } }
      return;
    }
    const uint8_t* hb = A.h_out[b].as<uint8_t>();
    if (rd.timed) { float ms = 0; if (hipEventElapsedTime (&ms, A.e_mot[b][0], A.e_mot[b][1]) == hipSuccess) motion_ms += ms; motion_bytes += rd.mot_bytes + rd.mbi_bytes; }
    if (cfg.sink) {
      for (size_t k = 0; k < rd.chains.size(); k++) {
        RoundChain& c = rd.chains[k];
        // (the sink path skips a chain without a delivered picture: there is no run to hand over, and nothing of it reaches the handle)
        if (c.s->stopped || c.pics.empty()) continue;
        lh264_decoded_t& r = *out[c.s->i];
        if (cfg.sink (cfg.user, c.s->i, c.first_picture, (int)c.pics.size(), c.pics.data(), hb + c.at, c.bytes) != 0) {
          c.s->stopped = true; r.status = LH264_E_ARG; r.error = "sink";
          continue;
        }
        take_chain (rd, b, k);                      // (the sink path keeps no bytes: the sink has them)
      }
    } else {
      run_parallel ((int)rd.chains.size(), threads, [&] (int k) {
        RoundChain& c = rd.chains[k];
        if (c.s->stopped) return;
        lh264_decoded_t& r = *out[c.s->i];
        if (!cfg.device_out && !cfg.no_pictures) r.bytes.insert (r.bytes.end(), hb + c.at, hb + c.at + c.bytes);
        take_chain (rd, b, (size_t)k);
      });
    }
    t_deliver += now_s() - t1;
  }

  void run() {
    const bool deferring = cfg.parse_dev || cfg.sparse;
    while (admit()) {
      const double t_a = now_s();
      run_parallel ((int)active.size(), threads, [&] (int k) { fill_and_select (*active[k], true, deferring); });
      if (deferring && !device_parse()) { deliver (rb ^ 1); continue; }
      const double t_b = now_s();
      t_parse += t_b - t_a;
      if (!plan_round()) { deliver (rb ^ 1); continue; }      // (the round on the device is still owed)
      stage_round();
      const double t_c = now_s();
      t_stage += t_c - t_b;
      enqueue_round();
      t_enqueue += now_s() - t_c;
      deliver (rb ^ 1);                               // the round before: its bytes arrive while this one reconstructs
      rb ^= 1;
    }
    finish();
  }
  // the rounds still on the device, the streams still active, the streams' digests; what a failure of the device stage leaves
  void finish() {
    deliver (0);
    deliver (1);
    hipStreamSynchronize (A.s_run);
    hipStreamSynchronize (A.s_down);
    for (auto& s : active) retire (*s);
    active.clear(); retired.clear();
    if (cfg.sha_stream) for (int i = 0; i < n; i++) { lh264_sha1_state_t fin = out[i]->stream_state; lh264sha1::finish (&fin, out[i]->stream_sha); }
    // (streams that were complete before a failure of the device stage keep their result; the others carry the error)
    if (device_failed) for (int i = next_stream; i < n; i++) { out[i]->status = LH264_E_HIP; out[i]->error = device_error; }
  }
  // lh264_decode_last_timing, _last_parse_timing, _last_motion, _last_chains; LH264_TRACE_DECODE
  void publish() const {
    g_timing[0] = (now_s() - t_call) * 1e3; g_timing[1] = t_parse * 1e3; g_timing[2] = t_stage * 1e3; g_timing[3] = t_enqueue * 1e3; g_timing[4] = t_wait * 1e3; g_timing[5] = t_deliver * 1e3;
    g_parse_timing[0] = t_dev_parse * 1e3; g_parse_timing[1] = n_dev_slices;
    g_motion_ms = motion_ms; g_motion_bytes = motion_bytes;
    g_chains[0] = n_rounds; g_chains[1] = n_launched; g_chains[2] = n_launched_jobs;
    if (trace_on()) fprintf (stderr, "[lh264 decode] %d streams: %.3f s (parse %.3f, staging %.3f, enqueue %.3f, waiting for the device %.3f, delivery %.3f); arena %.1f MB device, %.1f MB pinned\n",
                             n, g_timing[0] / 1e3, t_parse, t_stage, t_enqueue, t_wait, t_deliver, A.device_bytes() / 1e6, A.pinned_bytes() / 1e6);
  }
};

}  // namespace

extern "C" {

int lh264_debug_pack_cpu (const lh264_pack_job_t* jobs, int n) {
  if (!jobs || n < 0) return LH264_E_ARG;
  for (int k = 0; k < n; k++) {
    const lh264_pack_job_t& j = jobs[k];
    if (!pack_job_ok (j, {kAnySide, 3})) return LH264_E_ARG;
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
    if (!pack_job_ok (j, {kAnySide, 3}) || j.reserved != jobs[0].reserved) return LH264_E_ARG;      // (one kernel per launch: one scale)
    int ow, oh;
    lh264pack::scaled_size (j.crop_w, j.crop_h, j.reserved, &ow, &oh);
    max_bands = std::max (max_bands, bands_of (oh));
  }
  return debug_launch ({jobs, nullptr, nullptr, n, max_bands, 0, 0, 0, n ? jobs[0].reserved : 0, nullptr});
}

// a table of jobs the resize entry points take: windows the front end can deliver (even, up to 16,384 a side), reserved 0
static bool resize_jobs_ok (const lh264_pack_job_t* jobs, int n, int out_w, int out_h) {
  if (!jobs || n <= 0 || !lh264pack::size_ok (out_w, out_h)) return false;
  for (int k = 0; k < n; k++) if (!pack_job_ok (jobs[k], {kFrontEndSide, 0})) return false;
  return true;
}

int lh264_debug_resize_cpu (const lh264_pack_job_t* jobs, int n, int out_w, int out_h) {
  if (!resize_jobs_ok (jobs, n, out_w, out_h)) return LH264_E_ARG;
  for (int k = 0; k < n; k++) for (int band = 0; band * lh264pack::kBandRows < out_h; band++) lh264pack::pack_band_resized (jobs[k], out_w, out_h, band, 0, 1);
  return LH264_OK;
}

int lh264_debug_resize_dev (const lh264_pack_job_t* jobs, int n, int out_w, int out_h) {
  if (!resize_jobs_ok (jobs, n, out_w, out_h)) return LH264_E_ARG;
  return debug_launch ({jobs, nullptr, nullptr, n, bands_of (out_h), out_w, out_h, 0, 0, nullptr});
}

// a table the RGB entry points take: windows the front end can deliver, I420, a layout and standard bytes that are defined, and a sizing:
// the given size with reserved 0, or 0, 0 with reserved 0..3.  *max_bands: the bands of the tallest delivered picture
static bool rgb_jobs_ok (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job, int* max_bands) {
  if (!jobs || !std_per_job || n <= 0 || (layout != (int)LH264_COLOUR_RGB24 && layout != (int)LH264_COLOUR_RGBP)) return false;
  if ((out_w || out_h) && !lh264pack::size_ok (out_w, out_h)) return false;
  *max_bands = 1;
  for (int k = 0; k < n; k++) {
    const lh264_pack_job_t& j = jobs[k];
    if (!pack_job_ok (j, {kFrontEndSide, out_w ? 0 : 3}) || j.format != LH264_FMT_I420 || std_per_job[k] > 3) return false;
    int ow, oh;
    lh264pack::delivered_size (j.crop_w, j.crop_h, j.reserved, out_w, out_h, &ow, &oh);
    *max_bands = std::max (*max_bands, bands_of (oh));
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
  return debug_launch ({jobs, nullptr, std_per_job, n, max_bands, out_w, out_h, layout, 0, nullptr});
}

// what the float entry points take: a sample struct with a float type, the RGB table, every destination a multiple of 4
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
  return debug_launch ({jobs, nullptr, std_per_job, n, max_bands, out_w, out_h, layout, 0, sample});
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
  *max_bands = bands_of (out_h);
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
  const bool typed = sample && sample->type != LH264_SAMPLE_U8;
  return debug_launch ({jobs, places, colour ? std_per_job : nullptr, n, max_bands, out_w, out_h, colour, 0, typed ? sample : nullptr});
}

int lh264_filter_taps (uint32_t filter, int src_len, int dst_len, int X, int32_t* first, int16_t* k, int cap, int* n) {
  if ((filter != LH264_FILTER_BILINEAR && filter != LH264_FILTER_BICUBIC) || src_len < 1 || src_len > kFrontEndSide || dst_len < 1 || dst_len > 4096 || X < 0 || X >= dst_len ||
      !first || !n || cap < 0 || (cap && !k)) return LH264_E_ARG;
  std::vector<int32_t> ent; std::vector<int16_t> w;
  if (!filter_axis (filter, src_len, dst_len, &ent, &w)) return LH264_E_UNSUPPORTED;
  *first = ent[3 * (size_t)X]; *n = ent[3 * (size_t)X + 1];
  for (int i = 0; i < *n && i < cap; i++) k[i] = w[(size_t)ent[3 * (size_t)X + 2] + i];
  return LH264_OK;
}

// a table the filtered entry points take: what lh264_debug_view_* take, but places may be NULL, and a filter that has tables
static bool filter_jobs_ok (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, uint32_t filter, int colour, const uint8_t* std_per_job, const lh264_decode_sample_t* sample, int* max_bands) {
  if ((filter != LH264_FILTER_BILINEAR && filter != LH264_FILTER_BICUBIC) || !lh264pack::size_ok (out_w, out_h)) return false;
  const bool typed = sample && sample->type != LH264_SAMPLE_U8;
  if (sample && !sample_ok (sample)) return false;
  if (typed ? !sample_jobs_ok (jobs, n, out_w, out_h, colour, std_per_job, sample, max_bands) :
      colour ? !rgb_jobs_ok (jobs, n, out_w, out_h, colour, std_per_job, max_bands) : !resize_jobs_ok (jobs, n, out_w, out_h)) return false;
  *max_bands = bands_of (out_h);
  for (int k = 0; k < n && places; k++) if (!lh264pack::place_ok (places[k], out_w, out_h)) return false;
  return true;
}
// fp gets the tables of every job's geometry, rec the jobs' records: for the blob where it lies in host memory, or (at_zero) for a blob
// at address 0, which debug_launch moves to where it went on the device
static bool filter_tables (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, FilterPlan* fp, std::vector<lh264pack::FilterJob>* rec, bool at_zero) {
  for (int k = 0; k < n; k++) if (!fp->add_job (jobs[k].crop_w, jobs[k].crop_h, places ? places[k].w : out_w, places ? places[k].h : out_h)) return false;
  const uint8_t* base = at_zero ? nullptr : fp->blob.data();
  for (int k = 0; k < n; k++) rec->push_back (fp->job (base, jobs[k].crop_w, jobs[k].crop_h, places ? places[k].w : out_w, places ? places[k].h : out_h));
  return true;
}

int lh264_debug_filter_cpu (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, uint32_t filter, int colour, const uint8_t* std_per_job, const lh264_decode_sample_t* sample) {
  int max_bands = 0;
  if (!filter_jobs_ok (jobs, places, n, out_w, out_h, filter, colour, std_per_job, sample, &max_bands)) return LH264_E_ARG;
  FilterPlan fp {filter, {}, {}};
  std::vector<lh264pack::FilterJob> rec;
  if (!filter_tables (jobs, places, n, out_w, out_h, &fp, &rec, false)) return LH264_E_UNSUPPORTED;
  const bool typed = sample && sample->type != LH264_SAMPLE_U8;
  for (int k = 0; k < n; k++) for (int band = 0; band < max_bands; band++) {
    const lh264_pack_place_t pl = places ? places[k] : lh264_pack_place_t {0, 0, out_w, out_h, 0u, 0u};
    if (typed) lh264pack::pack_band_sample_filtered (jobs[k], rec[k], pl, out_w, out_h, colour, std_per_job[k], *sample, band, 0, 1);
    else if (colour) lh264pack::pack_band_rgb_filtered (jobs[k], rec[k], pl, out_w, out_h, colour, std_per_job[k], band, 0, 1);
    else lh264pack::pack_band_filtered (jobs[k], rec[k], pl, out_w, out_h, band, 0, 1);
  }
  return LH264_OK;
}

int lh264_debug_filter_dev (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, uint32_t filter, int colour, const uint8_t* std_per_job, const lh264_decode_sample_t* sample) {
  int max_bands = 0;
  if (!filter_jobs_ok (jobs, places, n, out_w, out_h, filter, colour, std_per_job, sample, &max_bands)) return LH264_E_ARG;
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  FilterPlan fp {filter, {}, {}};
  std::vector<lh264pack::FilterJob> rec;
  if (!filter_tables (jobs, places, n, out_w, out_h, &fp, &rec, true)) return LH264_E_UNSUPPORTED;
  const bool typed = sample && sample->type != LH264_SAMPLE_U8;
  return debug_launch ({jobs, places, colour ? std_per_job : nullptr, n, max_bands, out_w, out_h, colour, 0, typed ? sample : nullptr, rec.data()}, &fp);
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
  DevBuf d_jobs;
  const bool ok = upload (d_jobs, jobs, (size_t)n * sizeof (lh264_motion_job_t)) && launch_motion (d_jobs.as<lh264_motion_job_t>(), n, units, nullptr) && hipStreamSynchronize (nullptr) == hipSuccess;
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
  return lh264_decode_batch_ex5 (data, len, n, threads, opts, ext, sample, view, motion, nullptr, out);
}

int lh264_decode_batch_ex5 (const uint8_t* const* data, const size_t* len, int n, int threads, const lh264_decode_opts_t* opts, const lh264_decode_ext_t* ext, const lh264_decode_sample_t* sample, const lh264_decode_view_t* view, const lh264_decode_motion_t* motion, const lh264_decode_select_t* select, lh264_decoded_t** out) {
  return lh264_decode_batch_ex6 (data, len, n, threads, opts, ext, sample, view, motion, select, nullptr, out);
}

int lh264_decode_batch_ex6 (const uint8_t* const* data, const size_t* len, int n, int threads, const lh264_decode_opts_t* opts, const lh264_decode_ext_t* ext, const lh264_decode_sample_t* sample, const lh264_decode_view_t* view, const lh264_decode_motion_t* motion, const lh264_decode_select_t* select, const lh264_decode_filter_t* filter, lh264_decoded_t** out) {
  if (!data || !len || !out || n < 0) return LH264_E_ARG;
  DecodeConfig cfg;
  if (decode_config (opts, ext, sample, view, motion, select, filter, n, &cfg) != LH264_OK) return LH264_E_ARG;      // (every refusal of an argument comes before the device is asked for)
  if (lh264_device_count() <= 0) return LH264_E_NODEVICE;
  if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
  if (threads < 1) threads = 1;
  int device = 0;
  if (hipGetDevice (&device) != hipSuccess || device < 0 || device >= lh264host::kMaxDevices) return LH264_E_ARG;
  for (int i = 0; i < n; i++) { out[i] = new lh264_decoded(); out[i]->device = device; out[i]->sample_type = cfg.stype; out[i]->filter = (int)cfg.filter; out[i]->fields = cfg.fields; out[i]->sha = cfg.sha_bits; }
  auto arena_lock = g_arena.lock (device);
  Arena& A = arena_lock.get();
  if (!A.init()) { for (int i = 0; i < n; i++) { out[i]->status = LH264_E_HIP; out[i]->error = "creating the HIP streams failed"; } return LH264_OK; }
  DecodeCall call {cfg, A, data, len, n, threads, out};
  call.run();
  call.publish();
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
// the header walk of lh264_decode_batch_ex5 with a selection, and its rule: every slice deferred, none resolved
int lh264_parser_plan (const uint8_t* data, size_t len, const lh264_select_t* sel, int32_t* needed, int cap_needed, int* n_needed, int32_t* delivered, int cap_delivered, int* n_delivered) {
  if (!sel || !select_entry_ok (*sel) || !n_needed || !n_delivered || cap_needed < 0 || cap_delivered < 0 || (cap_needed && !needed) || (cap_delivered && !delivered) || (!data && len)) return LH264_E_ARG;
  const Selection q (*sel);
  Parser P;
  P.set_sparse_coeffs (true); P.set_sparse_levels (true);
  P.set_defer_slice_data (true); P.set_defer_cabac (true);
  P.begin_file (data, data ? len : 0);
  int nn = 0, nd = 0;
  long run_from = 0;                                   // the first picture of the current run that is not needed yet
  bool over = q.last() < 0;
  while (!over && !P.file_finished()) {
    P.feed_file_some (0);
    const long limit = P.error().empty() ? 0x7fffffffffffffffl : P.error_pictures();
    for (auto& f : P.frames()) {
      const long k = f->index;
      if (over || k >= limit) { over = true; break; }
      if (f->idr) run_from = k;
      if (q.requested (k)) {
        for (long j = run_from; j <= k; j++) { if (nn < cap_needed) needed[nn] = (int32_t)j; nn++; }
        if (nd < cap_delivered) delivered[nd] = (int32_t)k;
        nd++; run_from = k + 1;
      }
      over = k >= q.last();
    }
    P.frames().clear();
    over = over || !P.error().empty();
  }
  *n_needed = nn; *n_delivered = nd;
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
int lh264_decoded_filter (const lh264_decoded_t* d) { return d ? d->filter : LH264_E_ARG; }
long long lh264_decoded_parsed_slices (const lh264_decoded_t* d) { return d ? (long long)d->parsed_slices : 0; }
long long lh264_decoded_chain_pictures (const lh264_decoded_t* d) { return d ? (long long)d->chain_pictures : 0; }
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
  if (len) *len = d ? d->dev.len : 0;
  return d ? d->dev.p : nullptr;
}
int lh264_decoded_copy_dev (const lh264_decoded_t* d, void* dst_dev, size_t cap) {
  if (!d || !dst_dev || cap < d->dev.len) return LH264_E_ARG;
  if (d->dev.len && hipMemcpy (dst_dev, d->dev.p, d->dev.len, hipMemcpyDeviceToDevice) != hipSuccess) return LH264_E_HIP;
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
  if (motion) *motion = (const int16_t*)d->mot_dev.p;
  if (motion_bytes) *motion_bytes = d->mot_dev.len;
  if (info) *info = d->mbi_dev.p;
  if (info_bytes) *info_bytes = d->mbi_dev.len;
  return LH264_OK;
}
int lh264_decoded_motion_copy_dev (const lh264_decoded_t* d, void* motion_dst_dev, size_t motion_cap, void* info_dst_dev, size_t info_cap) {
  if (!d || !d->fields || (motion_dst_dev && motion_cap < d->mot_dev.len) || (info_dst_dev && info_cap < d->mbi_dev.len)) return LH264_E_ARG;
  if (motion_dst_dev && d->mot_dev.len && hipMemcpy (motion_dst_dev, d->mot_dev.p, d->mot_dev.len, hipMemcpyDeviceToDevice) != hipSuccess) return LH264_E_HIP;
  if (info_dst_dev && d->mbi_dev.len && hipMemcpy (info_dst_dev, d->mbi_dev.p, d->mbi_dev.len, hipMemcpyDeviceToDevice) != hipSuccess) return LH264_E_HIP;
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
