// slice_parse_check.cpp - the macroblock layers of csrc/lh264_slice.h (CAVLC) and csrc/lh264_slice_cabac.h (CABAC) under the host
// sanitizers: a stand-alone program that runs every slice of the Annex-B files it is given through lh264slice::parse_slice or
// lh264slice::parse_slice_cabac, each buffer (the CABAC context bytes and line included) an allocation of its own of exactly
// the size the task names (a byte read or written outside any of them is the sanitizer's to report), and compares what comes out with
// the host parser's parse_deferred: a status exactly where the host fails, the host's records and coefficients where it does not.  A
// picture with more than one slice has its first slice run once more with the limit drawn in by three macroblocks: OVERRUN, and
// nothing at or beyond the limit written.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iinclude tools/slice_parse_check.cpp \
//       losslessh264_amd/csrc/host/h264_parser.cpp losslessh264_amd/csrc/host/pip_symbols.cpp -o slice_parse_check
//   ./slice_parse_check tests/golden/streams/*.264 tests/golden/edge/*.264 ...
// tools/slice_parse_dump_cases.py writes the damaged streams of the tests into a directory and prints the whole list of inputs.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../losslessh264_amd/csrc/host/h264_parser.h"
#include "../losslessh264_amd/csrc/lh264_slice_cabac.h"

using namespace lh264host;

namespace {

struct Bufs {
  uint8_t* rbsp; uint8_t* scaling; int8_t* line; lh264_mb_t* mbs; int16_t* coeffs; lh264_slice_t* slices; uint8_t* state;
  Bufs (const FrameOut& f, const DeferredSlice& d) {
    const size_t n = (size_t)f.mb_w * f.mb_h;
    rbsp = (uint8_t*)malloc (d.rbsp.size() ? d.rbsp.size() : 1); if (d.rbsp.size()) memcpy (rbsp, d.rbsp.data(), d.rbsp.size());
    scaling = (uint8_t*)malloc (224); memcpy (scaling, d.pps.sl4, 96); memcpy (scaling + 96, d.pps.sl8, 128);
    line = (int8_t*)malloc ((size_t)f.mb_w * (d.cabac ? (size_t)lh264slice::kCabacLineBytes : 4));
    state = (uint8_t*)malloc (lh264slice::kCabacContexts);
    mbs = (lh264_mb_t*)aligned_alloc (16, n * sizeof (lh264_mb_t)); memset (mbs, 0, n * sizeof (lh264_mb_t));
    coeffs = (int16_t*)calloc (n * 384, 2);
    slices = (lh264_slice_t*)malloc (f.slices.size() * sizeof (lh264_slice_t)); memcpy (slices, f.slices.data(), f.slices.size() * sizeof (lh264_slice_t));
  }
  ~Bufs() { free (rbsp); free (scaling); free (line); free (mbs); free (coeffs); free (slices); free (state); }
};

SliceTask make_task (const FrameOut& f, const DeferredSlice& d, const Bufs& b) {
  const int n = f.mb_w * f.mb_h;
  SliceTask t; memset (&t, 0, sizeof (t));
  t.rbsp = b.rbsp; t.rbsp_bytes = (uint32_t)d.rbsp.size(); t.data_bit = (uint32_t)d.data_bit;
  t.first_mb = d.sh.first_mb;
  t.limit_mb = (size_t)d.sid + 1 < f.slices.size() && f.slices[(size_t)d.sid + 1].first_mb < n ? f.slices[(size_t)d.sid + 1].first_mb : n;
  t.mb_w = f.mb_w; t.mb_h = f.mb_h; t.slice_index = d.sid; t.slice_qp = d.sh.slice_qp;
  t.slice_type = (uint8_t)d.sh.slice_type; t.num_ref_idx_l0 = (uint8_t)d.sh.num_ref_idx_l0;
  t.transform_8x8 = d.pps.transform_8x8; t.constrained_intra_pred = d.pps.constrained_intra_pred; t.use_sl = d.sps_scaling || d.pps.scaling_matrix_present;
  t.chroma_qp_offset[0] = (int8_t)d.pps.chroma_qp_offset[0]; t.chroma_qp_offset[1] = (int8_t)d.pps.chroma_qp_offset[1];
  if (d.cabac) t.reserved = (uint8_t) (lh264slice::kTaskCabac | (d.sh.cabac_init_idc & 3));
  t.scaling = b.scaling; t.mbs = b.mbs; t.coeffs = b.coeffs; t.slice = b.slices + d.sid; t.line = b.line;
  return t;
}

lh264slice::Tables* T;
lh264slice::CabacTables* TC;
SliceResult walk (const SliceTask& t, const Bufs& b, lh264_mb_t* rec) {
  if (!lh264slice::task_is_cabac (t)) return lh264slice::parse_slice (*T, t, rec, t.line);
  lh264slice::cabac_init_states (t, b.state);
  return lh264slice::parse_slice_cabac (*TC, t, rec, (uint8_t*)t.line, b.state);
}

}  // namespace

int main (int argc, char** argv) {
  T = new lh264slice::Tables();
  lh264slice::fill_tables (*T);
  TC = new lh264slice::CabacTables();
  lh264slice::fill_cabac_tables (*TC);
  long files = 0, slices = 0, cabac = 0, failed = 0, overruns = 0, bad = 0;
  for (int a = 1; a < argc; a++) {
    FILE* fp = fopen (argv[a], "rb");
    if (!fp) { fprintf (stderr, "%s: cannot open\n", argv[a]); return 2; }
    std::vector<uint8_t> data;
    uint8_t tmp[65536]; size_t got;
    while ((got = fread (tmp, 1, sizeof (tmp), fp)) > 0) data.insert (data.end(), tmp, tmp + got);
    fclose (fp);
    files++;
    Parser P;
    P.set_defer_slice_data (true);
    P.set_defer_cabac (true);
    P.feed_file (data.data(), data.size());
    for (auto& fr : P.frames()) {
      FrameOut& f = *fr;
      const size_t n = (size_t)f.mb_w * f.mb_h;
      for (size_t s = 0; s < f.deferred.size(); s++) {
        alignas (16) lh264_mb_t rec;
        // the walk first: parse_deferred below fills the picture the comparison reads
        Bufs b (f, f.deferred[s]);
        const SliceTask t = make_task (f, f.deferred[s], b);
        const SliceResult r = walk (t, b, &rec);
        int over_status = -1; bool over_clean = true; int over_limit = 0;
        if (s == 0 && f.deferred.size() > 1 && t.limit_mb - t.first_mb > 3) {
          Bufs b2 (f, f.deferred[s]);
          SliceTask t2 = make_task (f, f.deferred[s], b2);
          t2.limit_mb -= 3; over_limit = t2.limit_mb;
          over_status = walk (t2, b2, &rec).status;
          for (size_t k = (size_t)t2.limit_mb; k < n; k++) {
            const uint8_t* q = (const uint8_t*)&b2.mbs[k];
            for (size_t i = 0; i < sizeof (lh264_mb_t); i++) if (q[i]) over_clean = false;
            for (int i = 0; i < 384; i++) if (b2.coeffs[k * 384 + (size_t)i]) over_clean = false;
          }
        }
        const bool ok = P.parse_deferred (f, s);
        slices++;
        if (f.deferred[s].cabac) cabac++;
        if ((r.status == 0) != ok) { printf ("%s: picture %d slice %zu: status %d, the host %s\n", argv[a], f.id, s, r.status, ok ? "parses" : "fails"); bad++; continue; }
        if (!ok) { failed++; continue; }
        const DeferredSlice& d = f.deferred[s];
        const lh264_slice_t& hs = f.slices[(size_t)d.sid];
        size_t last = (size_t)hs.first_mb + (size_t)hs.n_mbs;
        if (last > (size_t)t.limit_mb) last = (size_t)t.limit_mb;
        if (r.n_mbs != hs.n_mbs || (size_t)r.stop_bit != d.stop_bit || b.slices[d.sid].n_mbs != hs.n_mbs ||
            memcmp (b.mbs + hs.first_mb, f.mbs.data() + hs.first_mb, (last - (size_t)hs.first_mb) * sizeof (lh264_mb_t)) ||
            memcmp (b.coeffs + (size_t)hs.first_mb * 384, f.coeffs.data() + (size_t)hs.first_mb * 384, (last - (size_t)hs.first_mb) * 768)) {
          printf ("%s: picture %d slice %zu differs from the host parser's\n", argv[a], f.id, s); bad++;
        }
        if (over_status >= 0) {
          // the limit drawn in: either the slice ends in front of it anyway, or OVERRUN; never a byte at or beyond it
          overruns++;
          const bool expect_over = (size_t)hs.first_mb + (size_t)hs.n_mbs > (size_t)over_limit;
          if ((over_status == lh264slice::SLICE_OVERRUN) != expect_over || !over_clean) { printf ("%s: picture %d: overrun status %d, clean %d\n", argv[a], f.id, over_status, (int)over_clean); bad++; }
        }
      }
    }
  }
  printf ("%ld files, %ld slices, %ld of them CABAC (%ld the host fails on, %ld overrun runs), %ld mismatches\n", files, slices, cabac, failed, overruns, bad);
  delete T; delete TC;
  return bad ? 1 : 0;
}
