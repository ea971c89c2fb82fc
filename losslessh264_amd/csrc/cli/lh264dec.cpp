// lh264dec.cpp - console application with the calling convention of the reference's (codec/console/dec/src/h264dec.cpp:150-178,
// 79-121): the file names decide the mode.
//
//   lh264dec in.264 out.pip [out.yuv]   compress: out.pip = default stream, out.pip.<tag> = tagged streams (GPU); the optional
//                                       YUV dump = cropped I420 pictures through the ISVCDecoder object of the same library
//   lh264dec in.pip out.264             restore the original bytes from in.pip + in.pip.<tag>                  (host)
//   lh264dec in.264 out.lhp             compress into ONE container file; restored and compared before it is written, a
//                                       stream the round trip cannot carry is stored verbatim
//   lh264dec in.lhp out.264             restore from the container
//   lh264dec --segment-mbs N ...               (first) streams of more than N macroblocks are coded in segments of whole pictures
//   lh264dec --escapes ...                     (first) a stream with an mb_skip_run above 511 or 16 active references is compressed with
//                                       the escape stream beside it (out.pip.71, or in the container) and not refused / stored verbatim
//   lh264dec --tolerant ...                    (first) LH264_COMPRESS_TOLERANT: NAL units the format drops (delimiters, filler, ...) are kept and pictures
//                                       with lost slices are compressed; the container modes still restore, compare and fall back to verbatim
//   lh264dec --batch out_dir a.264 b.264 ...   many streams in one lh264_compress_batch call -> out_dir/<name>.lhp
//   lh264dec --decode [--nv12] out_dir a.264 b.264 ...   many streams in one lh264_decode_batch call -> out_dir/<name>.yuv: the
//                                       cropped pictures as I420 (or NV12), appended by a sink run by run (the file's size bounds nothing)
//   lh264dec --decode --sha1 [--nv12] out_dir a.264 ...   digests only, no .yuv: out_dir/<name>.sha1 with a line `index width height
//                                       frame_num idr hex` per picture and a last line `stream hex`, the SHA-1 of all of them in order
//   lh264dec --decode [--sha1] --scale N ...   N = 1 | 2 | 3: reduced-size pictures, the means of 2x2 / 4x4 / 8x8 blocks computed on the
//                                       device (lh264.h: scale_log2); 0 = full size
//   lh264dec --decode [--sha1] --at SPEC ...   only the pictures with the given numbers (decode order from 0) are delivered: SPEC is a,b,c
//                                       or start:stop:step (lh264.h: lh264_decode_batch_ex5); of the stream only what they need is
//                                       decoded, and nothing behind the last of them is read.  One SPEC for all files.  Not together
//                                       with --pick or --conceal
//   lh264dec --decode [--sha1] --pick intra|idr ...   only the pictures whose slices are all I slices / the IDR pictures are decoded and
//                                       written (lh264.h: pick); the index column of a .sha1 file is the picture's number in the stream.
//   lh264dec --decode [--sha1] --size WxH ...   every picture of every stream is written W x H (both even, 2..4096), resampled on the
//                                       device by an exact area average (lh264.h: out_width, out_height).  Not with a non-zero --scale
//                                       Not together with --conceal
//   lh264dec --decode [--sha1] --size WxH --filter area|bilinear|bicubic ...   the filter of that resampling (lh264.h:
//                                       lh264_decode_batch_ex6): the area average (the default), or an antialiased triangle / Catmull-Rom
//                                       kernel.  bilinear and bicubic need --size
//   lh264dec --decode [--sha1] [--crop x,y,w,h] [--size WxH --fit cover|contain [--fill y,cb,cr]] ...   fitted views (lh264.h:
//                                       lh264_decode_batch_ex3): a rectangle of every picture's window in the window's place; the largest
//                                       centred part of it with the size's aspect (cover), or the whole of it inside the size, the rest
//                                       filled (contain; default 16,128,128)
//   lh264dec --decode [--sha1] --rgb rgb24|rgbp --sample f32|f16|bf16 [--mul a,b,c] [--add a,b,c] ...   float RGB pictures, cast and
//                                       normalised on the device (lh264.h: lh264_decode_batch_ex2) -> out_dir/<name>.f32 | .f16 | .bf16
//
// Written against include/lh264.h and include/lh264_isvc.h only; links liblh264.so.
#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "lh264.h"
#include "lh264_isvc.h"

typedef std::vector<uint8_t> Bytes;

static bool load (const std::string& p, Bytes& v) {
  FILE* f = fopen (p.c_str(), "rb");
  if (!f) return false;
  fseek (f, 0, SEEK_END); const long n = ftell (f); fseek (f, 0, SEEK_SET);
  v.resize (n > 0 ? (size_t)n : 0);
  const bool ok = n <= 0 || fread (v.data(), 1, (size_t)n, f) == (size_t)n;
  fclose (f);
  return ok;
}
static bool save (const std::string& p, const uint8_t* d, size_t n) {
  FILE* f = fopen (p.c_str(), "wb");
  if (!f) return false;
  const bool ok = n == 0 || fwrite (d, 1, n, f) == n;
  fclose (f);
  return ok;
}
static bool ends_with (const std::string& s, const char* e) { const size_t n = strlen (e); return s.size() >= n && s.compare (s.size() - n, n, e) == 0; }
static std::string base_name (const std::string& p) { const size_t k = p.find_last_of ('/'); return k == std::string::npos ? p : p.substr (k + 1); }

struct Compressed {
  lh264_compressed_t* h = nullptr;
  ~Compressed() { if (h) lh264_compressed_free (h); }
};

// the tagged streams of a compressed stream as the arrays lh264_pip_pack / lh264_pip_restore take
static void tag_arrays (const lh264_compressed_t* h, const uint8_t* tags[72], size_t len[72]) {
  for (int t = 0; t < 72; t++) tags[t] = lh264_compressed_tag (h, t, &len[t]);
}

static int dump_yuv (const Bytes& bs, const std::string& path) {
  FILE* out = fopen (path.c_str(), "wb");
  if (!out) { perror (path.c_str()); return 2; }
  ISVCDecoder* dec = NULL;
  if (WelsCreateDecoder (&dec) || !dec) { fprintf (stderr, "WelsCreateDecoder failed\n"); fclose (out); return 1; }
  SDecodingParam param; memset (&param, 0, sizeof (param));
  param.eOutputColorFormat = videoFormatI420; param.uiTargetDqLayer = (unsigned char) - 1; param.eEcActiveIdc = ERROR_CON_SLICE_COPY;
  param.sVideoProperty.size = sizeof (param.sVideoProperty); param.sVideoProperty.eVideoBsType = VIDEO_BITSTREAM_DEFAULT;
  if (dec->Initialize (&param)) { fprintf (stderr, "decoder Initialize failed (no GPU?)\n"); WelsDestroyDecoder (dec); fclose (out); return 3; }
  auto emit = [&] (unsigned char** dst, const SBufferInfo& info) {
    if (info.iBufferStatus != 1) return;
    const int w = info.UsrData.sSystemBuffer.iWidth, h = info.UsrData.sSystemBuffer.iHeight;
    for (int p = 0; p < 3; p++) {
      const int pw = p ? w / 2 : w, ph = p ? h / 2 : h, st = info.UsrData.sSystemBuffer.iStride[p ? 1 : 0];
      for (int y = 0; y < ph; y++) fwrite (dst[p] + (size_t)y * st, 1, (size_t)pw, out);
    }
  };
  size_t pos = 0;
  while (pos < bs.size()) {                     // one start-code-delimited chunk per call, as h264dec.cpp:246-272
    size_t i;
    for (i = 1; pos + i + 2 < bs.size(); i++)
      if (bs[pos + i] == 0 && bs[pos + i + 1] == 0 && (bs[pos + i + 2] == 1 || (pos + i + 3 < bs.size() && bs[pos + i + 2] == 0 && bs[pos + i + 3] == 1))) break;
    if (pos + i + 2 >= bs.size()) i = bs.size() - pos;
    unsigned char* dst[3] = {0, 0, 0}; SBufferInfo info; memset (&info, 0, sizeof (info));
    if (i >= 4) { dec->DecodeFrameNoDelay (bs.data() + pos, (int)i, dst, &info); emit (dst, info); }
    pos += i;
  }
  unsigned char* dst[3] = {0, 0, 0}; SBufferInfo info; memset (&info, 0, sizeof (info));
  dec->DecodeFrame2 (NULL, 0, dst, &info); emit (dst, info);
  dec->Uninitialize(); WelsDestroyDecoder (dec);
  fclose (out);
  return 0;
}

// --segment-mbs N: streams of more macroblocks are coded in segments of at most N (whole pictures); 0: the library's default
// --escapes: LH264_COMPRESS_ESCAPES; --tolerant: LH264_COMPRESS_TOLERANT
static lh264_compress_opts_t g_opts = {sizeof (lh264_compress_opts_t), 0, 0};

static int compress_files (const std::string& src, const std::string& dst, const char* yuv) {
  Bytes in;
  if (!load (src, in)) { perror (src.c_str()); return 2; }
  const uint8_t* d = in.data(); const size_t n = in.size();
  Compressed c;
  if (lh264_compress_batch_opts (&d, &n, 1, 0, &g_opts, &c.h) != LH264_OK || lh264_compressed_status (c.h) != LH264_OK) {
    fprintf (stderr, "cannot compress %s: %s\n", src.c_str(), c.h ? lh264_compressed_error (c.h) : lh264_last_error());
    return 1;
  }
  size_t ml; const uint8_t* m = lh264_compressed_main (c.h, &ml);
  if (!save (dst, m, ml)) { perror (dst.c_str()); return 2; }
  size_t total = ml;
  for (int t = 0; t < 72; t++) {
    size_t tl; const uint8_t* p = lh264_compressed_tag (c.h, t, &tl);
    if (p) { if (!save (dst + "." + std::to_string (t), p, tl)) { perror (dst.c_str()); return 2; } total += tl; }
  }
  printf ("%s: %zu bytes -> %zu bytes (%.4f), %d pictures\n", src.c_str(), n, total, n ? (double)total / (double)n : 0.0, lh264_compressed_pictures (c.h));
  return yuv ? dump_yuv (in, yuv) : 0;
}

static int restore_files (const std::string& src, const std::string& dst) {
  Bytes m;
  if (!load (src, m)) { perror (src.c_str()); return 2; }
  std::vector<Bytes> tb (72); const uint8_t* tags[72]; size_t len[72]; int nt = 0;
  for (int t = 0; t < 72; t++) { const bool h = load (src + "." + std::to_string (t), tb[t]); tags[t] = h ? (tb[t].empty() ? (const uint8_t*)"" : tb[t].data()) : nullptr; len[t] = tb[t].size(); nt += h; }
  size_t need = 0;
  Bytes out (64);
  int rc = lh264_pip_restore (m.data(), m.size(), tags, len, 72, out.data(), out.size(), &need);
  if (rc == LH264_E_ARG && need > out.size()) { out.resize (need); rc = lh264_pip_restore (m.data(), m.size(), tags, len, 72, out.data(), out.size(), &need); }
  if (rc != LH264_OK) { fprintf (stderr, "cannot restore %s: %s\n", src.c_str(), lh264_restore_error()); return 1; }
  if (!save (dst, out.data(), need)) { perror (dst.c_str()); return 2; }
  printf ("%s (+%d tagged streams) -> %s: %zu bytes\n", src.c_str(), nt, dst.c_str(), need);
  return 0;
}

// container for one already compressed (or failed) stream: verified, verbatim when the round trip does not hold or does not pay
static bool make_container (const Bytes& in, const lh264_compressed_t* h, Bytes& blob, std::string& why) {
  why.clear();
  if (h && lh264_compressed_status (h) == LH264_OK && lh264_compressed_pictures (h) > 0) {
    size_t ml; const uint8_t* m = lh264_compressed_main (h, &ml);
    const uint8_t* tags[72]; size_t len[72];
    tag_arrays (h, tags, len);
    Bytes back (in.size() + 64); size_t bl = 0;
    if (lh264_pip_restore (m, ml, tags, len, 72, back.data(), back.size(), &bl) == LH264_OK && bl == in.size() && memcmp (back.data(), in.data(), bl) == 0) {
      blob.resize (lh264_pip_pack_bound (ml, len, 72));
      size_t n = 0;
      if (lh264_pip_pack (m, ml, tags, len, 72, 0, blob.data(), blob.size(), &n) == LH264_OK) { blob.resize (n); if (n < in.size() + 32) return true; why = "no gain"; }
    } else why = "the restored stream differs";
  } else why = h ? lh264_compressed_error (h) : "not compressed";
  if (why.empty()) why = "no picture";
  blob.resize (in.size() + 64);
  size_t n = 0;
  if (lh264_pip_pack (in.data(), in.size(), nullptr, nullptr, 0, LH264_PIP_VERBATIM, blob.data(), blob.size(), &n) != LH264_OK) return false;
  blob.resize (n);
  return true;
}

static int compress_single (const std::vector<std::string>& srcs, const std::vector<std::string>& dsts) {
  const int n = (int)srcs.size();
  std::vector<Bytes> in (n);
  std::vector<const uint8_t*> d (n); std::vector<size_t> l (n);
  for (int i = 0; i < n; i++) { if (!load (srcs[i], in[i])) { perror (srcs[i].c_str()); return 2; } d[i] = in[i].data(); l[i] = in[i].size(); }
  std::vector<lh264_compressed_t*> h (n, nullptr);
  // every device of the node takes a share of the batch
  const int nd = lh264_device_count();
  std::vector<int> devs;
  for (int i = 0; i < nd && i < n; i++) devs.push_back (i);
  const int rc = devs.size() > 1 ? lh264_compress_batch_devices_opts (d.data(), l.data(), n, 0, devs.data(), (int)devs.size(), &g_opts, h.data())
                                 : lh264_compress_batch_opts (d.data(), l.data(), n, 0, &g_opts, h.data());
  int ret = 0;
  for (int i = 0; i < n; i++) {
    Bytes blob; std::string why;
    if (!make_container (in[i], rc == LH264_OK ? h[i] : nullptr, blob, why) || !save (dsts[i], blob.data(), blob.size())) { fprintf (stderr, "cannot write %s\n", dsts[i].c_str()); ret = 2; }
    else printf ("%s: %zu bytes -> %zu bytes (%.4f)%s%s%s\n", srcs[i].c_str(), in[i].size(), blob.size(), in[i].empty() ? 0.0 : (double)blob.size() / (double)in[i].size(),
                 why.empty() ? "" : "  [verbatim: ", why.c_str(), why.empty() ? "" : "]");
    if (h[i]) lh264_compressed_free (h[i]);
  }
  return ret;
}

// --decode: one lh264_decode_batch over all inputs, a sink that appends every run of pictures to its stream's file
struct DecodeFiles { std::vector<FILE*> f; std::vector<size_t> bytes; };
static int decode_sink (void* user, int stream, int, int, const lh264_decoded_pic_t*, const uint8_t* bytes, size_t len) {
  DecodeFiles& d = * (DecodeFiles*)user;
  if (len && fwrite (bytes, 1, len, d.f[stream]) != len) return 1;
  d.bytes[stream] += len;
  return 0;
}
// the names of `lh264dec --decode --conceal METHOD` (and of decode_batch (conceal=...) in Python)
static int conceal_method (const char* name) {
  static const struct { const char* n; int m; } k[] = {
    {"off", LH264_CONCEAL_OFF}, {"slice_copy", LH264_CONCEAL_SLICE_COPY}, {"slice_copy_cross_idr", LH264_CONCEAL_SLICE_COPY_CROSS_IDR},
    {"slice_copy_cross_idr_freeze", LH264_CONCEAL_SLICE_COPY_CROSS_IDR_FREEZE}, {"mv_copy", LH264_CONCEAL_SLICE_MV_COPY_CROSS_IDR},
    {"mv_copy_freeze", LH264_CONCEAL_SLICE_MV_COPY_CROSS_IDR_FREEZE}};
  for (const auto& e : k) if (!strcmp (name, e.n)) return e.m;
  return -1;
}
// --rgb rgb24|rgbp [--matrix M] [--range R]: what lh264_decode_batch_ex takes beside the options (colour 0: lh264_decode_batch as ever)
static lh264_decode_ext_t g_ext = {sizeof (lh264_decode_ext_t), LH264_COLOUR_YUV, LH264_MATRIX_AUTO, LH264_RANGE_AUTO, 0, 0};
static const char* const kRgbUsage = "--rgb: rgb24 | rgbp, not with --nv12; --matrix: auto | bt601 | bt709 and --range: auto | limited | full, with --rgb only";
static int one_of (const char* text, const char* a, const char* b, const char* c) {      // 0, 1, 2 or -1
  return !strcmp (text, a) ? 0 : !strcmp (text, b) ? 1 : c && !strcmp (text, c) ? 2 : -1;
}
// --sample f32|f16|bf16 [--mul a,b,c] [--add a,b,c]: what lh264_decode_batch_ex2 takes beside both (type 0: lh264_decode_batch_ex as ever)
static lh264_decode_sample_t g_sample = {sizeof (lh264_decode_sample_t), LH264_SAMPLE_U8, {0, 0, 0}, {0, 0, 0}};
static const char* const kSampleUsage = "--sample: f32 | f16 | bf16, with --rgb only; --mul and --add: three finite numbers a,b,c (R, G, B), with --sample only";
static bool parse_three (const char* text, float* v) {      // "a,b,c", every one finite as binary32
  for (int k = 0; k < 3; k++) {
    if (!*text || *text == ' ' || *text == ',') return false;
    char* end = nullptr;
    const float x = (float)strtod (text, &end);
    if (end == text || *end != (k < 2 ? ',' : 0) || !std::isfinite (x)) return false;
    v[k] = x;
    text = end + 1;
  }
  return true;
}
// [--crop x,y,w,h] [--fit cover|contain [--fill y,cb,cr]]: what lh264_decode_batch_ex3 takes beside the three (nothing named: NULL, the
// call as ever)
static lh264_rect_t g_crop = {0, 0, 0, 0};
static lh264_decode_view_t g_view = {sizeof (lh264_decode_view_t), LH264_FIT_STRETCH, 0, 0, nullptr, 0, 0};
static bool g_view_named = false;
static const char* const kViewUsage = "--fit: cover | contain, with --size only; --fill: y,cb,cr in 0..255, with --fit contain only; --crop: x,y,w,h, four even numbers, x, y >= 0, w, h >= 2";
static bool parse_ints (const char* text, int n, int top, int* v) {      // "a,b,..": n numbers in 0..top
  for (int k = 0; k < n; k++) {
    int digits = 0; v[k] = 0;
    for (; *text >= '0' && *text <= '9'; text++) { if (++digits > 5) return false; v[k] = v[k] * 10 + (*text - '0'); }
    if (!digits || v[k] > top || *text != (k < n - 1 ? ',' : 0)) return false;
    text++;
  }
  return true;
}
static const lh264_decode_view_t* view_arg() { return g_view_named ? &g_view : nullptr; }
// --filter area|bilinear|bicubic: what lh264_decode_batch_ex6 takes beside the six (area: NULL, the call as ever)
static lh264_decode_filter_t g_filter = {sizeof (lh264_decode_filter_t), LH264_FILTER_AREA, 0, 0};
static const char* const kFilterUsage = "--filter: area | bilinear | bicubic; bilinear and bicubic with --size only";
static const lh264_decode_filter_t* filter_arg() { return g_filter.filter != LH264_FILTER_AREA ? &g_filter : nullptr; }
static const char* out_suffix() {
  return !g_ext.colour ? ".yuv" : g_sample.type == LH264_SAMPLE_F32 ? ".f32" : g_sample.type == LH264_SAMPLE_F16 ? ".f16" : g_sample.type == LH264_SAMPLE_BF16 ? ".bf16" : ".rgb";
}
// --size WxH: both even, 2..4096
static const char* const kSizeUsage = "--size: WxH, both even, 2..4096; not with a non-zero --scale";
static bool parse_size (const char* text, int* w, int* h) {
  int v[2] = {0, 0}, k = 0, digits = 0;
  for (const char* c = text; *c; c++) {
    if (*c == 'x' && k == 0 && digits) { k = 1; digits = 0; continue; }
    if (*c < '0' || *c > '9' || ++digits > 4) return false;
    v[k] = v[k] * 10 + (*c - '0');
  }
  if (k != 1 || !digits) return false;
  for (int q = 0; q < 2; q++) if (v[q] < 2 || v[q] > 4096 || (v[q] & 1)) return false;
  *w = v[0]; *h = v[1];
  return true;
}
// --motion | --motion-only: what lh264_decode_batch_ex4 takes beside the four (0: NULL, the call as ever); 2: the fields and no picture
static int g_motion = 0;
static const char* const kMotionUsage = "--motion, --motion-only: not with --sha1";
// --at SPEC: the selection lh264_decode_batch_ex5 takes beside the five (NULL without it), one entry for every file.  SPEC is a,b,c
// (strictly increasing numbers) or start:stop:step with start, stop and step optional (stop: exclusive, none: to the stream's end)
static std::vector<int32_t> g_at_list;
static lh264_select_t g_at = {nullptr, 0, 0, 0, 1};
static lh264_decode_select_t g_select = {sizeof (lh264_decode_select_t), 0, &g_at, 0};
static const char* const kAtUsage = "--at: a,b,c (strictly increasing picture numbers) | start:stop:step (stop, step optional); not with --pick or --conceal";
static const lh264_decode_select_t* select_arg() { return g_select.n_selects ? &g_select : nullptr; }
static bool parse_at (const char* v) {
  auto number = [] (const char*& p, long long* out) {      // digits, at most nine of them
    const char* b = p; long long x = 0;
    while (*p >= '0' && *p <= '9' && p - b < 10) x = x * 10 + (*p++ - '0');
    *out = x;
    return p != b && p - b < 10;
  };
  g_at_list.clear();
  g_at = {nullptr, 0, 0, 0, 1};
  if (strchr (v, ':')) {
    long long part[3] = {0, -1, 1};
    const char* p = v;
    for (int k = 0; k < 3; k++) {
      if (*p != ':' && *p != 0 && !number (p, &part[k])) return false;
      if (*p == 0) break;
      if (*p != ':' || k == 2) return false;
      p++;
    }
    if (part[2] < 1) return false;
    g_at.first = (uint32_t)part[0]; g_at.step = (uint32_t)part[2];
    if (part[1] >= 0) {
      g_at.count = part[1] > part[0] ? (uint32_t) ((part[1] - part[0] + part[2] - 1) / part[2]) : 0;
      if (!g_at.count) { g_at_list.reserve (1); g_at.list = g_at_list.data(); }      // (an empty range: the empty list)
    }
  } else {
    const char* p = v;
    for (;;) {
      long long x;
      if (!number (p, &x) || (!g_at_list.empty() && x <= g_at_list.back())) return false;
      g_at_list.push_back ((int32_t)x);
      if (*p == 0) break;
      if (*p++ != ',') return false;
    }
    g_at.list = g_at_list.data(); g_at.n_list = (uint32_t)g_at_list.size();
  }
  g_select.n_selects = 1;
  return true;
}
static int decode_files (const std::string& out_dir, const std::vector<std::string>& srcs, bool nv12, int conceal, int device_parse /* 0 host, 1 device, 2 device with CABAC */, int scale, uint32_t pick, int out_w, int out_h) {
  const int n = (int)srcs.size();
  std::vector<Bytes> in (n);
  std::vector<const uint8_t*> d (n); std::vector<size_t> l (n);
  for (int i = 0; i < n; i++) { if (!load (srcs[i], in[i])) { perror (srcs[i].c_str()); return 2; } d[i] = in[i].data(); l[i] = in[i].size(); }
  DecodeFiles files; files.f.assign (n, nullptr); files.bytes.assign (n, 0);
  std::vector<std::string> dsts (n);
  for (int i = 0; i < n && g_motion != 2; i++) {
    dsts[i] = out_dir + "/" + base_name (srcs[i]) + out_suffix();
    files.f[i] = fopen (dsts[i].c_str(), "wb");
    if (!files.f[i]) { perror (dsts[i].c_str()); for (FILE* f : files.f) if (f) fclose (f); return 2; }
  }
  lh264_decode_opts_t o; memset (&o, 0, sizeof (o));
  o.struct_bytes = sizeof (o); o.format = nv12 ? LH264_FMT_NV12 : LH264_FMT_I420; o.sink = decode_sink; o.user = &files; o.conceal = (uint32_t)conceal; o.parse = device_parse ? LH264_PARSE_DEVICE : LH264_PARSE_HOST; o.parse_flags = device_parse == 2 ? LH264_PARSE_FLAG_CABAC : 0; o.scale_log2 = (uint32_t)scale; o.pick = pick; o.out_width = (uint32_t)out_w; o.out_height = (uint32_t)out_h;
  if (g_motion == 2) { o.sink = nullptr; o.user = nullptr; o.flags = LH264_DECODE_NO_PICTURES; }
  const lh264_decode_motion_t motion = {sizeof (lh264_decode_motion_t), LH264_MOTION_FIELDS, 0, 0};
  std::vector<lh264_decoded_t*> h (n, nullptr);
  const int rc = lh264_decode_batch_ex6 (d.data(), l.data(), n, 0, &o, g_ext.colour ? &g_ext : nullptr, g_sample.type ? &g_sample : nullptr, view_arg(), g_motion ? &motion : nullptr, select_arg(), filter_arg(), h.data());
  for (FILE* f : files.f) if (f) fclose (f);
  if (rc != LH264_OK) { fprintf (stderr, "lh264_decode_batch failed: %d%s\n", rc, rc == LH264_E_NODEVICE ? " (no HIP device visible)" : ""); return 1; }
  int ret = 0;
  for (int i = 0; i < n; i++) {
    const int st = lh264_decoded_status (h[i]);
    if (g_motion) {
      // the stream's motion blocks and macroblock blocks, as the handle holds them: <name>.mv and <name>.mbi
      const int16_t* mv = nullptr; const uint8_t* mbi = nullptr; size_t mv_bytes = 0, mbi_bytes = 0;
      const std::string stem = out_dir + "/" + base_name (srcs[i]);
      if (lh264_decoded_motion (h[i], &mv, &mv_bytes, &mbi, &mbi_bytes) != LH264_OK || !save (stem + ".mv", (const uint8_t*)mv, mv_bytes) || !save (stem + ".mbi", mbi, mbi_bytes)) { fprintf (stderr, "cannot write %s.mv / .mbi\n", stem.c_str()); ret = 2; }
      if (g_motion == 2) { dsts[i] = stem + ".mv"; files.bytes[i] = mv_bytes + mbi_bytes; }
    }
    printf ("%s -> %s: %d pictures, %zu bytes%s%s\n", srcs[i].c_str(), dsts[i].c_str(), lh264_decoded_pictures (h[i]), files.bytes[i], st == LH264_OK ? "" : "  [stopped: ", st == LH264_OK ? "" : (std::string (lh264_decoded_error (h[i])) + "]").c_str());
    if (st != LH264_OK) ret = 1;
    lh264_decoded_free (h[i]);
  }
  return ret;
}

// --decode --sha1: one digests-only lh264_decode_batch; no picture leaves the device
static std::string hex20 (const uint8_t* d) { char b[41]; for (int k = 0; k < 20; k++) snprintf (b + 2 * k, 3, "%02x", d[k]); return std::string (b, 40); }
static int decode_sha1_files (const std::string& out_dir, const std::vector<std::string>& srcs, bool nv12, int conceal, int device_parse /* 0 host, 1 device, 2 device with CABAC */, int scale, uint32_t pick, int out_w, int out_h) {
  const int n = (int)srcs.size();
  std::vector<Bytes> in (n);
  std::vector<const uint8_t*> d (n); std::vector<size_t> l (n);
  for (int i = 0; i < n; i++) { if (!load (srcs[i], in[i])) { perror (srcs[i].c_str()); return 2; } d[i] = in[i].data(); l[i] = in[i].size(); }
  lh264_decode_opts_t o; memset (&o, 0, sizeof (o));
  o.struct_bytes = sizeof (o); o.format = nv12 ? LH264_FMT_NV12 : LH264_FMT_I420; o.conceal = (uint32_t)conceal; o.parse = device_parse ? LH264_PARSE_DEVICE : LH264_PARSE_HOST; o.parse_flags = device_parse == 2 ? LH264_PARSE_FLAG_CABAC : 0; o.scale_log2 = (uint32_t)scale; o.pick = pick; o.out_width = (uint32_t)out_w; o.out_height = (uint32_t)out_h;
  o.flags = LH264_DECODE_SHA1_PICTURES | LH264_DECODE_SHA1_STREAM | LH264_DECODE_NO_PICTURES;
  std::vector<lh264_decoded_t*> h (n, nullptr);
  const int rc = lh264_decode_batch_ex6 (d.data(), l.data(), n, 0, &o, g_ext.colour ? &g_ext : nullptr, g_sample.type ? &g_sample : nullptr, view_arg(), nullptr, select_arg(), filter_arg(), h.data());
  if (rc != LH264_OK) { fprintf (stderr, "lh264_decode_batch failed: %d%s\n", rc, rc == LH264_E_NODEVICE ? " (no HIP device visible)" : ""); return 1; }
  int ret = 0;
  for (int i = 0; i < n; i++) {
    const int st = lh264_decoded_status (h[i]);
    const std::string dst = out_dir + "/" + base_name (srcs[i]) + ".sha1";
    FILE* f = fopen (dst.c_str(), "w");
    if (!f) { perror (dst.c_str()); ret = 2; lh264_decoded_free (h[i]); continue; }
    uint8_t dig[20];
    const int np = lh264_decoded_pictures (h[i]);
    for (int k = 0; k < np; k++) {
      lh264_decoded_pic_t p;
      if (lh264_decoded_picture (h[i], k, &p) != LH264_OK || lh264_decoded_picture_sha1 (h[i], k, dig) != LH264_OK) { ret = 1; break; }
      fprintf (f, "%d %d %d %d %d %s\n", lh264_decoded_picture_index (h[i], k), p.width, p.height, p.frame_num, p.idr, hex20 (dig).c_str());
    }
    std::string total;
    if (lh264_decoded_stream_sha1 (h[i], dig) == LH264_OK) { total = hex20 (dig); fprintf (f, "stream %s\n", total.c_str()); } else ret = 1;
    fclose (f);
    printf ("%s -> %s: %d pictures, stream %s%s%s\n", srcs[i].c_str(), dst.c_str(), np, total.c_str(), st == LH264_OK ? "" : "  [stopped: ", st == LH264_OK ? "" : (std::string (lh264_decoded_error (h[i])) + "]").c_str());
    if (st != LH264_OK) ret = 1;
    lh264_decoded_free (h[i]);
  }
  return ret;
}

static int restore_single (const std::string& src, const std::string& dst) {
  Bytes f;
  if (!load (src, f)) { perror (src.c_str()); return 2; }
  size_t need = 0;
  Bytes out (64);
  int rc = lh264_pip_restore_file (f.data(), f.size(), out.data(), out.size(), &need);
  if (rc == LH264_E_ARG && need > out.size()) { out.resize (need); rc = lh264_pip_restore_file (f.data(), f.size(), out.data(), out.size(), &need); }
  if (rc != LH264_OK) { fprintf (stderr, "cannot restore %s: %s\n", src.c_str(), lh264_restore_error()); return 1; }
  if (!save (dst, out.data(), need)) { perror (dst.c_str()); return 2; }
  printf ("%s -> %s: %zu bytes\n", src.c_str(), dst.c_str(), need);
  return 0;
}

int main (int argc, char** argv) {
  for (;;) {                                    // the options that go first, in any order
    if (argc >= 3 && !strcmp (argv[1], "--segment-mbs")) { g_opts.segment_mbs = strtoull (argv[2], nullptr, 10); argv[2] = argv[0]; argv += 2; argc -= 2; }
    else if (argc >= 2 && !strcmp (argv[1], "--escapes")) { g_opts.reserved |= LH264_COMPRESS_ESCAPES; argv[1] = argv[0]; argv += 1; argc -= 1; }
    else if (argc >= 2 && !strcmp (argv[1], "--tolerant")) { g_opts.reserved |= LH264_COMPRESS_TOLERANT; argv[1] = argv[0]; argv += 1; argc -= 1; }
    else break;
  }
  if (argc >= 4 && !strcmp (argv[1], "--batch")) {
    std::vector<std::string> srcs, dsts;
    for (int i = 3; i < argc; i++) { srcs.push_back (argv[i]); dsts.push_back (std::string (argv[2]) + "/" + base_name (argv[i]) + ".lhp"); }
    return compress_single (srcs, dsts);
  }
  if (argc >= 4 && !strcmp (argv[1], "--decode")) {
    bool fill_named = false;
    bool nv12 = false, sha1 = false; int device_parse = 0, conceal = 0, scale = 0, out_w = 0, out_h = 0, first = 2; uint32_t pick = LH264_PICK_ALL; bool matrix_named = false, add_named = false, mul_named = false;
    for (;;) {
      if (first < argc && !strcmp (argv[first], "--nv12")) { nv12 = true; first++; }
      else if (first < argc && !strcmp (argv[first], "--sha1")) { sha1 = true; first++; }
      else if (first < argc && !strcmp (argv[first], "--motion")) { if (!g_motion) g_motion = 1; first++; }
      else if (first < argc && !strcmp (argv[first], "--motion-only")) { g_motion = 2; first++; }
      else if (first < argc && !strcmp (argv[first], "--device-parse")) { if (!device_parse) device_parse = 1; first++; }
      else if (first < argc && !strcmp (argv[first], "--device-parse-cabac")) { device_parse = 2; first++; }
      else if (first + 1 < argc && !strcmp (argv[first], "--conceal")) {
        conceal = conceal_method (argv[first + 1]);
        if (conceal < 0) { fprintf (stderr, "--conceal: off | slice_copy | slice_copy_cross_idr | slice_copy_cross_idr_freeze | mv_copy | mv_copy_freeze\n"); return 2; }
        first += 2;
      } else if (first + 1 < argc && !strcmp (argv[first], "--scale")) {
        if (strlen (argv[first + 1]) != 1 || argv[first + 1][0] < '0' || argv[first + 1][0] > '3') { fprintf (stderr, "--scale: 0 | 1 | 2 | 3\n"); return 2; }
        scale = argv[first + 1][0] - '0';
        first += 2;
      } else if (first + 1 < argc && !strcmp (argv[first], "--pick")) {
        if (!strcmp (argv[first + 1], "intra")) pick = LH264_PICK_INTRA;
        else if (!strcmp (argv[first + 1], "idr")) pick = LH264_PICK_IDR;
        else { fprintf (stderr, "--pick: intra | idr\n"); return 2; }
        first += 2;
      } else if (first < argc && !strcmp (argv[first], "--at")) {
        if (first + 1 >= argc || !parse_at (argv[first + 1])) { fprintf (stderr, "%s\n", kAtUsage); return 2; }
        first += 2;
      } else if (first + 1 < argc && !strcmp (argv[first], "--size")) {
        if (!parse_size (argv[first + 1], &out_w, &out_h)) { fprintf (stderr, "%s\n", kSizeUsage); return 2; }
        first += 2;
      } else if (first < argc && !strcmp (argv[first], "--filter")) {
        const int k = one_of (first + 1 < argc ? argv[first + 1] : "", "area", "bilinear", "bicubic");
        if (k < 0) { fprintf (stderr, "%s\n", kFilterUsage); return 2; }
        g_filter.filter = (uint32_t)k;
        first += 2;
      } else if (first < argc && (!strcmp (argv[first], "--rgb") || !strcmp (argv[first], "--matrix") || !strcmp (argv[first], "--range"))) {
        const char* v = first + 1 < argc ? argv[first + 1] : "";
        const bool rgb = !strcmp (argv[first], "--rgb"), matrix = !strcmp (argv[first], "--matrix");
        const int k = rgb ? one_of (v, "rgb24", "rgbp", nullptr) : matrix ? one_of (v, "auto", "bt601", "bt709") : one_of (v, "auto", "limited", "full");
        if (k < 0) { fprintf (stderr, "%s\n", kRgbUsage); return 2; }
        if (rgb) g_ext.colour = (uint32_t)k + LH264_COLOUR_RGB24;
        else { (matrix ? g_ext.matrix : g_ext.range) = (uint32_t)k; matrix_named = true; }
        first += 2;
      } else if (first < argc && (!strcmp (argv[first], "--fit") || !strcmp (argv[first], "--fill") || !strcmp (argv[first], "--crop"))) {
        const char* v = first + 1 < argc ? argv[first + 1] : "";
        int q[4] = {0, 0, 0, 0};
        if (!strcmp (argv[first], "--fit")) {
          const int k = one_of (v, "cover", "contain", nullptr);
          if (k < 0) { fprintf (stderr, "%s\n", kViewUsage); return 2; }
          g_view.fit = (uint32_t)k + LH264_FIT_COVER;
        } else if (!strcmp (argv[first], "--fill")) {
          if (!parse_ints (v, 3, 255, q)) { fprintf (stderr, "%s\n", kViewUsage); return 2; }
          g_view.fill = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16; fill_named = true;
        } else {
          if (!parse_ints (v, 4, 16384, q) || ((q[0] | q[1] | q[2] | q[3]) & 1) || q[2] < 2 || q[3] < 2) { fprintf (stderr, "%s\n", kViewUsage); return 2; }
          g_crop = {q[0], q[1], q[2], q[3]}; g_view.n_crops = 1; g_view.crops = &g_crop;
        }
        g_view_named = true;
        first += 2;
      } else if (first < argc && (!strcmp (argv[first], "--sample") || !strcmp (argv[first], "--mul") || !strcmp (argv[first], "--add"))) {
        const char* v = first + 1 < argc ? argv[first + 1] : "";
        if (!strcmp (argv[first], "--sample")) {
          const int k = one_of (v, "f32", "f16", "bf16");
          if (k < 0) { fprintf (stderr, "%s\n", kSampleUsage); return 2; }
          g_sample.type = (uint32_t)k + LH264_SAMPLE_F32;
        } else {
          if (!parse_three (v, !strcmp (argv[first], "--mul") ? g_sample.mul : g_sample.add)) { fprintf (stderr, "%s\n", kSampleUsage); return 2; }
          (!strcmp (argv[first], "--mul") ? mul_named : add_named) = true;
        }
        first += 2;
      } else break;
    }
    if ((g_ext.colour && nv12) || (!g_ext.colour && matrix_named)) { fprintf (stderr, "%s\n", kRgbUsage); return 2; }
    if ((g_sample.type && !g_ext.colour) || (!g_sample.type && (add_named || mul_named))) { fprintf (stderr, "%s\n", kSampleUsage); return 2; }
    if (g_sample.type && !mul_named) g_sample.mul[0] = g_sample.mul[1] = g_sample.mul[2] = 1.0f;
    if (out_w && scale) { fprintf (stderr, "%s\n", kSizeUsage); return 2; }
    if (filter_arg() && !out_w) { fprintf (stderr, "%s\n", kFilterUsage); return 2; }
    if (g_motion && sha1) { fprintf (stderr, "%s\n", kMotionUsage); return 2; }
    if ((g_view.fit != LH264_FIT_STRETCH && !out_w) || (fill_named && g_view.fit != LH264_FIT_CONTAIN)) { fprintf (stderr, "%s\n", kViewUsage); return 2; }
    if (g_view.fit == LH264_FIT_CONTAIN && !fill_named) g_view.fill = 16u | 128u << 8 | 128u << 16;
    if (select_arg() && (pick != LH264_PICK_ALL || conceal != 0)) { fprintf (stderr, "%s\n", kAtUsage); return 2; }
    // (--pick with --conceal: concealment copies from the picture decoded before, which is not decoded)
    if (argc < first + 2 || (pick != LH264_PICK_ALL && conceal != 0)) { fprintf (stderr, "usage: %s --decode [--device-parse | --device-parse-cabac] [--sha1 | --motion | --motion-only] [--nv12] [--conceal METHOD | --pick intra|idr | --at SPEC] [--crop x,y,w,h] [--scale N | --size WxH [--filter area|bilinear|bicubic] [--fit cover|contain [--fill y,cb,cr]]] [--rgb rgb24|rgbp [--matrix M] [--range R] [--sample f32|f16|bf16 [--mul a,b,c] [--add a,b,c]]] out_dir in.264...\n", argv[0]); return 2; }
    std::vector<std::string> srcs;
    for (int i = first + 1; i < argc; i++) srcs.push_back (argv[i]);
    return sha1 ? decode_sha1_files (argv[first], srcs, nv12, conceal, device_parse, scale, pick, out_w, out_h) : decode_files (argv[first], srcs, nv12, conceal, device_parse, scale, pick, out_w, out_h);
  }
  if (argc < 3) {
    fprintf (stderr, "usage: %s [--segment-mbs N] [--escapes] [--tolerant] in.264 out.pip [out.yuv] | in.pip out.264 | in.264 out.lhp | in.lhp out.264 | --batch out_dir in.264... | --decode [--device-parse | --device-parse-cabac] [--sha1 | --motion | --motion-only] [--nv12] [--conceal METHOD | --pick intra|idr | --at SPEC] [--crop x,y,w,h] [--scale N | --size WxH [--filter area|bilinear|bicubic] [--fit cover|contain [--fill y,cb,cr]]] [--rgb rgb24|rgbp [--matrix M] [--range R] [--sample f32|f16|bf16 [--mul a,b,c] [--add a,b,c]]] out_dir in.264...\n", argv[0]);
    return 2;
  }
  const std::string a = argv[1], b = argv[2];
  if (ends_with (a, ".lhp")) return restore_single (a, b);
  if (ends_with (b, ".lhp")) return compress_single ({a}, {b});
  if (base_name (a).find (".pip") != std::string::npos) return restore_files (a, b);      // as the reference decides (h264dec.cpp:167-173)
  return compress_files (a, b, argc > 3 ? argv[3] : nullptr);
}
