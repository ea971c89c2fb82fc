// lh264_restore.h - what the host passes of the device restore (csrc/host/pip_restore.cpp) and its kernel (lh264_restore.hip)
// share: the slice descriptor pass 1 records, the CAVLC and CABAC tables, and the per-stream job of one kernel workgroup.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define LH264R_HD __host__ __device__
#else
#define LH264R_HD
#endif

namespace lh264r {

// what the model and the writers read of a slice header (Parser::HeaderInfo), in stream order
struct RestoreSlice {
  int32_t mb_w, mb_h, first_mb, slice_type, frame_num, slice_qp, num_ref_idx_l0;
  uint8_t transform_8x8, constrained_intra_pred;
  uint8_t cabac;                       // 0: a CAVLC slice; else 1 | cabac_init_idc << 1
  uint8_t phase;                       // CAVLC: hdr_bits & 7, where the slice data starts in its byte; CABAC: 0 (the data starts on a byte)
};
static_assert (sizeof (RestoreSlice) == 32, "RestoreSlice layout");

// the tables of pip_restore.cpp's Restorer, flattened for the device (built by lh264host::restore_tables); a length of 0 = the
// host's lookup finds nothing and writes nothing
struct RestoreTables {
  int32_t cell[18], tree_bits[18];     // kCell / kTreeBits by LH264_TB_*
  uint16_t tok_code[5][17][4];         // coeff_token by (table, total_coeff, trailing_ones)
  uint16_t tz_code[16][16];            // total_zeros by (total_coeff, zeros_left)
  uint16_t rb_code[8][16];             // run_before by (min (zeros_left, 7), run)
  uint8_t tok_len[5][17][4];
  uint8_t tz_len[16][16];
  uint8_t tzc_code[4][4], tzc_len[4][4];   // chroma DC total_zeros
  uint8_t rb_len[8][16];
  uint8_t cbp_code[2][48];             // coded_block_pattern -> codeNum: [0] intra, [1] inter
  uint8_t zz4[16], zz8[64];            // kZigzag4x4 / kZigzag8x8 (the writer's scans)
  uint8_t zz16[16], zz64[64];          // kZz16 / kZz64 (the model's scan position -> level index)
  uint8_t scan8[16], cache30[16], z2raster[16], chroma_nzc[2][4];
};
static_assert (sizeof (RestoreTables) % 4 == 0, "RestoreTables is copied by words");

// the tables of the CABAC writer (h264_cabac_tables.h and pip_restore.cpp's), as the CAVLC ones above; built by
// lh264host::restore_cabac_tables.  The encoder reads `enc` for every bin (the kernel keeps a copy in LDS), `init` once per slice
struct RestoreCabacEnc {
  uint8_t range_lps[64][4], next_lps[64], next_mps[64];   // kCabacRangeLps / kCabacNextLps / kCabacNextMps
  uint8_t sig8x8[64], last8x8[64];                        // kSig8x8 / kLast8x8 (63 used)
  uint8_t cat_cbf[8], cat_map[8], cat_abs[8];             // kCatCbf / kCatMap / kCatAbs (5 used)
};
struct RestoreCabacTables {
  RestoreCabacEnc enc;
  int8_t init[460][4][2];              // kCabacInit: (m, n) by context and column (0: I slices, 1 + cabac_init_idc: P slices)
};
static_assert (sizeof (RestoreCabacEnc) % 4 == 0 && sizeof (RestoreCabacTables) % 4 == 0, "the CABAC tables are copied by words");

// The escape stream (include/lh264.h LH264_TAG_ESC) as pass 1 hands it to both restorers: the entries of each table in order, fixed
// width (a varint above 32 bits saturates: no stream has that many symbols).  And the state of one table while the symbols are read:
// `gap` symbols to go until the entry applies, then `rep` symbols that get `high`; rep 0: the table has no entry left.  cur: the
// next entry to load.  One step per SKIPRUN / NUMREF tree symbol, the same code in the host restore and in the kernel's chain
struct RestoreEscape { uint32_t gap, high, repeat; };
struct EscapeCursor { uint32_t gap, rep, high, cur; };
LH264R_HD inline void escape_load (EscapeCursor& c, const RestoreEscape* e, uint32_t n) {
  if (c.cur < n) { c.gap = e[c.cur].gap; c.high = e[c.cur].high; c.rep = e[c.cur].repeat; c.cur++; }
  else c.rep = 0;
}
LH264R_HD inline uint32_t escape_next (EscapeCursor& c, const RestoreEscape* e, uint32_t n) {      // the symbol's high part; c.rep != 0
  if (c.gap) { c.gap--; return 0; }
  const uint32_t h = c.high;
  if (--c.rep == 0) escape_load (c, e, n);
  return h;
}
// a restored value must fit an int: high parts above this are corrupt whatever the table
enum { kEscapeHighMax = 0x3fffff };

// status of one stream after the kernel; anything but RS_OK sends the stream to the host restore (LH264_RESTORE_PATH_FALLBACK)
enum { RS_OK = 0, RS_CORRUPT = 1, RS_STORE_FULL = 2, RS_OUT_FULL = 3 };

// one stream: its inputs, its work memory (sized by the host from pass 1) and its outputs, all in device memory
struct RestoreJob {
  const uint8_t* tags;                 // the tag streams, concatenated
  uint32_t tag_off[72], tag_len[72];
  uint32_t tag_present[3];             // bit t: tags[t] exists (tag LH264_TAG_PCM: the I_PCM samples)
  uint32_t n_slices, n_max;            // slices; the largest picture in macroblocks
  const RestoreSlice* slices;
  const RestoreEscape* esc[2];         // tag LH264_TAG_ESC by table: [0] SKIPRUN, [1] NUMREF (staged behind the tags)
  uint32_t n_esc[2];
  uint32_t esc_bad, pad;               // the tag is malformed: the stream ends with RS_CORRUPT and the host restore names the reason
  uint8_t* cells;                      // 2 x n_max Cell
  uint8_t* ws;                         // n_max WState (the kernel instance with the CABAC writer: its longer WState)
  int8_t* ipm;                         // n_max x 8
  uint8_t* nxn;                        // n_max
  uint32_t* hash;                      // slots x {key + 1, pool offset}; zeroed before the launch
  uint32_t* pool;                      // pool_cap packed DynProbs
  uint32_t slots, pool_cap;            // slots: a power of two
  uint8_t* out;                        // the slices' bits, each slice from a fresh byte and `phase` zero bits (a CABAC slice: its bytes)
  uint32_t out_cap;
  uint32_t* slice_end;                 // per slice: its end in out (bytes)
  int32_t* status;                     // [0] RS_*; [1] prior keys, [2] pool words, [3] output bytes used
};

}  // namespace lh264r
