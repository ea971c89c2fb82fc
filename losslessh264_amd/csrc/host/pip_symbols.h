// pip_symbols.h - host side of SURVEY section 8 row a10: turns the parsed macroblock syntax of a stream into the ordered
// list of (prior table, prior index, value, tag) symbols the recompressor codes for everything that is not a residual
// coefficient.  The coefficient symbols (row a8) are produced on the device and spliced in at the marker.
// What must be reproduced of the reference: WHICH prior codes WHICH value in WHICH order and to which tag - the per-macroblock
// emit code of WelsDecodeSliceForNonRecoding (decoder/core/src/decode_slice.cpp:2174-2473) and the prior selection of
// MacroblockModel (decoder/core/src/macroblock_model.cpp:370-645), including its history image FreqImage
// (decoder/core/inc/decoded_macroblock.h:106-192).
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "../../../include/lh264.h"
#include "h264_parser.h"

namespace lh264host {

// bits of each prior table's binary tree (Branch<n>), by LH264_TB_*; 0: the table has none.  A TREE symbol holds 0 .. 2^n - 1, a POW2
// symbol (emitBitsZeroToPow2Inclusive<n>) 0 .. 2^n.  One table for the symbolizer's range guard and for both restorers
constexpr int kTreeBits[LH264_TB_COUNT] = {4, 0, 3, 0, 0, 0, 0, 0, 0, 9, 7, 8, 4, 2, 4, 0, 0, 4};

// The part of a SKIPRUN / NUMREF value its tree drops (value >> kTreeBits[table]), as stream LH264_TAG_ESC of the container carries it
// (include/lh264.h: entries of four LEB128 varints: table, gap, high, repeat).  symbol() sees every tree symbol of the two tables in
// coding order; a run of equal nonzero high parts is one entry
class EscapeLog {
 public:
  void symbol (int table, uint32_t value);
  // the stream so far, with the runs still open closed (SKIPRUN first, then NUMREF); empty: no value was out of range
  std::vector<uint8_t> finished() const;
 private:
  struct Run { uint64_t gap = 0, high = 0, repeat = 0; };   // repeat 0: none open
  std::vector<uint8_t> bytes_;
  Run open_[2];
  uint64_t since_[2] = {0, 0};          // symbols of the table behind its last entry
  static void append (std::vector<uint8_t>& v, int table, const Run& r);
};

class Symbolizer {
 public:
  // appends the picture's symbols to f.syn_syms / f.syn_off (pictures of one stream, in decode order)
  void picture (FrameOut& f);
  // empty, or the first value met that its prior table cannot carry ("mb_skip_run 687 is outside the container's range 0..511"): the
  // symbols of such a stream do not restore it
  const std::string& out_of_range() const { return out_of_range_; }
  // whether the escape stream carries EVERY value that was out of range - a stream for which it does restores from its symbols plus
  // that stream; not so a value of another table, more than 16 references, a run beyond any picture -, and the escape stream of the
  // pictures so far (EscapeLog::finished); empty when it would not restore the stream
  std::vector<uint8_t> escapes() const { return beyond_escapes_ ? std::vector<uint8_t>() : escapes_.finished(); }
  bool escapes_carry_all() const { return !beyond_escapes_; }

 private:
  std::string out_of_range_;
  EscapeLog escapes_;
  bool beyond_escapes_ = false;
  struct Cell {                       // what the model remembers of a macroblock (DecodedMacroblock, decoded_macroblock.h:4-34)
    uint8_t initialized = 0, zeroed = 0, cbp_c = 0, cbp_l = 0, chroma_mode = 0, luma16_mode = 0;
    uint16_t cached_skips = 0;
    uint32_t mb_type = 0, num_ref = 0;
  };
  std::vector<Cell> img_[2];
  int img_w_ = 0, img_h_ = 0, cur_ = 0, last_frame_id_ = 0;
  std::vector<int8_t> ipm_;           // the decoder's pIntraPredMode[mb][0..6] (raw modes of the bottom row / right column)
  std::vector<uint8_t> nxn_;          // macroblock is I4x4 / I8x8
  std::vector<lh264_ctx_sym_t> flat_; std::vector<uint32_t> start_, cnt_;   // scratch of picture()
  void update_frame (int frame_id);
};

}  // namespace lh264host
