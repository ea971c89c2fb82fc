// h264_cabac_ctx_tables.h - the context-index tables of the CABAC residual blocks (9.3.3.1.3, Table 9-43 and Table 9-34), defined in
// h264_parser.cpp: for the host parser and for the walk that restates it (lh264_slice_cabac.h)
#pragma once
#include <stdint.h>
namespace lh264host {
// ctxIdxInc of significant_coeff_flag (frame coded) and last_significant_coeff_flag for 8x8 blocks, Table 9-43
extern const uint8_t kSig8x8[63], kLast8x8[63];
// per ctxBlockCat 0..4: the offsets of coded_block_flag, of the significance maps and of coeff_abs_level_minus1 within their context ranges
extern const uint8_t kCatCbf[5], kCatMap[5], kCatAbs[5];
}  // namespace lh264host
