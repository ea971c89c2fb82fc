// TEST INFRASTRUCTURE ONLY (oracle/): a flat C entry point onto the REFERENCE's own arithmetic coder - DynProb, Branch<n>,
// ArithmeticCodedOutput::emitBit / emitBits / emitBitsZeroToPow2Inclusive and CompressionStream::emitInt / emitUEGkInt
// (codec/decoder/core/inc/compression_stream.h) over vpx_writer (bitwriter.h) - included from where they lie and linked from the
// libraries oracle/Makefile builds out of /root/reference.  tests/test_coder_synth.py codes the same symbols through this and
// through oracle/liboracle.so (orc_coder_symbols) and requires identical bytes.  Nothing here is product code.
//
// A record is {kind, cell, value, tag}: `cell` numbers the prior the symbol is coded with (records with the same kind and cell share
// it; the caller maps the product's (table, index) priors to cells), kinds:
//   0 IntPrior<3,4> (DC)   1 UnsignedIntPrior<3,4> (nonzero count)   2 UEGkIntPrior<14,4,2,4,0> (coefficient, tags tag+1..tag+4 as
//   encode4x4 names them; its EXP tag is touched first, decode_slice.cpp:2083)   3 UEGkIntPrior<9,4,3,4,3> (motion vector difference)
//   4..12 Branch<1..9> tree   13 / 14 emitBitsZeroToPow2Inclusive<3> / <7> (preferred value in `aux`)   15 one bit   16 raw bits
//   (emitBits, width in `aux`); trees and POW2 priors of one cell share one array of DynProbs
// CompressionStream's constructor builds the whole MacroblockModel (GBs of tables); emitInt / emitUEGkInt only use tag() and its map
// of tagged streams, so the stream object here is raw storage with only that map constructed.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <new>
#include <vector>

#include "compression_stream.h"

extern "C" {

struct refc_rec { int32_t kind, cell, value, tag, aux; };

// codes n records; afterwards refc_tag(tag, &len) gives the bytes of every tag (vpx_stop_encode done), NULL if the tag was never used
static std::map<int32_t, std::vector<uint8_t>> g_out;

int refc_code (const refc_rec* r, long n) {
  g_out.clear();
  ArithmeticCodedOutput::TEST_PROB = DynProb();
  void* mem = calloc (1, sizeof (CompressionStream));
  CompressionStream* cs = (CompressionStream*)mem;
  new (&cs->taggedStreams) std::map<int32_t, ArithmeticCodedOutput>();
  std::map<int32_t, IntPrior<3, 4>> dc;
  std::map<int32_t, UnsignedIntPrior<3, 4>> nz;
  std::map<int32_t, UEGkIntPrior<14, 4, 2, 4, 0>> ac;
  std::map<int32_t, UEGkIntPrior<9, 4, 3, 4, 3>> mvd;
  std::map<int32_t, Sirikata::Array1d<DynProb, 512>> trees;       // a tree of n bits uses the first 2^n - 1, a POW2 prior the first 2^n
  std::map<int32_t, DynProb> bits;
  int rc = 0;
  for (long i = 0; i < n && rc == 0; i++) {
    const refc_rec& s = r[i];
    switch (s.kind) {
    case 0: cs->emitInt (s.value, &dc[s.cell], s.tag); break;
    case 1: cs->emitInt (s.value, &nz[s.cell], s.tag); break;
    case 2:
      cs->tag (s.tag + 2);
      cs->emitUEGkInt (s.value, &ac[s.cell], s.tag + 2, s.tag + 3, s.tag + 1, s.tag + 4);
      break;
    case 3: cs->emitUEGkInt (s.value, &mvd[s.cell], s.tag); break;
#define TREE(NB) case 3 + NB: cs->tag (s.tag).emitBits<NB> ((uint32_t) (uint16_t)s.value & ((1u << NB) - 1u), Branch<NB> (trees[s.cell].slice<0, (1 << NB) - 1>())); break;
    TREE (1) TREE (2) TREE (3) TREE (4) TREE (5) TREE (6) TREE (7) TREE (8) TREE (9)
#undef TREE
    case 13: cs->tag (s.tag).emitBitsZeroToPow2Inclusive<3> ((uint32_t) (uint16_t)s.value, trees[s.cell].slice<0, 8>(), (uint32_t)s.aux); break;
    case 14: cs->tag (s.tag).emitBitsZeroToPow2Inclusive<7> ((uint32_t) (uint16_t)s.value, trees[s.cell].slice<0, 128>(), (uint32_t)s.aux); break;
    case 15: cs->tag (s.tag).emitBit (s.value != 0, &bits[s.cell]); break;
    case 16: cs->tag (s.tag).emitBits ((uint16_t)s.value, s.aux); break;
    default: rc = -1;
    }
  }
  for (auto& t : cs->taggedStreams) {
    vpx_stop_encode (&t.second.writer);
    g_out[t.first].assign (t.second.buffer.begin(), t.second.buffer.begin() + t.second.writer.pos);
  }
  cs->taggedStreams.~map();
  free (mem);
  return rc;
}

const uint8_t* refc_tag (int tag, long* len) {
  auto it = g_out.find (tag);
  if (it == g_out.end()) { *len = 0; return nullptr; }
  *len = (long)it->second.size();
  return it->second.data();
}

}  // extern "C"
