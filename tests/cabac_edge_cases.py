"""What tests/test_cabac_edges.py and tests/test_cabac_edges_gpu.py share: the committed CABAC syntax-edge streams
(tests/golden/cabac_edge/, written by tests/golden/make_cabac_edge_streams.py with tests/h264_synth_cabac.py), the reference's recorded
verdict on them (tests/golden/cabac_edge_ref.json) and the helpers of edge_cases.py bound to this set."""
import json
import os

import edge_cases as E
import golden_io

DIR = os.path.join(golden_io.GOLDEN_DIR, "cabac_edge")
REF = json.load(open(os.path.join(golden_io.GOLDEN_DIR, "cabac_edge_ref.json")))
NAMES = sorted(REF)
REFUSED = {"cabac_refidx16"}                                    # 16 active references: carried by the escape stream only
NOT_REFUSED = [n for n in NAMES if n not in REFUSED]
TAG_ESC = 71
# files that differ from the reference's, by tag, as edge_cases.FILES_DIFFER
FILES_DIFFER = {}
# Conformant streams that the reference decodes, and whose files this code writes byte for byte as the reference does, but that the
# reference does not give back from its own files: {name: (its restore's exit status, part of what it said last, the reason)}.  The
# reference's restore direction is the decoder run again with the model as the source of symbols, and its encoder-side CABAC state
# (EncoderState in its decode_slice.cpp) covers less than its decoder.  The property here stays: what compress accepts restores to the
# input on every path.
REFERENCE_DOES_NOT_RESTORE = {
    "cabac_pcm": (-6, "computeNeighborPriorsCabac(): Assertion `0' failed", "its CABAC writer has no case for I_PCM (it says: Invalid type 512)"),
    "cabac_qp": (-6, "failed to open input", "holds an I_PCM macroblock too: its restore loses its place at it and asks for a tag file that compress did not write"),
    "cabac_sigmap": (-6, "stack smashing detected", "its restore overruns a buffer of its own on the 8x8 blocks with a single coefficient at each of the 64 positions"),
    "cabac_skip": (-6, "Invalid decoded macroblock type", "the 1x1 stream behind the 40x30 one: it throws its priors out at the change of size and reads a macroblock type that does not exist"),
    "cabac_mixed": (-6, "Assertion `i1 < s1' failed", "a prior index past the end of one of its tables, in the second picture (the first CAVLC one behind a CABAC one)"),
    "cabac_levels": (0, "", "its decoder refuses the levels on the way back (DecodeCurrentAccessUnit() failed in frame 0); it ends well with the parameter sets alone"),
    "cabac_carry": (0, "", "as cabac_levels: levels of several thousand; it ends well with the parameter sets and the first picture"),
}


def data(name):
    return E.data(name, DIR)


def made():
    return E.made("make_cabac_edge_streams")


def parsed(name):
    return E.parsed(name, DIR)


def cpu_compress(name):
    return E.cpu_compress(name, DIR)


def same_as_reference_files(name, main, tags):
    return E.same_as_reference_files(name, main, tags, REF, FILES_DIFFER)
