#!/usr/bin/env python3
"""Fixture for tests/test_oracle_vs_ref.py: tests/golden/ref_kernels_sha1.json = per case the SHA-1 of the reference's outputs on
the case's seeded inputs.  Runs every case with the oracle and the reference's own kernels (oracle/_ref/libref_kernels.so, built by
oracle/Makefile), compares the two output by output and writes the digests.  Data only."""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import test_oracle_vs_ref as T  # noqa: E402


def main():
    ref = C.CDLL(os.path.join(O.ORACLE_DIR, "_ref", "libref_kernels.so"))    # static init of the reference builds its 8.78 GiB model (~30 s)
    out = {}
    for name, (case, args) in T.CASES.items():
        h = hashlib.sha1()
        case(O.lib(), ref, h, *args)
        out[name] = h.hexdigest()
        print(name, out[name])
    json.dump(out, open(os.path.join(HERE, "ref_kernels_sha1.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
