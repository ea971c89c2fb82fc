"""Writes the inputs of tools/slice_parse_check.cpp that are not files in the repository - the 20 damaged CAVLC streams of
tests/slice_parse_cases.py and the 20 damaged CABAC streams of tests/slice_parse_cabac_cases.py - into a directory, and prints the
checker's whole argument list: every committed stream (tests/golden/streams, edge, cabac_edge, escape, slice_parse,
slice_parse_cabac) and the files written.  So the figures of DESIGN.md section 4.4 can be taken again:

    python tools/slice_parse_dump_cases.py /tmp/cases > /tmp/cases/list
    xargs ./slice_parse_check < /tmp/cases/list
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import slice_parse_cases as K  # noqa: E402


def main(out):
    import slice_parse_cabac_cases as KC
    os.makedirs(out, exist_ok=True)
    paths = [p for _, p in K.committed()]
    d = os.path.join(K.GOLDEN, "slice_parse_cabac")
    paths += [os.path.join(d, f) for f in sorted(os.listdir(d))]
    for prefix, cases in (("cavlc", K.damaged_cases()), ("cabac", KC.damaged_cases())):
        for label, data in cases:
            p = os.path.join(out, "%s_%s.264" % (prefix, label))
            open(p, "wb").write(data)
            paths.append(p)
    print("\n".join(paths))


if __name__ == "__main__":
    main(sys.argv[1])
