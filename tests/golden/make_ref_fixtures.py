"""Extracts the data that two tests compare against from a libllsm2 source tree,
so that the tests run without one:

  ref_header_functions.txt  every llsm_* function that the reference's five
                            installed headers (makefile:132-135) declare, one
                            name per line (tests/test_abi.py)
  ref_cheby_tables.npz      the Chebyshev filter tables of filter-coef.h
                            (cheby_l_a, cheby_l_b, cheby_h_a, cheby_h_b;
                            48 x 5 each, float64; tests/test_oracle_dsp.py)

Only names and table values are kept: no source text.

Run:  python tests/golden/make_ref_fixtures.py /path/to/libllsm2
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADERS = ["llsm.h", "llsmrt.h", "dsputils.h", "llsmutils.h", "buffer.h"]


def header_functions(ref):
    names = set()
    for h in HEADERS:
        t = open(os.path.join(ref, h)).read()
        t = re.sub(r"/\*.*?\*/", "", t, flags=re.S); t = re.sub(r"//.*", "", t)
        names |= set(re.findall(r"\b(llsm_[a-zA-Z0-9_]+)\s*\(", t))
    return sorted(names)


def cheby_tables(ref):
    txt = open(os.path.join(ref, "filter-coef.h")).read()
    tabs = {}
    for name in ("cheby_l_a", "cheby_l_b", "cheby_h_a", "cheby_h_b"):
        m = re.search(name + r"\[240\]\s*=\s*\{([^}]*)\}", txt)
        tabs[name] = np.array([float(v) for v in m.group(1).replace("\n", " ").split(",") if v.strip()]).reshape(48, 5)
    return tabs


if __name__ == "__main__":
    ref = sys.argv[1]
    with open(os.path.join(HERE, "ref_header_functions.txt"), "w") as f:
        f.write("\n".join(header_functions(ref)) + "\n")
    np.savez(os.path.join(HERE, "ref_cheby_tables.npz"), **cheby_tables(ref))
