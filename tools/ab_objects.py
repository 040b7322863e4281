"""Everything the host object path returns (tests/object_path_probe.py: llsm_analyze / llsm_analyze_batch /
llsm_synthesize / llsm_synthesize_batch on small chunks, two blocks, a frameless utterance, a replaced frame, deep copies,
use_l1) for ONE library under the environment's setting of the route switches, for A/B runs of host-side changes.

    LLSM_PACKED_FRAMES=1 LLSM_AMD_LIB=/path/to/parent.so python tools/ab_objects.py parent_p1.npz
    LLSM_PACKED_FRAMES=1 python tools/ab_objects.py new_p1.npz
    python tools/ab_objects.py --compare parent_p1.npz new_p1.npz

One process per library and setting (the switches are read once): LLSM_PACKED_FRAMES 0 / 1 / 2, LLSM_FRAME_SLABS and
LLSM_OUTPUT_POOL both 0 / both 1.  --compare needs no GPU: it holds two such files to the same keys and the same bytes in
every array, and exits 1 otherwise (tools/ab_rows.py's comparison).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        from ab_rows import compare
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    from object_path_probe import collect
    res = collect()
    np.savez(sys.argv[1], **res)
    print(f"{len(res) - 1} arrays of {res['library']} -> {sys.argv[1]}")
