"""-m gpu: the routes of the host object path (capi.cpp analyze_block / synthesize_block) give the same
bits.  LLSM_PACKED_FRAMES chooses how a block's frames cross the link (0: eleven rows, 1: packed records the device writes
and reads in place, 2: packed records through staging, the default); LLSM_FRAME_SLABS and LLSM_OUTPUT_POOL choose heap or
slab frames and heap or pooled outputs.  The switches are read once per process, so each setting runs
tests/object_path_probe.py in a fresh child process; the default setting runs once per module."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("LLSM_PACKED_FRAMES", "LLSM_FRAME_SLABS", "LLSM_OUTPUT_POOL")
SETTINGS = {
    "rows": {"LLSM_PACKED_FRAMES": "0"},
    "records_in_place": {"LLSM_PACKED_FRAMES": "1"},
    "heap_everywhere": {"LLSM_FRAME_SLABS": "0", "LLSM_OUTPUT_POOL": "0"},
    "slabs_and_pool_everywhere": {"LLSM_FRAME_SLABS": "1", "LLSM_OUTPUT_POOL": "1"},
}
_default = {}


def probe(setting):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(setting)
    r = subprocess.run([sys.executable, os.path.join(HERE, "object_path_probe.py"), "--digests"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def default_digests():
    if not _default:
        _default.update(probe({}))
    return _default


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_every_route_gives_the_bits_of_the_default_route(name):
    """Every frame member of llsm_analyze_batch (f0_refine 0 and 1, two blocks, a frameless utterance) and of llsm_analyze,
    the F0 written back, the residuals, and every output sample of llsm_synthesize_batch (untouched chunks, a replaced frame,
    deep copies, use_l1) and of llsm_synthesize: bit for bit what the default setting gives; and every setting leaves no
    live slab and no live output byte behind."""
    want = default_digests()
    got = probe(SETTINGS[name])
    assert sorted(got) == sorted(want)
    assert sum(k.startswith("ana/") for k in got) >= 60 and sum(k.startswith("syn/") for k in got) >= 30
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, differ
    zero = ["int64", [1], hashlib.sha1(np.zeros(1, np.int64).tobytes()).hexdigest()]
    for d in (want, got):
        for k in ("end/slabs", "end/slab_bytes", "end/output_bytes"):
            assert d[k] == zero, k
