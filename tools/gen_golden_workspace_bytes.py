#!/usr/bin/env python
"""Writes tests/golden/workspace_bytes.json: what tests/test_workspace_bytes.py's record() returns from the library SF_LIB_PATH names.
    SF_LIB_PATH=<build of the commit the fixture pins>/slotformer_amd/libslotformer_hip.so python tools/gen_golden_workspace_bytes.py
The fixture pins a PARENT's byte counts: never run this against the tree whose carves are under test.  CPU only."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

if __name__ == '__main__':
    if not os.environ.get('SF_LIB_PATH'):
        sys.exit('set SF_LIB_PATH to the library of the commit the fixture pins')
    from slotformer_amd import _lib
    import test_workspace_bytes as t
    lib = _lib.lib()
    lib.sf_set_precision(1)
    with open(t.GOLDEN, 'w') as f:
        json.dump(t.record(lib), f, indent=0, sort_keys=True)
        f.write('\n')
    print(t.GOLDEN)
