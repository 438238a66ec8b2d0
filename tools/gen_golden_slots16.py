#!/usr/bin/env python
"""Golden vectors of the 9 .. 16-slot cases (tests/slots16_cases.py) from the REFERENCE's own classes on CPU, through the case
functions of tools/gen_golden.py (same shims, same seeds-to-weights rule, same oracle cross-check).  Outputs only, under
tests/golden/: savi_n9, savi_n11, savi_n16, roll_n11, savi_train_n11.

    python tools/gen_golden_slots16.py [name ...]
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (puts the repository root and tests/ on sys.path)
import slots16_cases as sc  # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    want = set(sys.argv[1:])
    for table, fn in ((sc.SAVI_CASES, gg.case_savi), (sc.ROLL_CASES, gg.case_rollout), (sc.SAVI_TRAIN_CASES, gg.case_savi_train)):
        for name, (cfg, kw) in table.items():
            if not want or name in want:
                fn(name, cfg, **kw)


if __name__ == '__main__':
    main()
