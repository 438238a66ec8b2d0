#!/usr/bin/env python
"""harness.rollout_video_slots at a frame offset: one engine call for all phases (one_call=True) against one call per phase
(one_call=False, the reference's restatement) -- the rollout drivers' job at the reference's shapes.

    python tools/bench_rollout_phases.py [--windows 3] [--seconds 1.0] [--out FILE.md]

Both forms run in one process, alternating window by window; a window is at least `--seconds` of back-to-back calls that end in a device
synchronise, after a warm-up of every shape; the figure is the median over the windows of the time per call.  Prints a markdown table
(and writes it to --out)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from slotformer_amd import _lib, configs, harness  # noqa: E402
from slotformer_amd.video_prediction.models import SlotRollouter  # noqa: E402


class Model:
    """what rollout_video_slots asks of a SlotFormer: the rollouter behind `{'slots'} -> {'pred_slots'}` (slotformer.py:152-159)"""

    def __init__(self, rollouter):
        self.rollouter, self.history_len, self.rollout_len = rollouter, rollouter.history_len, 0
        self.device = next(rollouter.parameters()).device

    def eval(self):
        return self

    def __call__(self, data):
        return {'pred_slots': self.rollouter(data['slots'][:, :self.history_len], self.rollout_len)}


# name, rollouter configuration, observed frames, target length, frame offset (slotformer_clevrer_params.py / slotformer_physion_params.py)
JOBS = [('CLEVRER (C2, 7 x 128, hist 6)', configs.C2_ROLL, 128, 160, 2), ('Physion (C4_ROLL_REF, 6 x 192, hist 15)', configs.C4_ROLL_REF, 45, 150, 3)]


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_rollout_phases: needs a GPU (a CPU run measures nothing)')
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    old_tok = lib.sf_get_layer_tok()
    rows = ['| job | B | layer_tok | one call per phase (ms) | one call (ms) | speed-up | windows (ms): per phase / one call | max rel. difference |',
            '|---|---|---|---|---|---|---|---|']
    try:
        with torch.no_grad():
            for name, cfg, obs, target, f in JOBS:
                torch.manual_seed(0)
                model = Model(SlotRollouter(**cfg['rollout_dict']).eval().to(dev))
                rd = cfg['rollout_dict']
                for B in args.batches:
                    ori = torch.randn(B, obs, rd['num_slots'], rd['slot_size'], device=dev)
                    for tok in (0, 1):
                        lib.sf_set_layer_tok(tok)
                        forms = {k: (lambda k=k: harness.rollout_video_slots(model, ori, f, obs_frames=obs, target_len=target, one_call=k))
                                 for k in (False, True)}
                        outs = {k: fn() for k, fn in forms.items()}   # warm-up, and the results compared at the timed shape
                        diff = ((outs[True] - outs[False]).abs().max() / outs[False].abs().max()).item()
                        n = {k: max(2, int(args.seconds / window(fn, 3)) + 1) for k, fn in forms.items()}
                        t = {False: [], True: []}
                        for _ in range(args.windows):
                            for k in (False, True):   # alternating
                                t[k].append(window(forms[k], n[k]) * 1e3)
                        a, b = statistics.median(t[False]), statistics.median(t[True])
                        rows.append(f'| {name} {obs} -> {target}, f = {f} | {B} | {"on" if tok else "off"} | {a:.2f} | {b:.2f} | {a / b:.2f} x | '
                                    f'{" ".join(f"{x:.2f}" for x in t[False])} / {" ".join(f"{x:.2f}" for x in t[True])} | {diff:.1e} |')
                        print(rows[-1], flush=True)
    finally:
        lib.sf_set_layer_tok(old_tok)
    table = '\n'.join(rows)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(table + '\n')


if __name__ == '__main__':
    main()
