#!/usr/bin/env python
"""Write tests/golden/vp_metrics.npz: the REFERENCE's own adjusted_rand_index (both modes), miou_metric and mse_metric on the seeded blob masks
and frames of tests/test_vp_metrics.py (fixture_masks / fixture_frames, 64 x 64 and 128 x 128), and for each the largest distance between the
reference's result and the float64 restatement of that test file (`<name>_ref_minus_f64`): the reference evaluates the ARI in float32 on counts
up to 2.7e8, so it is not exact, and the tests allow twice that distance.

    python tools/gen_golden_vp_metrics.py --reference PATH_TO_THE_REFERENCE_TREE

The reference's vp_utils.py is loaded by path; it imports skimage.metrics, torchvision.ops and slotformer.base_slots.models at its top, which are
replaced by empty stand-in modules here.  Only functions that need none of them are called, so SSIM, PSNR (skimage) and the box metrics
(torchvision) have NO reference-generated fixture: they are held to the float64 restatements alone.  Only results are written, no reference code."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def load_reference(path):
    for name, attrs in (('skimage', ()), ('skimage.metrics', ('structural_similarity', 'peak_signal_noise_ratio')), ('torchvision', ()),
                        ('torchvision.ops', ()), ('slotformer', ()), ('slotformer.base_slots', ()),
                        ('slotformer.base_slots.models', ('to_rgb_from_tensor', ))):
        if name not in sys.modules or name.startswith('slotformer'):
            m = types.ModuleType(name)
            for a in attrs:
                setattr(m, a, None)
            sys.modules[name] = m
    spec = importlib.util.spec_from_file_location('reference_vp_utils', os.path.join(path, 'slotformer', 'video_prediction', 'vp_utils.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('SLOTFORMER_REFERENCE'), required='SLOTFORMER_REFERENCE' not in os.environ)
    args = ap.parse_args()
    import test_vp_metrics as t   # before the stand-ins: it imports the project's own packages
    ref = load_reference(args.reference)
    out = {}
    for res in (64, 128):
        gt, pm = t.fixture_masks(res)
        tabs = [t.table_of(a, b) for a, b in zip(gt, pm)]
        tg, tp = torch.from_numpy(gt), torch.from_numpy(pm)
        for name, fg in (('ari', False), ('fari', True)):
            r = ref.adjusted_rand_index(tg, tp, ignore_background=fg).double().numpy()
            f64 = np.array([t.ari_of(x, fg) for x in tabs])
            out[f'{name}_{res}'], out[f'{name}_{res}_ref_minus_f64'] = r, np.abs(r - f64).max()
        r = float(ref.miou_metric(tg, tp))
        out[f'miou_{res}'], out[f'miou_{res}_ref_minus_f64'] = np.float64(r), np.float64(abs(r - np.mean([t.miou_of(x) for x in tabs])))
        x, y = t.fixture_frames(res)
        r = float(ref.mse_metric(x, y))
        f64 = ((x.astype(np.float64) - y.astype(np.float64))**2).sum(-1).sum(-1).mean()
        out[f'mse_{res}'], out[f'mse_{res}_ref_minus_f64'] = np.float64(r), np.float64(abs(r - f64))
    for k in sorted(out):
        if k.endswith('ref_minus_f64'):
            print(f'{k}: {float(out[k]):.3e}')
    np.savez(os.path.join(ROOT, 'tests', 'golden', 'vp_metrics.npz'), **out)


if __name__ == '__main__':
    main()
