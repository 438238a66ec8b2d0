#!/usr/bin/env python
"""Write tests/golden/phyre_readout_grads.npz: the gradients of the REFERENCE's own PHYREReadout (slotformer/phyre_planning/models/readout.py)
on the fixture of tools/gen_golden_phyre_readout.py (`fixture_case` of tests/phyre_readout_cases.py) -- `calc_train_loss(...).backward()` with the
model in .eval(), so without dropout.

    python tools/gen_golden_phyre_readout_grads.py --reference PATH_TO_THE_REFERENCE_TREE

The reference is loaded by path with the stand-ins of gen_golden_phyre_readout.py (see there), and cast to float64 (`model.double()`), so the file
holds the gradients of the reference's arithmetic and not float32 rounding.  Stored: the loss, every vector gradient (biases, LayerNorm
parameters, CLS, cls_mlp.2.weight) in full, and of each matrix its first 16 rows plus the float64 Frobenius norm of the whole -- results only, no
reference code; the file stays well under 1 MB."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

ROWS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('SLOTFORMER_REFERENCE'), required='SLOTFORMER_REFERENCE' not in os.environ)
    args = ap.parse_args()
    import phyre_readout_cases as cases
    from gen_golden_phyre_readout import load_by_path
    base = os.path.join(args.reference, 'slotformer')
    nerv = [('nerv', {}), ('nerv.training', {'BaseModel': torch.nn.Module, 'BaseParams': object})]
    savi = [('slotformer', {}), ('slotformer.base_slots', {}), ('slotformer.base_slots.models', {'StoSAVi': object})]
    vp = load_by_path('reference_slotformer', os.path.join(base, 'video_prediction', 'models', 'slotformer.py'), nerv + savi)
    for name, _ in savi:
        del sys.modules[name]
    nerv += [('nerv.models', {}), ('nerv.models.transformer', {'build_pos_enc': vp.build_pos_enc})]
    ref = load_by_path('reference_phyre_readout', os.path.join(base, 'phyre_planning', 'models', 'readout.py'), nerv)
    rd, sd, slots, labels = cases.fixture_case()
    model = ref.PHYREReadout(dict(rd)).eval()
    own = model.state_dict()
    model.load_state_dict({k: (own[k] if k == 'enc_t_pe' else sd[k]) for k in own})
    model = model.double()
    data = {'slots': torch.from_numpy(slots).double(), 'label': torch.from_numpy(labels).double()}
    loss = model.calc_train_loss(data, model(data))['vqa_loss']
    loss.backward()
    out = {'loss': np.float64(loss.item()), 'rows': np.int64(ROWS)}
    keys = []
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.numpy()
        keys.append(k)
        if g.ndim == 2 and g.shape[0] > 1:
            out['head.' + k] = g[:ROWS].copy()
            out['norm.' + k] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
        else:
            out['full.' + k] = g.copy()
    out['keys'] = np.array(json.dumps(keys))
    path = os.path.join(ROOT, 'tests', 'golden', 'phyre_readout_grads.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes; loss', float(out['loss']), len(keys), 'gradients')


if __name__ == '__main__':
    main()
