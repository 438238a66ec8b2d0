#!/usr/bin/env python
"""Write tests/golden/physion_readout.npz: the REFERENCE's own PhysionReadout (slotformer/physion_vqa/models/readout.py) on the seeded inputs of
tests/physion_readout_cases.py (`fixture_case`: N 6, C 192, F 192, B 4, T 5) for agg_func max / sum / mean -- its logits, `vqa_loss`, the `acc_*`
values of calc_eval_loss, the CPU-autograd gradients of the loss (every 4th row of dW1, to keep the file small), its state-dict keys and shapes,
and the settings of readout_physion_params.py as plain data.

    python tools/gen_golden_physion_readout.py --reference PATH_TO_THE_REFERENCE_TREE

The reference's readout.py is loaded by path; its one outside import (nerv.training.BaseModel) is replaced by a stand-in nn.Module.  Weights and
slots come from the seeded generator the tests share, so the file holds results only, no reference code."""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

DW1_ROW_STEP = 4


def load_by_path(name, path, stand_ins):
    for mod_name, attrs in stand_ins:
        m = types.ModuleType(mod_name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[mod_name] = m
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('SLOTFORMER_REFERENCE'), required='SLOTFORMER_REFERENCE' not in os.environ)
    args = ap.parse_args()
    import physion_readout_cases as cases
    base = os.path.join(args.reference, 'slotformer', 'physion_vqa')
    nerv = [('nerv', {}), ('nerv.training', {'BaseModel': torch.nn.Module, 'BaseParams': object})]
    ref = load_by_path('reference_readout', os.path.join(base, 'models', 'readout.py'), nerv)
    cfg = load_by_path('reference_readout_params', os.path.join(base, 'configs', 'readout_physion_params.py'), nerv).SlotFormerParams
    out = {'dW1_row_step': np.int64(DW1_ROW_STEP)}
    out['config'] = np.array(json.dumps(dict(readout_dict=cfg.readout_dict, video_len=cfg.video_len, lr=cfg.lr, max_epochs=cfg.max_epochs,
                                             train_batch_size=cfg.train_batch_size, val_batch_size=cfg.val_batch_size, optimizer=cfg.optimizer,
                                             warmup_steps_pct=cfg.warmup_steps_pct)))
    s = cases.FIXTURE_SHAPE
    for agg in cases.AGGS:
        slots, W1, b1, w2, b2, labels = cases.fixture_case(agg)
        model = ref.PhysionReadout(dict(num_slots=s['N'], slot_size=s['C'], agg_func=agg, feats_dim=s['F']))
        sd = model.state_dict()
        if agg == 'max':
            out['state_dict_keys'] = np.array(json.dumps([[k, list(v.shape)] for k, v in sd.items()]))
        model.load_state_dict({'comb_idx': sd['comb_idx'], 'linear1.weight': torch.from_numpy(W1[0]), 'linear1.bias': torch.from_numpy(b1[0]),
                               'linear2.weight': torch.from_numpy(w2[0])[None], 'linear2.bias': torch.from_numpy(b2)})
        data = {'slots': torch.from_numpy(slots), 'label': torch.from_numpy(labels)}
        res = model(data)
        loss = model.calc_train_loss(data, res)['vqa_loss']
        loss.backward()
        ev = model.calc_eval_loss(data, res)
        out[f'{agg}_logits'] = res['logits'].detach().numpy()
        out[f'{agg}_vqa_loss'] = np.float32(loss.item())
        out[f'{agg}_acc_keys'] = np.array(json.dumps([k for k in ev if k.startswith('acc_')]))
        out[f'{agg}_acc'] = np.array([float(v) for k, v in ev.items() if k.startswith('acc_')], np.float32)
        out[f'{agg}_dW1_rows'] = model.linear1.weight.grad.numpy()[::DW1_ROW_STEP]
        out[f'{agg}_db1'] = model.linear1.bias.grad.numpy()
        out[f'{agg}_dw2'] = model.linear2.weight.grad.numpy()[0]
        out[f'{agg}_db2'] = model.linear2.bias.grad.numpy()
    path = os.path.join(ROOT, 'tests', 'golden', 'physion_readout.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
