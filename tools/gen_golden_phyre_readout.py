#!/usr/bin/env python
"""Write tests/golden/phyre_readout.npz: the REFERENCE's own PHYREReadout (slotformer/phyre_planning/models/readout.py) with the settings of
readout_phyre_params-fold0.py on the seeded weights and slots of tests/phyre_readout_cases.py (`fixture_case`: 6 videos of 4 frames, 8 slots of
128) -- its logits, `vqa_loss`, the `acc_*` keys and values of calc_eval_loss, its state-dict keys and shapes, its `enc_t_pe` table, and the
config as plain data.

    python tools/gen_golden_phyre_readout.py --reference PATH_TO_THE_REFERENCE_TREE

The reference's readout.py is loaded by path.  Its outside imports are replaced: nerv.training.BaseModel by a stand-in nn.Module, and
nerv.models.transformer.build_pos_enc by the `build_pos_enc` of the reference's OWN video_prediction/models/slotformer.py, loaded by path too.
The nerv package is third-party and not part of the reference tree; its table is ASSUMED to be the same sinusoid the reference restates there
(last row = position 0, sines then cosines).  The model runs in
.eval(): its encoder layers carry dropout 0.1.  Weights and slots come from the seeded generator the tests share, so the file holds results
only, no reference code."""
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
    import phyre_readout_cases as cases
    base = os.path.join(args.reference, 'slotformer')
    nerv = [('nerv', {}), ('nerv.training', {'BaseModel': torch.nn.Module, 'BaseParams': object})]
    # slotformer.py imports the SAVi model for its decoder, which the position table does not touch: a stand-in
    savi = [('slotformer', {}), ('slotformer.base_slots', {}), ('slotformer.base_slots.models', {'StoSAVi': object})]
    vp = load_by_path('reference_slotformer', os.path.join(base, 'video_prediction', 'models', 'slotformer.py'), nerv + savi)
    for name, _ in savi:
        del sys.modules[name]
    nerv += [('nerv.models', {}), ('nerv.models.transformer', {'build_pos_enc': vp.build_pos_enc})]
    ref = load_by_path('reference_phyre_readout', os.path.join(base, 'phyre_planning', 'models', 'readout.py'), nerv)
    cfg = load_by_path('reference_phyre_readout_params', os.path.join(base, 'phyre_planning', 'configs', 'readout_phyre_params-fold0.py'),
                       nerv).SlotFormerParams
    rd, sd, slots, labels = cases.fixture_case()
    assert rd == dict(cfg.readout_dict), 'tests/phyre_readout_cases.py: READOUT_DICT differs from readout_phyre_params-fold0.py'
    model = ref.PHYREReadout(dict(cfg.readout_dict)).eval()
    own = model.state_dict()
    out = {'config': np.array(json.dumps(dict(model=cfg.model, readout_dict=cfg.readout_dict, n_sample_frames=cfg.n_sample_frames,
                                              video_len=cfg.video_len, lr=cfg.lr, max_epochs=cfg.max_epochs, optimizer=cfg.optimizer,
                                              train_batch_size=cfg.train_batch_size, val_batch_size=cfg.val_batch_size,
                                              warmup_steps_pct=cfg.warmup_steps_pct))),
           'state_dict_keys': np.array(json.dumps([[k, list(v.shape)] for k, v in own.items()])),
           'enc_t_pe': own['enc_t_pe'].numpy().copy()}
    model.load_state_dict({k: (own[k] if k == 'enc_t_pe' else sd[k]) for k in own})
    data = {'slots': torch.from_numpy(slots), 'label': torch.from_numpy(labels)}
    with torch.no_grad():
        res = model(data)
        ev = model.calc_eval_loss(data, res)
    out['logits'] = res['logits'].numpy()
    out['vqa_loss'] = np.float32(ev['vqa_loss'].item())
    out['acc_keys'] = np.array(json.dumps([k for k in ev if k.startswith('acc_')]))
    out['acc'] = np.array([float(v) for k, v in ev.items() if k.startswith('acc_')], np.float32)
    path = os.path.join(ROOT, 'tests', 'golden', 'phyre_readout.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    print('logits', out['logits'], 'acc', out['acc'])


if __name__ == '__main__':
    main()
