#!/usr/bin/env python
"""Write tests/golden/clevrer_aloe_grads.npz: the REFERENCE's own CLEVRERAloe (slotformer/clevrer_vqa/models/aloe.py, transformer.py) in eval() on
the seeded weights and the mixed batch of tests/aloe_fit_cases.py (`fixture_train_case`: 2 layers, d 72 = 4 x 18, ffn 64, 3 videos of 3 frames,
4 slots of 32, 12 text positions; 3 descriptive questions and 2 multiple-choice ones with 2 + 1 choices) -- both logits, both losses of
calc_train_loss, and every parameter gradient of (cls_answer_loss + mc_answer_loss).backward().

    python tools/gen_golden_clevrer_vqa_grads.py --reference PATH_TO_THE_REFERENCE_TREE

The reference's classes are loaded by path over the stand-ins of tools/gen_golden_clevrer_vqa.py (see there for what is assumed about the
third-party encoder).  The file holds results and names only."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('SLOTFORMER_REFERENCE'), required='SLOTFORMER_REFERENCE' not in os.environ)
    args = ap.parse_args()
    import aloe_fit_cases as fit_cases
    from gen_golden_clevrer_vqa import stand_ins, load_models
    stand_ins()
    ref_tm, ref_aloe = load_models(os.path.join(args.reference, 'slotformer', 'clevrer_vqa', 'models'))
    tc = fit_cases.fixture_train_case()
    td, ld, vd, lossd = tc['cfg']
    tm = ref_tm.CLEVRERTransformerModel(transformer_dict=dict(td), lang_dict=dict(ld), vision_dict=dict(vd), loss_dict=dict(lossd))
    model = ref_aloe.CLEVRERAloe(tm).eval()
    own = model.state_dict()
    short = {k: k[len('transformer_model.'):].replace('transformer_encoder.encoder.layers.', 'transformer_encoder.layers.') for k in own}
    model.load_state_dict({k: tc['sd'][short[k]] for k in own})

    slots = torch.from_numpy(tc['slots'])
    B1 = tc['B1']
    vidx = torch.as_tensor(tc['video_index'][:B1])
    data = {'cls_video_emb': slots[vidx], 'cls_q_tokens': torch.from_numpy(tc['tokens'][:B1]), 'cls_q_pad_mask': torch.from_numpy(tc['pad'][:B1]),
            'cls_label': torch.from_numpy(tc['cls_label']), 'mc_video_emb': slots[torch.from_numpy(tc['mc_video'])],
            'mc_q_tokens': torch.from_numpy(tc['tokens'][B1:]), 'mc_q_pad_mask': torch.from_numpy(tc['pad'][B1:]),
            'mc_label': torch.from_numpy(tc['mc_label']), 'mc_flag': torch.from_numpy(tc['mc_flag'])}
    res = model(data)
    loss = model.calc_train_loss(data, res)
    (loss['cls_answer_loss'] + loss['mc_answer_loss']).backward()
    grads = {short[k]: p.grad for k, p in model.named_parameters() if p.requires_grad}
    keys = fit_cases.grad_keys(tc['cfg'])
    assert sorted(keys) == sorted(grads), set(keys) ^ set(grads)
    out = {'keys': np.array(json.dumps(keys)), 'cls_loss': np.float32(loss['cls_answer_loss'].item()), 'mc_loss': np.float32(loss['mc_answer_loss'].item()),
           'cls_logits': res['cls_answer_logits'].detach().numpy(), 'mc_logits': res['mc_answer_logits'].detach().numpy()}
    for k in keys:
        out['grad.' + k] = grads[k].numpy().astype(np.float32)
    np.savez_compressed(fit_cases.GOLDEN, **out)
    print(fit_cases.GOLDEN, os.path.getsize(fit_cases.GOLDEN), 'bytes')
    ref = fit_cases.loss_and_grads64(tc)
    print('float64 restatement vs the reference float32: losses', ref['losses'], (float(out['cls_loss']), float(out['mc_loss'])), 'worst gradient rel',
          max(fit_cases.rel_err(ref['grads'][k], out['grad.' + k]) for k in keys))


if __name__ == '__main__':
    main()
