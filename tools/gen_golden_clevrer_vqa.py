#!/usr/bin/env python
"""Write tests/golden/clevrer_aloe.npz, tests/golden/clevrer_vocab.json and tests/golden/clevrer_vqa_params.json: the REFERENCE's own
CLEVRERAloe (slotformer/clevrer_vqa/models/aloe.py, transformer.py) with the settings of aloe_clevrer_params-rollout.py on the seeded weights
and inputs of tests/clevrer_vqa_cases.py (`fixture_case`: 3 videos of 25 frames, 7 slots of 128, 32 text positions) -- the logits of both
question kinds, both losses, the keys and values of calc_eval_loss, the state-dict keys and shapes of the parameters the reference owns itself,
and the config as plain data.

    python tools/gen_golden_clevrer_vqa.py --reference PATH_TO_THE_REFERENCE_TREE

The reference's transformer.py and aloe.py are loaded by path.  Their outside imports are replaced by stand-ins of our own, because the nerv
package is third-party and not part of the reference tree:

  * nerv.training.BaseModel                             a plain nn.Module
  * nerv.utils.batch_cat_vec(x, vec, dim=-1)            widens the last dim by len(vec).  ASSUMED: the values are appended AFTER the features
  * nerv.utils.batch_gather                             only reached with use_mask_obj_loss, which the model refuses: a stub that raises
  * nerv.models.transformer.build_transformer_encoder   inferable from the call sites: it takes (x, src_key_padding_mask=), has a 'learnable'
    position encoding of input_len rows, is built from d_model, heads, ffn_dim, layers, norm_first and norm_last=False.  ASSUMED: the position
    table is added to every row, CLS included, and the layers are torch's nn.TransformerEncoderLayer (relu, eps 1e-5, batch_first)

NOT knowable here: the parameter names of nerv's encoder wrapper.  The golden file therefore records the state-dict keys of the reference-owned
parameters only, and this repository's load_state_dict accepts a foreign encoder layout by suffix (clevrer_vqa/models/transformer.py:
remap_encoder_keys).  The model runs in .eval(): its encoder layers carry dropout 0.1.  Weights and inputs come from the seeded generator the
tests share, so the files hold results, a list of names and settings only, no reference code."""
import argparse
import ast
import importlib.util
import json
import os
import shutil
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
CONFIGS = ('aloe_clevrer_params.py', 'aloe_clevrer_params-rollout.py')


class StandInEncoder(nn.Module):
    """Our reading of build_transformer_encoder(pos_enc='learnable', norm_last=False)."""

    def __init__(self, input_len, d_model, num_heads, ffn_dim, num_layers, norm_first):
        super().__init__()
        self.pos_enc = nn.Parameter(torch.zeros(1, input_len, d_model))
        layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=num_heads, dim_feedforward=ffn_dim, norm_first=norm_first, batch_first=True)
        self.encoder = nn.TransformerEncoder(encoder_layer=layer, num_layers=num_layers, enable_nested_tensor=False)

    def forward(self, x, src_key_padding_mask=None):
        return self.encoder(x + self.pos_enc, src_key_padding_mask=src_key_padding_mask)


def build_transformer_encoder(input_len, pos_enc, d_model, num_heads, ffn_dim, num_layers, norm_first=True, norm_last=False):
    assert pos_enc == 'learnable' and not norm_last
    return StandInEncoder(input_len, d_model, num_heads, ffn_dim, num_layers, norm_first)


def batch_cat_vec(x, vec, dim=-1):
    assert dim == -1
    return torch.cat([x, vec.expand(*x.shape[:-1], vec.shape[0]).to(x.dtype)], dim=-1)


def batch_gather(*a, **k):
    raise NotImplementedError('batch_gather is only reached with use_mask_obj_loss')


def stand_ins():
    table = [('nerv', {}), ('nerv.training', {'BaseModel': nn.Module, 'BaseParams': object}),
             ('nerv.utils', {'batch_cat_vec': batch_cat_vec, 'batch_gather': batch_gather}), ('nerv.models', {}),
             ('nerv.models.transformer', {'build_transformer_encoder': build_transformer_encoder})]
    for mod_name, attrs in table:
        m = types.ModuleType(mod_name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[mod_name] = m


def load_models(models_dir):
    """transformer.py and aloe.py as submodules of a made-up package, so that aloe.py's relative import resolves"""
    pkg = types.ModuleType('reference_clevrer_models')
    pkg.__path__ = [models_dir]
    sys.modules[pkg.__name__] = pkg
    out = []
    for name in ('transformer', 'aloe'):
        full = f'{pkg.__name__}.{name}'
        spec = importlib.util.spec_from_file_location(full, os.path.join(models_dir, name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
        out.append(mod)
    return out


def config_settings(path):
    """The class attributes of a config file's SlotFormerParams as plain data (the file is executed with the stand-in BaseParams); the two
    attributes that hold paths of the machine the file lies on are replaced: `cur_dir` is dropped, `vocab_file` becomes its file name."""
    spec = importlib.util.spec_from_file_location('reference_aloe_params', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.SlotFormerParams
    with open(path) as f:
        tree = ast.parse(f.read())
    imports = [f'{n.module}.{a.name}' for n in tree.body if isinstance(n, ast.ImportFrom) for a in n.names]
    attrs = {k: getattr(p, k) for k in dir(p) if not k.startswith('_') and not callable(getattr(p, k)) and k != 'cur_dir'}
    attrs['vocab_file'] = os.path.basename(attrs['vocab_file'])
    return {'imports': imports, 'attrs': attrs}, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('SLOTFORMER_REFERENCE'), required='SLOTFORMER_REFERENCE' not in os.environ)
    args = ap.parse_args()
    import clevrer_vqa_cases as cases
    base = os.path.join(args.reference, 'slotformer', 'clevrer_vqa')
    golden = os.path.join(ROOT, 'tests', 'golden')
    stand_ins()
    ref_tm, ref_aloe = load_models(os.path.join(base, 'models'))

    files = {}
    for name in CONFIGS:
        files[f'clevrer_vqa/configs/{name}'], params = config_settings(os.path.join(base, 'configs', name))
    with open(os.path.join(golden, 'clevrer_vqa_params.json'), 'w') as f:
        json.dump({'files': files}, f, indent=1, sort_keys=True)
        f.write('\n')
    shutil.copyfile(os.path.join(base, 'datasets', 'cache', 'CLEVRER_vocab.json'), os.path.join(golden, 'clevrer_vocab.json'))
    with open(os.path.join(golden, 'clevrer_vocab.json')) as f:
        vocab = json.load(f)

    fc = cases.fixture_case()
    td, ld, vd, lossd = fc['cfg']
    assert td == dict(params.transformer_dict) and vd == dict(params.vision_dict) and lossd == dict(params.loss_dict), \
        'tests/clevrer_vqa_cases.py: the config differs from aloe_clevrer_params-rollout.py'
    assert ld == dict(question_vocab_size=len(vocab['q_vocab']), answer_vocab_size=len(vocab['a_vocab']), question_len=params.max_question_len)
    tm = ref_tm.CLEVRERTransformerModel(transformer_dict=dict(td), lang_dict=dict(ld), vision_dict=dict(vd), loss_dict=dict(lossd))
    model = ref_aloe.CLEVRERAloe(tm).eval()
    own = model.state_dict()
    owned = [[k, list(v.shape)] for k, v in own.items() if not k.startswith('transformer_model.transformer_encoder.')]
    sd = {}
    for k in own:
        short = k[len('transformer_model.'):]
        sd[k] = fc['sd'][short.replace('transformer_encoder.encoder.layers.', 'transformer_encoder.layers.')]
    model.load_state_dict(sd)

    slots = torch.from_numpy(fc['slots'])
    data = {'cls_video_emb': slots, 'cls_q_tokens': torch.from_numpy(fc['cls_tokens']), 'cls_q_pad_mask': torch.from_numpy(fc['cls_pad']),
            'cls_label': torch.from_numpy(fc['cls_label']), 'mc_video_emb': slots[torch.from_numpy(fc['mc_video'])],
            'mc_q_tokens': torch.from_numpy(fc['mc_tokens']), 'mc_q_pad_mask': torch.from_numpy(fc['mc_pad']),
            'mc_label': torch.from_numpy(fc['mc_label']), 'mc_flag': torch.from_numpy(fc['mc_flag']), 'mc_subtype': torch.from_numpy(fc['mc_subtype'])}
    with torch.no_grad():
        res = model(data)
        train = model.calc_train_loss(data, res)
        ev = model.calc_eval_loss(data, res)
    out = {'config': np.array(json.dumps(dict(model=params.model, transformer_dict=td, lang_dict=ld, vision_dict=vd, loss_dict=lossd,
                                              n_sample_frames=params.n_sample_frames, max_n_objects=params.max_n_objects,
                                              max_question_len=params.max_question_len, max_choice_len=params.max_choice_len,
                                              val_batch_size=params.val_batch_size))),
           'state_dict_keys': np.array(json.dumps(owned)),
           'cls_logits': res['cls_answer_logits'].numpy(), 'mc_logits': res['mc_answer_logits'].numpy(),
           'cls_answer_loss': np.float32(train['cls_answer_loss'].item()), 'mc_answer_loss': np.float32(train['mc_answer_loss'].item()),
           'train_bs': np.array([train['cls_bs'], train['mc_bs']]),
           'eval_keys': np.array(json.dumps(list(ev))), 'eval_values': np.array([float(v) for v in ev.values()], np.float64)}
    path = os.path.join(golden, 'clevrer_aloe.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    for mc, key in ((False, 'cls_logits'), (True, 'mc_logits')):
        tok, pad = (fc['mc_tokens'], fc['mc_pad']) if mc else (fc['cls_tokens'], fc['cls_pad'])
        ref64 = cases.forward64(fc['sd'], fc['cfg'], fc['slots'], tok, pad, mc, video_index=fc['mc_video'][fc['mc_flag']] if mc else None)
        print(key, 'float64 restatement vs the reference float32: rel', float(np.abs(ref64 - out[key]).max() / np.abs(ref64).max()),
              'clearance (margin, bar)', cases.clearance(ref64, mc))
    print('eval', dict(zip(ev, out['eval_values'])), 'losses', out['cls_answer_loss'], out['mc_answer_loss'])


if __name__ == '__main__':
    main()
