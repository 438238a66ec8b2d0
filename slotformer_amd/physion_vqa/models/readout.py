"""Linear readout for the Physion VQA task on the MI355X engine (reference: slotformer/physion_vqa/models/readout.py).

"Do the two objects touch?": a linear relation over every pair of slots of a timestep, aggregated over the pairs by max / sum / mean, a linear
logit per timestep, and the maximum over time.  The module holds the parameters under the reference's state-dict names (`comb_idx`,
`linear1.*`, `linear2.*`); forward, loss, accuracy and backward run on the kernels of csrc/physion_readout.hip (`sf_physion_readout_*`), which
never build the gathered [B, T, pairs, 2C] tensor: linear1 of a pair is one product per slot and an add."""
from itertools import combinations

import numpy as np
import torch
import torch.nn as nn

from ...nerv_compat import BaseModel
from ... import ops, train

ACC_THRESHS = tuple(np.arange(0.1, 1, 0.2))   # readout.py:95


class PhysionReadout(BaseModel):

    def __init__(self, readout_dict=dict(num_slots=6, slot_size=192, agg_func='max', feats_dim=192)):
        super().__init__()
        self.readout_dict = readout_dict
        self.num_slots = readout_dict['num_slots']
        self.slot_size = readout_dict['slot_size']
        self.agg_func = readout_dict['agg_func']
        assert self.agg_func in ['sum', 'mean', 'max']
        self.feats_dim = readout_dict['feats_dim']
        combs = list(combinations(list(range(self.num_slots)), 2))
        self.register_buffer('comb_idx', torch.tensor(combs).long().flatten())   # [pairs * 2]; the kernels walk the same order
        self.linear1 = nn.Linear(self.slot_size * 2, self.feats_dim)   # relation
        self.linear2 = nn.Linear(self.feats_dim, 1)   # logits

    def _check(self, slots):
        """An unsupported readout_dict constructs (its checkpoints load); it is refused at first use."""
        if not ops.physion_readout_ok(self.num_slots, self.slot_size, self.feats_dim):
            raise NotImplementedError(f'PhysionReadout(num_slots={self.num_slots}, slot_size={self.slot_size}, feats_dim={self.feats_dim}) has no '
                                      f'kernel: {ops.READOUT_LIMITS}')
        if not (torch.is_tensor(slots) and slots.is_cuda and self.linear1.weight.is_cuda):
            raise RuntimeError('slotformer_amd: PhysionReadout runs on a HIP device only; there is no CPU fallback')
        if slots.dim() != 4 or tuple(slots.shape[2:]) != (self.num_slots, self.slot_size):
            raise ValueError(f'PhysionReadout: slots are [B, T, {self.num_slots}, {self.slot_size}], got {tuple(slots.shape)}')

    def forward(self, data_dict, return_steps=False):
        """data_dict['slots'] [B,T,N,C] -> {'logits': [B]} (return_steps: also 'step_logits' [B,T]).  Optional keys: 'video_index' [B] picks the
        batch out of a larger slots tensor without a gather copy, 'video_len' reads only the first frames."""
        slots = data_dict['slots']
        self._check(slots)
        out = train.readout_with_grad(self, slots, video_index=data_dict.get('video_index'), video_len=data_dict.get('video_len'),
                                      return_steps=return_steps)
        return {'logits': out[0], 'step_logits': out[1]} if return_steps else {'logits': out}

    def calc_train_loss(self, data_dict, out_dict):
        pred = out_dict['logits'].flatten()
        if not pred.is_cuda:
            raise RuntimeError('slotformer_amd: PhysionReadout runs on a HIP device only; there is no CPU fallback')
        return {'vqa_loss': train.readout_loss(pred, data_dict['label'].flatten())}

    @torch.no_grad()
    def calc_eval_loss(self, data_dict, out_dict):
        """+ acc_0.10 .. acc_0.90 (readout.py:89-101): loss and the five counts in one launch."""
        pred = out_dict['logits'].flatten()
        if not pred.is_cuda:
            raise RuntimeError('slotformer_amd: PhysionReadout runs on a HIP device only; there is no CPU fallback')
        loss, _, counts, _ = ops.physion_readout_score(pred, data_dict['label'].flatten(), threshs=ACC_THRESHS, want_grad=False)
        ret_dict = {'vqa_loss': loss[0]}
        acc = counts[0].float() / pred.numel()
        for i, thresh in enumerate(ACC_THRESHS):
            ret_dict[f'acc_{thresh:.2f}'] = acc[i]
        return ret_dict

    @property
    def dtype(self):
        return self.linear1.weight.dtype

    @property
    def device(self):
        return self.linear1.weight.device
