"""Transformer readout for the PHYRE task-success classifier on the MI355X engine (reference: slotformer/phyre_planning/models/readout.py).

"Will the green ball touch the blue object?": the slots of a few selected timesteps are projected to d_model, get a temporal position row, a CLS
token is put in front, a pre-LN Transformer encoder reasons over the 1 + T x N tokens, and an MLP on the CLS row gives one logit.  The module
holds the parameters under the reference's state-dict names (`CLS`, `in_proj.*`, `transformer_encoder.layers.i.*`, `enc_t_pe`, `cls_mlp.0.*`,
`cls_mlp.2.*`); the forward is three launches of csrc/phyre_readout.hip and csrc/layer_tok128.hip (`sf_phyre_readout_fwd_f32`): the token rows
straight from the slots tensor (no gathered copy), all layers at once, the head.

Training runs through `phyre_planning.fit` / `train.phyre_readout_with_grad` (csrc/phyre_readout_train.hip: one launch per layer in each
direction); a differentiable `Module.forward` is not built, and `forward` says so when the module is in training mode."""
import numpy as np
import torch
import torch.nn as nn

from ...nerv_compat import BaseModel
from ...video_prediction.models.slotformer import build_pos_enc
from ... import engine, ops

ACC_THRESHS = tuple(np.arange(0.1, 1, 0.2))   # readout.py:103
READOUT_DEFAULTS = dict(num_slots=8, slot_size=128, t_pe='sin', d_model=128, num_layers=4, num_heads=8, ffn_dim=512, norm_first=True,
                        sel_slots=[0, 3])
_NO_CPU = 'slotformer_amd: PHYREReadout runs on a HIP device only; there is no CPU fallback'


class PHYREReadout(BaseModel):

    def __init__(self, readout_dict=None):
        super().__init__()
        self.readout_dict = dict(READOUT_DEFAULTS) if readout_dict is None else readout_dict
        rd = self.readout_dict
        self.num_slots = rd['num_slots']
        self.slot_size = rd['slot_size']
        self.sel_slots = rd['sel_slots']   # reason over the slots at these timesteps
        self.T = len(self.sel_slots)
        d_model = rd['d_model']
        # the reference's construction order (readout.py:46-67), which fixes the state-dict order: the module's own parameters (CLS, enc_t_pe)
        # come first, then in_proj, transformer_encoder and cls_mlp
        self.in_proj = nn.Linear(self.slot_size, d_model)
        self.CLS = nn.Parameter(torch.zeros(1, 1, d_model))
        layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=rd['num_heads'], dim_feedforward=rd['ffn_dim'], norm_first=rd['norm_first'],
                                           batch_first=True)
        self.transformer_encoder = nn.TransformerEncoder(encoder_layer=layer, num_layers=rd['num_layers'], enable_nested_tensor=False)
        self.enc_t_pe = build_pos_enc(rd['t_pe'], self.T, d_model)
        self.cls_mlp = nn.Sequential(nn.Linear(d_model, d_model), nn.ReLU(), nn.Linear(d_model, 1))

    def shape_ok(self):
        rd = self.readout_dict
        return bool(rd['norm_first']) and self.enc_t_pe is not None and ops.phyre_readout_ok(
            self.num_slots, self.slot_size, self.T, rd['d_model'], rd['num_heads'], rd['ffn_dim'], rd['num_layers'])

    def _check(self, slots):
        """An uncovered readout_dict constructs (its checkpoints load); it is refused at first use."""
        if self.training:
            raise NotImplementedError('slotformer_amd: the training kernels of this readout run through phyre_planning.fit / '
                                      'train.phyre_readout_with_grad; a differentiable Module.forward is not built -- call .eval() first')
        if not self.shape_ok():
            rd = self.readout_dict
            raise NotImplementedError(f'PHYREReadout(num_slots={self.num_slots}, slot_size={self.slot_size}, sel_slots={list(self.sel_slots)}, '
                                      f'd_model={rd["d_model"]}, num_heads={rd["num_heads"]}, ffn_dim={rd["ffn_dim"]}, num_layers={rd["num_layers"]}, '
                                      f'norm_first={rd["norm_first"]}, t_pe={rd["t_pe"]!r}) has no kernel: {ops.PHYRE_LIMITS}')
        if not (torch.is_tensor(slots) and slots.is_cuda and self.CLS.is_cuda):
            raise RuntimeError(_NO_CPU)
        if slots.dim() != 4 or tuple(slots.shape[2:]) != (self.num_slots, self.slot_size):
            raise ValueError(f'PHYREReadout: slots are [B, T, {self.num_slots}, {self.slot_size}], got {tuple(slots.shape)}')

    @torch.no_grad()
    def logits_of(self, slots, sel=None, video_index=None, want_conf=False, scatter_index=None, scatter_table=None):
        """The kernel call behind `forward`: `sel` replaces `self.sel_slots` as the frame of every token group (-1: a frame of zeros; the
        position row stays the place in the table); video_index / scatter_*: see ops.phyre_readout_fwd.  -> (logits [B], conf [B] or None)."""
        self._check(slots)
        sel = list(self.sel_slots) if sel is None else [int(s) for s in sel]
        if len(sel) != self.T:
            raise ValueError(f'PHYREReadout: the frame table holds {self.T} entries (len(sel_slots)), got {len(sel)}')
        if any(s < -1 or s >= slots.shape[1] for s in sel):
            raise IndexError(f'PHYREReadout: frame table {sel} on slots of {slots.shape[1]} frames (entries are -1 or a frame number)')
        plan = engine.phyre_readout_plan(self)
        rd = self.readout_dict
        return ops.phyre_readout_fwd(slots, sel, self.in_proj.weight, self.in_proj.bias, self.enc_t_pe, self.CLS, plan.layers, rd['num_layers'],
                                     self.cls_mlp[0].weight, self.cls_mlp[0].bias, self.cls_mlp[2].weight, self.cls_mlp[2].bias,
                                     video_index=video_index, want_conf=want_conf, scatter_index=scatter_index, scatter_table=scatter_table,
                                     d_model=rd['d_model'], num_heads=rd['num_heads'], ffn=rd['ffn_dim'])

    def forward(self, data_dict):
        """data_dict['slots'] [B,T_all,N,C] -> {'logits': [B]} from the frames `sel_slots`.  Optional key 'video_index' [B]: picks the batch out of
        a larger slots tensor without a gather copy."""
        return {'logits': self.logits_of(data_dict['slots'], video_index=data_dict.get('video_index'))[0]}

    def calc_train_loss(self, data_dict, out_dict):
        pred = out_dict['logits'].flatten()
        if not pred.is_cuda:
            raise RuntimeError(_NO_CPU)
        loss, _, _, _ = ops.physion_readout_score(pred, data_dict['label'].flatten(), want_grad=False)
        return {'vqa_loss': loss[0]}

    @torch.no_grad()
    def calc_eval_loss(self, data_dict, out_dict):
        """+ acc_0.10 .. acc_0.90 (readout.py:98-109): loss and the five counts in one launch."""
        pred = out_dict['logits'].flatten()
        if not pred.is_cuda:
            raise RuntimeError(_NO_CPU)
        loss, _, counts, _ = ops.physion_readout_score(pred, data_dict['label'].flatten(), threshs=ACC_THRESHS, want_grad=False)
        ret_dict = {'vqa_loss': loss[0]}
        acc = counts[0].float() / pred.numel()
        for i, thresh in enumerate(ACC_THRESHS):
            ret_dict[f'acc_{thresh:.2f}'] = acc[i]
        return ret_dict

    @property
    def dtype(self):
        return self.CLS.dtype

    @property
    def device(self):
        return self.CLS.device
