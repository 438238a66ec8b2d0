"""The Aloe reasoner over slots and question tokens on the MI355X engine (reference: slotformer/clevrer_vqa/models/transformer.py, the model of
Ding et al. 2020).

A CLS token, the slots of T frames (t-major, slot-minor) and the question (and choice) tokens form one sequence; every vision row is
vision_in_proj([slot | 0 1]), every text row q_in_proj([q_embedding[token] | type pair | 1 0]); a learnable position row is added to every row;
a pre-LN Transformer encoder runs with the padded text positions masked out as keys; an MLP on the CLS row gives the answer logits
(`cls_answer_mlp`: one per answer word; `mc_answer_mlp`: one logit per choice).  The module holds the parameters under the reference's names
and construction order; the forward is csrc/aloe.hip (`sf_aloe_fwd_f32`).  `forward` / `answer` are inference: training runs through `clevrer_vqa.fit` and
`train.aloe_with_grad` (csrc/aloe_train.hip).

The reference builds its encoder with nerv.models.transformer.build_transformer_encoder, a third-party function that is not part of the
reference tree.  From the call sites: it takes (x, src_key_padding_mask=), has a 'learnable' position encoding of input_len rows and is built
from d_model, heads, ffn_dim, layers, norm_first, norm_last=False.  ASSUMED here: the position table is added to every row, CLS included; the
layers are torch's nn.TransformerEncoderLayer (relu, eps 1e-5, batch_first); batch_cat_vec appends the id pair AFTER the features.  The wrapper's
parameter names are not knowable, so `AloeEncoder` names them plainly (`pos_enc`, `layers.i.*`) and `remap_encoder_keys` accepts a foreign
layout by suffix."""
import re

import torch
import torch.nn as nn

from ... import engine, ops

_NO_CPU = 'slotformer_amd: CLEVRERAloe runs on a HIP device only; there is no CPU fallback'
_NO_TRAIN = ('slotformer_amd: CLEVRERAloe is inference-only -- the backward of the Aloe reasoner (training, dropout, fit) is not built; '
             'call .eval() first')
LAYER_LEAVES = ('self_attn.in_proj_weight', 'self_attn.in_proj_bias', 'self_attn.out_proj.weight', 'self_attn.out_proj.bias', 'linear1.weight',
                'linear1.bias', 'linear2.weight', 'linear2.bias', 'norm1.weight', 'norm1.bias', 'norm2.weight', 'norm2.bias')
_LAYER_KEY = re.compile(r'(?:^|\.)layers\.(\d+)\.(' + '|'.join(re.escape(leaf) for leaf in LAYER_LEAVES) + r')$')


class AloeEncoder(nn.Module):
    """What build_transformer_encoder(pos_enc='learnable', norm_last=False) is assumed to be: a position table [1, input_len, d_model] added to
    every row, then the layers.  A parameter container: the layers run in csrc/aloe.hip."""

    def __init__(self, input_len, d_model, num_heads, ffn_dim, num_layers, norm_first=True):
        super().__init__()
        self.pos_enc = nn.Parameter(torch.zeros(1, input_len, d_model))
        nn.init.trunc_normal_(self.pos_enc, std=0.02)
        self.layers = nn.ModuleList([
            nn.TransformerEncoderLayer(d_model=d_model, nhead=num_heads, dim_feedforward=ffn_dim, norm_first=norm_first, batch_first=True)
            for _ in range(num_layers)])
        self.norm_first = norm_first


def build_transformer(input_len, pos_enc, d_model, num_heads, ffn_dim, num_layers, norm_first=True):
    """The reference's factory (transformer.py:9-32) on the assumed encoder."""
    if pos_enc != 'learnable':
        raise NotImplementedError(f"pos_enc={pos_enc!r}: only 'learnable' is supported (both reference configs)")
    return AloeEncoder(input_len, d_model, num_heads, ffn_dim, num_layers, norm_first=norm_first)


def remap_encoder_keys(state_dict, prefix, input_len, d_model):
    """A state dict whose encoder keys under `prefix` follow ANOTHER wrapper's layout -> one in this module's: every key ending in
    `layers.{i}.<leaf>` maps to layer i whatever stands between the prefix and `layers`; the one remaining tensor of input_len rows by d_model is
    the position table; anything else under the prefix is an error that lists the keys.  Keys outside the prefix pass through."""
    out, left = {}, []
    for key, val in state_dict.items():
        if not key.startswith(prefix):
            out[key] = val
            continue
        m = _LAYER_KEY.search(key[len(prefix):])
        if m:
            out[f'{prefix}layers.{m.group(1)}.{m.group(2)}'] = val
        else:
            left.append(key)
    tables = [k for k in left if torch.is_tensor(state_dict[k]) and state_dict[k].dim() >= 2 and
              tuple(state_dict[k].shape[-2:]) == (input_len, d_model) and state_dict[k].numel() == input_len * d_model]
    if len(tables) == 1:
        out[prefix + 'pos_enc'] = state_dict[tables[0]].reshape(1, input_len, d_model)
        left.remove(tables[0])
    if left:
        raise KeyError(f'slotformer_amd: encoder keys under {prefix!r} that are neither `layers.i.<leaf>` nor the one [{input_len}, {d_model}] '
                       f'position table: {sorted(left)}')
    return out


class CLEVRERTransformerModel(nn.Module):

    def __init__(self,
                 transformer_dict=dict(input_len=207, input_dim=16, pos_enc='learnable', num_layers=28, num_heads=10, ffn_dim=1024,
                                       norm_first=True, cls_mlp_size=128),
                 lang_dict=dict(question_len=20, question_vocab_size=82, answer_vocab_size=22),
                 vision_dict=dict(vision_dim=64),
                 loss_dict=dict(use_mask_obj_loss=False)):
        super().__init__()
        input_dim = transformer_dict['input_dim']
        lang_emb_dim = input_dim - 2
        self.input_dim = input_dim + 2
        # the id pairs concatenated to the text / vision features (fixed, from Aloe); question and choice need different ids
        self.text_token = nn.Parameter(torch.tensor([1, 0]).float(), requires_grad=False)
        self.vision_token = nn.Parameter(torch.tensor([0, 1]).float(), requires_grad=False)
        self.cls_token = nn.Parameter(torch.tensor([0, 1]).float(), requires_grad=False)
        self.mc_question_token = nn.Parameter(torch.tensor([1, 0]).float(), requires_grad=False)
        self.mc_choice_token = nn.Parameter(torch.tensor([0, 1]).float(), requires_grad=False)
        num_heads = transformer_dict['num_heads']
        self.d_model = self.input_dim * num_heads   # from Aloe
        self.input_len = transformer_dict['input_len'] + 1   # CLS token
        self.transformer_dict = transformer_dict
        self.transformer_encoder = build_transformer(self.input_len, transformer_dict['pos_enc'], self.d_model, num_heads,
                                                     transformer_dict['ffn_dim'], transformer_dict['num_layers'],
                                                     norm_first=transformer_dict['norm_first'])
        self.q_embedding = nn.Embedding(lang_dict['question_vocab_size'], lang_emb_dim)
        self.q_in_proj = nn.Linear(self.input_dim, self.d_model)
        self.question_len = lang_dict['question_len']
        self.num_answer_classes = lang_dict['answer_vocab_size']
        cls_mlp_size = transformer_dict['cls_mlp_size']
        self.cls_answer_mlp = nn.Sequential(nn.Linear(self.d_model, cls_mlp_size), nn.ReLU(), nn.Linear(cls_mlp_size, self.num_answer_classes))
        self.mc_answer_mlp = nn.Sequential(nn.Linear(self.d_model, cls_mlp_size), nn.ReLU(), nn.Linear(cls_mlp_size, 1))
        vision_dim = vision_dict['vision_dim'] + 2
        self.vision_in_proj = nn.Linear(vision_dim, self.d_model)
        self.CLS = nn.Parameter(torch.zeros(1, 1, self.d_model))   # from Aloe, zero-initialised
        self.mask_obj_loss = loss_dict['use_mask_obj_loss']
        if self.mask_obj_loss:   # (refused as the reference refuses it, transformer.py:136)
            raise AssertionError("don't use `mask_obj_loss` when using SAVi slots")

    def load_state_dict(self, state_dict, strict=True, **kw):
        return super().load_state_dict(remap_encoder_keys(state_dict, 'transformer_encoder.', self.input_len, self.d_model), strict=strict, **kw)

    def shape_ok(self, num_slots, T, text_len):
        td = self.transformer_dict
        return bool(td['norm_first']) and ops.aloe_ok(num_slots, self.vision_in_proj.in_features - 2, T, text_len, self.d_model, td['num_heads'],
                                                      td['ffn_dim'], td['num_layers'])

    @torch.no_grad()
    def answer(self, slots, tokens, pad_mask, multiple_choice, video_index=None, start=None, frame_offset=1, num_frames=None, want_answers=False):
        """The kernel call behind `forward`: slots [V, T_all, N, C] on the device, read in place -- batch entry b is video `video_index[b]`
        (default b) at frames `start[b] + t * frame_offset` for t < num_frames (default: T_all frames from 0; this is datasets/clevrer.py:
        _get_slots, the caller applies the predictive-question shift to `start`); tokens / pad_mask [B, text_len].  -> (logits [B, A] -- A = 1 for
        multiple choice --, answers [B] int32 or None: the argmax / logit > 0)."""
        if self.training:
            raise NotImplementedError(_NO_TRAIN)
        if not (torch.is_tensor(slots) and slots.is_cuda and self.CLS.is_cuda):
            raise RuntimeError(_NO_CPU)
        if slots.dim() != 4:
            raise ValueError(f'CLEVRERTransformerModel: slots are [V, T, N, C], got {tuple(slots.shape)}')
        N, T = slots.shape[2], slots.shape[1] if num_frames is None else int(num_frames)
        text_len = tokens.shape[-1]
        if 1 + T * N + text_len != self.input_len:
            raise ValueError(f'CLEVRERTransformerModel: 1 + {T} frames x {N} slots + {text_len} text positions = {1 + T * N + text_len} tokens, the '
                             f'position table holds input_len + 1 = {self.input_len}')
        if not self.shape_ok(N, T, text_len):
            td = self.transformer_dict
            raise NotImplementedError(f'CLEVRERTransformerModel(slots {N} x {slots.shape[3]}, {T} frames, {text_len} text positions, d_model='
                                      f'{self.d_model}, num_heads={td["num_heads"]}, ffn_dim={td["ffn_dim"]}, num_layers={td["num_layers"]}, '
                                      f'norm_first={td["norm_first"]}) has no kernel: {ops.ALOE_LIMITS}')
        plan = engine.aloe_plan(self)
        s = type(plan.struct).from_buffer_copy(plan.struct)
        s.num_slots, s.T, s.text_len = N, T, text_len
        mlp = self.mc_answer_mlp if multiple_choice else self.cls_answer_mlp
        return ops.aloe_fwd(s, slots, tokens, pad_mask, (mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias), multiple_choice,
                            video_index=video_index, start=start, frame_offset=frame_offset, want_answers=want_answers)

    def _kind(self, inputs, kind):
        """One question kind of a batch -> logits or None.  The slots are `<kind>_video_emb` [B, T, N, C] as the reference's collate stacks
        them, or -- read in place, no gathered copy -- `slots` [V, T_all, N, C] with `<kind>_video_index` [B], optional `<kind>_start` [B],
        `frame_offset` and `num_frames`.  Multiple choice: row i of the text belongs to question mc_flag[i]; the video of a choice is an INDEX
        composition (video_index[mc_flag]), never a gathered copy of slots."""
        tokens = inputs[f'{kind}_q_tokens']
        if len(tokens) == 0:
            return None
        mc = kind == 'mc'
        if 'slots' in inputs:
            slots, vidx, start = inputs['slots'], inputs[f'{kind}_video_index'], inputs.get(f'{kind}_start')
            offset, frames = inputs.get('frame_offset', 1), inputs.get('num_frames')
        else:
            slots, vidx, start, offset, frames = inputs[f'{kind}_video_emb'], None, None, 1, None
        if not (torch.is_tensor(slots) and slots.is_cuda and torch.is_tensor(tokens) and tokens.is_cuda):
            raise RuntimeError(_NO_CPU)
        if mc:
            flag = inputs['mc_flag'].long()
            vidx = flag if vidx is None else torch.as_tensor(vidx, device=flag.device)[flag]
            start = None if start is None else torch.as_tensor(start, device=flag.device)[flag]
        logits, _ = self.answer(slots, tokens, inputs[f'{kind}_q_pad_mask'], mc, video_index=vidx, start=start, frame_offset=offset,
                                num_frames=frames)
        return logits.view(-1) if mc else logits

    def forward(self, inputs):
        if self.training:
            raise NotImplementedError(_NO_TRAIN)
        return {'cls_answer_logits': self._kind(inputs, 'cls'), 'mc_answer_logits': self._kind(inputs, 'mc'), 'gt_v_emb': None, 'pred_v_emb': None}

    @torch.no_grad()
    def loss_function(self, data_dict, out_dict):
        """The two loss VALUES (transformer.py:326-361) from one launch of the score kernel; no graph is attached."""
        cls_logits, mc_logits = out_dict['cls_answer_logits'], out_dict['mc_answer_logits']
        if cls_logits is None and mc_logits is None:
            zero = torch.tensor(0.).type_as(self.CLS)
            return {'cls_answer_loss': zero, 'mc_answer_loss': zero.clone()}
        losses, _, _ = ops.aloe_score(cls_logits, data_dict.get('cls_label'), mc_logits, data_dict.get('mc_label'), data_dict.get('mc_flag'),
                                      data_dict.get('mc_subtype'), device=self.CLS.device)
        return {'cls_answer_loss': losses[0], 'mc_answer_loss': losses[1]}
