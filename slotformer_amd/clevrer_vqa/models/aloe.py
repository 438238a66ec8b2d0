"""CLEVRERAloe: the VQA model on pre-computed slots (reference: slotformer/clevrer_vqa/models/aloe.py) -- forward, the loss values and the
accuracy bookkeeping of calc_eval_loss, the latter two as one launch of the score kernel (csrc/aloe.hip)."""
import torch

from ...nerv_compat import BaseModel
from ... import ops
from .transformer import CLEVRERTransformerModel, remap_encoder_keys


class CLEVRERAloe(BaseModel):

    def __init__(self, transformer_model: CLEVRERTransformerModel):
        super().__init__()
        self.transformer_model = transformer_model

    def load_state_dict(self, state_dict, strict=True, **kw):
        tm = self.transformer_model
        return super().load_state_dict(remap_encoder_keys(state_dict, 'transformer_model.transformer_encoder.', tm.input_len, tm.d_model),
                                       strict=strict, **kw)

    def forward(self, data_dict):
        return self.transformer_model(data_dict)

    def calc_train_loss(self, data_dict, out_dict):
        """Values only, no graph attached: the differentiable loss is `train.aloe_loss` on the logits of `train.aloe_with_grad`."""
        loss_dict = self.transformer_model.loss_function(data_dict, out_dict)
        loss_dict['cls_bs'] = 0 if out_dict['cls_answer_logits'] is None else out_dict['cls_answer_logits'].shape[0]
        loss_dict['mc_bs'] = 0 if out_dict['mc_answer_logits'] is None else out_dict['mc_answer_logits'].shape[0]
        return loss_dict

    @torch.no_grad()
    def eval_counts(self, data_dict, out_dict, counts=None):
        """The ten int32 counts of calc_eval_loss on the device -- (right, questions) for ops.ALOE_COUNT_KEYS --, ADDED to `counts` when passed:
        a validation loop accumulates them over its batches and reads them once.  -> (counts, ques_correct [Q] or None)."""
        cls_logits, mc_logits = out_dict['cls_answer_logits'], out_dict['mc_answer_logits']
        if cls_logits is None and mc_logits is None:
            return (torch.zeros(10, dtype=torch.int32, device=self.device) if counts is None else counts), None
        _, ques, counts = ops.aloe_score(cls_logits, data_dict.get('cls_label'), mc_logits, data_dict.get('mc_label'), data_dict.get('mc_flag'),
                                         data_dict.get('mc_subtype'), counts=counts, device=self.device)
        return counts, (ques if mc_logits is not None else None)

    @torch.no_grad()
    def calc_eval_loss(self, data_dict, out_dict):
        """The reference's keys (aloe.py:46-92): `<kind>_acc` as 0-dim device tensors (0. for an empty kind), `<kind>_bs` as ints."""
        counts, _ = self.eval_counts(data_dict, out_dict)
        host = counts.cpu().tolist()
        ret = {}
        for i, key in enumerate(ops.ALOE_COUNT_KEYS):
            bs = host[2 * i + 1]
            ret[f'{key}_acc'] = counts[2 * i].float() / float(bs) if bs else torch.tensor(0.).to(self.device)
            ret[f'{key}_bs'] = bs
        return ret

    @property
    def dtype(self):
        return self.transformer_model.CLS.dtype

    @property
    def device(self):
        return self.transformer_model.CLS.device
