"""Shared by test_slotformer_fit.py (CPU) and test_slotformer_fit_gpu.py: the small SlotFormer the tests train, its slot table, and the float64
restatement of the rollout loss (slotformer.py:289-318)."""
import torch

ROLL = dict(num_slots=3, slot_size=64, history_len=2, t_pe='sin', slots_pe='', d_model=64, num_layers=2, num_heads=2, ffn_dim=64, norm_first=True)
HIST, S, V, T, N, C = 2, 3, 4, 12, 3, 64
RES = 8   # decoder: a 2x2 broadcast grid, two stride-2 layers -> 8x8


def decoder_checkpoint(path, slot_size=C, res=RES):
    """A checkpoint file holding a seeded `decoder.*` / `decoder_pos_embedding.*`, as SlotFormer borrows it from a SAVi run."""
    from slotformer_amd.host import containers
    from slotformer_amd.base_slots.models.utils import SoftPositionEmbed
    torch.manual_seed(11)
    dec, reached = containers.deconv_stack((slot_size, 64, 64), 5, '', 2, res)
    assert reached == res
    pos = SoftPositionEmbed(slot_size, (2, 2))
    sd = {'decoder.' + k: v for k, v in dec.state_dict().items()}
    sd.update({'decoder_pos_embedding.' + k: v for k, v in pos.state_dict().items()})
    torch.save({'state_dict': sd}, path)
    return path


def build_model(ckpt, seed=3, img=False, single_step=False, rollout_len=S):
    from slotformer_amd.video_prediction.models import SlotFormer, SingleStepSlotFormer
    torch.manual_seed(seed)
    dec = dict(dec_channels=(C, 64, 64), dec_resolution=(2, 2), dec_ks=5, dec_norm='', dec_ckp_path=ckpt)
    roll = dict(ROLL)
    cls = SlotFormer
    if single_step:
        roll.update(history_len=1, cond_len=2)
        cls = SingleStepSlotFormer
    return cls((RES, RES), roll['history_len'] + rollout_len, slot_dict=dict(num_slots=N, slot_size=C), dec_dict=dec, rollout_dict=roll,
               loss_dict=dict(rollout_len=rollout_len, use_img_recon_loss=img))


def no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.


def seeded_table(seed=5, v=V, t=T, n=N, c=C):
    return torch.randn(v, t, n, c, generator=torch.Generator().manual_seed(seed))


def gather_clips(table, clips, n_frames, f):
    """[M, n_frames, ...]: the reference's sampler (datasets/clevrer.py:323-335) on a table."""
    return torch.stack([torch.stack([table[int(v), int(s) + j * f] for j in range(n_frames)]) for v, s in clips.tolist()])


def mse_reference(pred, target, hist, w=None, clip_len=None, scale=1.):
    """slotformer.py:289-318 in float64 on dense pred / target [B, S, ...] -> (loss, d_pred, per-step sums, per-step counts, count)."""
    p, t = pred.double().flatten(2), target.double().flatten(2)
    B, S_, E = p.shape
    w = torch.ones(S_, dtype=torch.float64) if w is None else w.double()
    keep = torch.ones(B, S_, dtype=torch.bool)
    if clip_len is not None:
        keep = (torch.arange(S_)[None] + hist) < clip_len.long()[:, None]
    diff = (p - t) * keep[:, :, None]
    count = float(keep.sum()) * E
    sq = diff**2
    loss = scale * float((sq * w[None, :, None]).sum()) / count if count else 0.
    d = scale * w[None, :, None] * 2 * diff / count if count else torch.zeros_like(diff)
    return loss, d.reshape(pred.shape), sq.sum((0, 2)), keep.sum(0).double() * E, count
