"""slotformer.base_slots counterpart: exports build_model, and the loop that trains the three base models -- StoSAVi / SAVi, STEVE and the dVAE --
on frames that live on the device: `fit` (the reference's nerv runs of SAViMethod, STEVEMethod and dVAEMethod: Adam, warm-up + cosine, gradient
clipping, STEVE's two rates, the dVAE's temperature anneal) and `evaluate`, around `clip_index`, `clip_schedule` and `cosine_anneal`.  The uint8
frames of a dataset fit the HBM of one MI355X (CLEVRER at 64 x 64 x 128 frames: 1.5 MB a video), so a batch is a list of (video, start) pairs
gathered and normalised by one launch, and every random draw of step s -- kernel noise, Gumbel noise, dropout masks -- is a function of (seed, s)."""
import math

import torch

from .._call import require_device
from .models import build_model
from .models.dVAE import dVAE
from .models.steve import STEVE

LOSS_W = {'savi': (1., 1e-4), 'steve': (1., 1.), 'dvae': (1., )}   # the reference configurations' weights
TERMS = {'savi': ('post_recon_loss', 'kld_loss'), 'steve': ('token_recon_loss', 'img_recon_loss'), 'dvae': ('recon_loss', )}


def __getattr__(name):
    """`clip_index` and `clip_schedule` of video_prediction, re-exported: Physion's and CLEVRER's datasets sample the clips of the base models by
    exactly those rules (filter_enter=False).  Looked up on first use, because video_prediction's models import this package's."""
    if name in ('clip_index', 'clip_schedule'):
        from .. import video_prediction
        return getattr(video_prediction, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def build_dataset(params, *a, **k):
    raise NotImplementedError('datasets are host-side I/O outside the hot path (SURVEY.md 2.1 row 13)')


def build_method(*a, **k):
    raise NotImplementedError('the nerv trainer is outside the hot path (SURVEY.md 2.1 row 12)')


def cosine_anneal(step, start_value, final_value, final_step, start_step=0):
    """The dVAE's temperature schedule: start_value up to start_step, final_value from final_step on, and between them half a cosine,
    0.5 (a - b) cos(pi * progress) + 0.5 (a + b) with progress = (step - start_step) / (final_step - start_step)."""
    if step < start_step:
        return float(start_value)
    if step >= final_step:
        return float(final_value)
    progress = (step - start_step) / (final_step - start_step)
    return 0.5 * (start_value - final_value) * math.cos(math.pi * progress) + 0.5 * (start_value + final_value)


def _kind(model):
    return 'dvae' if isinstance(model, dVAE) else 'steve' if isinstance(model, STEVE) else 'savi'


def _check_frames(frames, model, who):
    """The shape of the frame table: contiguous uint8 [V, T, H, W, 3] at the model's resolution (a dVAE: any multiple of 4).  That it lives on the
    device is checked last, so that every other refusal shows on host tensors too."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError(f'slotformer_amd.base_slots.{who}: frames are a contiguous uint8 [V, T, H, W, 3] table, got '
                         f'{getattr(frames, "dtype", type(frames).__name__)} {tuple(getattr(frames, "shape", ()))}')
    res = getattr(model, 'resolution', None)
    H, W = frames.shape[2:4]
    if (res is not None and (H, W) != tuple(res)) or (res is None and (H % 4 or W % 4)):
        want = f'{res[0]}, {res[1]}' if res is not None else 'H, W (multiples of 4)'
        raise ValueError(f'slotformer_amd.base_slots.{who}: frames are uint8 [V, T, {want}, 3] at the model\'s resolution, got {tuple(frames.shape)}')


def _steve_ids(model, tokens, img, cv, cs, T, frame_offset):
    """The token targets of a batch [B, T, h*w]: picked from the table, or tokenised on the fly from the gathered frames."""
    if tokens is None:
        return model.dvae.tokenize_ids(img).flatten(2, 3)
    t = cs.long()[:, None] + torch.arange(T, device=cs.device) * frame_offset
    return tokens[cv.long()[:, None], t]


def _train_terms(kind, model, img, ids, sd, tau):
    """One training forward on the gathered batch img [B, T, 3, H, W] -> [(differentiable term, its value as a float64 device scalar), ...] in
    TERMS order.  The image terms are `train.clip_mse` in its dense form."""
    from .. import train
    B, T = img.shape[:2]
    if kind == 'savi':
        out = model({'img': img, 'noise_seed': sd})
        mse, st = train.clip_mse(out['post_recon_combined'].reshape(B, T, -1), img.reshape(B, T, -1))
        terms = [(mse, st[0])]
        if 'kld' in out:   # (kld_method 'none': plain SAVi has no such term)
            terms.append((out['kld'], out['kld'].detach().double()))
        return terms
    if kind == 'dvae':
        out = model({'img': img, 'gumbel_tau': tau, 'gumbel_seed': sd})
        mse, st = train.clip_mse(out['recon'].reshape(B, T, -1), img.reshape(B, T, -1))
        return [(mse, st[0])]
    # STEVE: the autograd chain itself -- no inference encode for the segmentation masks, which no loss reads
    model._reset_rnn()
    slots = model._encode_with_grad(img, None, None)[1]
    out = model._decode_tokens(img, slots, ids, gumbel_seed=sd)
    ce = model._token_recon_loss(out)
    terms = [(ce, ce.detach().double())]
    if model.use_img_recon_loss:
        mse, st = train.clip_mse(out['recon_img'].reshape(B, T, -1), out['gt_img'].reshape(B, T, -1))
        terms.append((mse, st[0]))
    return terms


def fit(model, frames, clips, epochs, batch_size, lr, seed, n_sample_frames, frame_offset=1, warmup_pct=0.05, min_lr_ratio=0.01, clip_grad=None,
        loss_w=None, mean=0.5, std=0.5, tokens=None, dec_lr=None, tau=(1., 0.1, 0.15), resume=None, stop_after=None, allreduce=False):
    """Train a base model in place on clips of a device-resident frame table, uint8 [V, T, H, W, 3] at `model.resolution` (what `FrameIngest`
    produces): the reference's base_slots run -- Adam at `lr` with linear warm-up over warmup_pct of the steps and cosine decay, gradient clipping
    (`clip_grad`) -- for
      StoSAVi / SAVi  loss_w[0] * post_recon_loss + loss_w[1] * kld_loss (default 1, 1e-4), decay to lr * min_lr_ratio; the kernel noise of step s
                      is `noise_seed = _step_seed(seed, s)` (`train.kernel_sample`: sample and KL term in one launch per frame); kld_method 'none'
                      has no such term;
      dVAE            recon_loss on clips of n_sample_frames frames (1 in the reference); the Gumbel temperature follows `cosine_anneal` from
                      tau[0] to tau[1] over the first tau[2] of the steps; `gumbel_seed = _step_seed(seed, s)`;
      STEVE           loss_w[0] * token_recon_loss (+ loss_w[1] * img_recon_loss with `use_img_recon_loss`); `dec_lr` is required: the Transformer
                      decoder's own rate (`train.steve_param_groups`), both groups decaying to 0; the targets come from `tokens` (int16 / int64
                      [V, T, h*w] on the device, the token files) or from `model.dvae.tokenize_ids` on the gathered batch; `fused_token_loss`
                      is honoured; the segmentation masks of `STEVE.encode`, which no loss reads, are not computed.

    clips: (video, start) pairs [M, 2] (`clip_index`); a clip is n_sample_frames frames, frame_offset apart.  All host work happens before the
    loop: the clips are validated against the table, the whole schedule (`clip_schedule(M, epochs, batch_size, seed)`) is uploaded, one FlatAdam is
    built, the rates and temperatures of every step are computed.  A step gathers its batch with `train.clip_frames`, takes the image losses
    through `train.clip_mse`, and ends in `FlatAdam.step()`: no synchronisation, no `.item()` and no host-to-device copy inside an epoch.  The
    dropout seeds of step s are drawn under `torch.random.fork_rng` after `torch.manual_seed(_step_seed(seed, s))`: one seed -> one result, and
    the caller's generator is left alone.

    Returns {TERMS name: its mean over the steps of every epoch run [epochs run] (device float32; None for a term the model does not have), 'state':
    {'optimizer', 'step', 'seed', 'epochs'}}.  stop_after / resume: as in `video_prediction.fit`."""
    from .. import train
    from ..video_prediction import _check_clips, _step_seed, _token_table, clip_schedule
    kind = _kind(model)
    who = 'fit'
    _check_frames(frames, model, who)
    T, f = int(n_sample_frames), int(frame_offset)
    if T < 1 or f < 1:
        raise ValueError(f'slotformer_amd.base_slots.fit: n_sample_frames >= 1 and frame_offset >= 1, got {n_sample_frames!r}, {frame_offset!r}')
    clips = _check_clips(clips, frames.shape, T, f)
    M = clips.shape[0]
    if tokens is not None:
        if kind != 'steve':
            raise ValueError('slotformer_amd.base_slots.fit: tokens= are the targets of the STEVE token loss; this model has none')
        _token_table(tokens, frames, model, who)
    if kind == 'steve' and dec_lr is None:
        raise ValueError('slotformer_amd.base_slots.fit: a STEVE model trains its Transformer decoder at a rate of its own: pass dec_lr=')
    loss_w = tuple(float(w) for w in (LOSS_W[kind] if loss_w is None else loss_w))
    if len(loss_w) < len(LOSS_W[kind]):
        raise ValueError(f'slotformer_amd.base_slots.fit: loss_w weighs {TERMS[kind]}, got {loss_w}')
    dev = frames.device
    sched = clip_schedule(M, epochs, batch_size, seed)
    per_epoch = len(sched[0]) if sched else 0
    if sched and per_epoch == 0:
        raise ValueError(f'slotformer_amd.base_slots.fit: {M} clips do not fill one batch of {batch_size}')
    require_device(frames, what='the frame table')
    total = per_epoch * len(sched)
    order = torch.stack([b for e in sched for b in e]).long() if total else torch.zeros(0, int(batch_size), dtype=torch.long)   # [total, B]
    sched_video = clips[:, 0][order].contiguous().to(dev)
    sched_start = clips[:, 1][order].contiguous().to(dev)
    warmup = float(warmup_pct) * total
    if kind == 'steve':
        peaks = (float(lr), float(dec_lr))
        opt = train.FlatAdam(train.steve_param_groups(model, *peaks), allreduce=allreduce, clip_grad=clip_grad)
        rates = [[train.warmup_cosine_lr(s, total, warmup, p) for p in peaks] for s in range(total)]
    else:
        opt = train.FlatAdam([p for p in model.parameters() if p.requires_grad], lr=lr, allreduce=allreduce, clip_grad=clip_grad)
        rates = [[train.warmup_cosine_lr(s, total, warmup, float(lr), float(lr) * float(min_lr_ratio))] for s in range(total)]
    taus = [cosine_anneal(s, tau[0], tau[1], float(tau[2]) * total) for s in range(total)] if kind == 'dvae' else None
    first = 0
    if resume is not None:
        if int(resume['seed']) != int(seed) or int(resume['epochs']) != int(epochs):
            raise ValueError('slotformer_amd.base_slots.fit: resume= continues a run of the same seed and epochs')
        first = int(resume['step'])
        if first % max(per_epoch, 1) or first > total:
            raise ValueError(f'slotformer_amd.base_slots.fit: resume at step {first} is not an epoch boundary of this schedule')
        opt.load_state_dict(resume['optimizer'])
    e0 = first // per_epoch if per_epoch else 0
    e1 = len(sched) if stop_after is None else min(len(sched), e0 + int(stop_after))
    stats = torch.zeros(max(e1 - e0, 0), len(TERMS[kind]), dtype=torch.float64, device=dev)
    was_training = model.training
    model.train()
    step = first
    for e in range(e0, e1):
        for _ in range(per_epoch):
            cv, cs = sched_video[step], sched_start[step]
            sd = _step_seed(seed, step)
            img = train.clip_frames(frames, cv, cs, f, 0, T, mean, std)
            ids = _steve_ids(model, tokens, img, cv, cs, T, f) if kind == 'steve' else None
            opt.zero_grad()
            with torch.random.fork_rng(devices=[]):
                torch.default_generator.manual_seed(sd)   # the dropout seeds (train._new_seed) of this step: torch.manual_seed's CPU half
                terms = _train_terms(kind, model, img, ids, sd, taus[step] if taus else None)
                sum(w * t for w, (t, _) in zip(loss_w, terms)).backward()
            for k, (_, value) in enumerate(terms):
                stats[e - e0, k] += value
            for g, rate in zip(opt.param_groups, rates[step]):
                g['lr'] = rate
            opt.step()
            step += 1
    model.train(was_training)
    n = float(max(per_epoch, 1))
    sd_opt = opt.state_dict()
    sd_opt['state'] = {i: {k: v.clone() for k, v in s.items()} for i, s in sd_opt['state'].items()}
    absent = 'kld_loss' if kind == 'savi' and model.kld_method == 'none' else 'img_recon_loss' if kind == 'steve' and not model.use_img_recon_loss else None
    out = {name: (stats[:, k] / n).float() if name != absent else None for k, name in enumerate(TERMS[kind])}
    out['state'] = {'optimizer': sd_opt, 'step': step, 'seed': int(seed), 'epochs': int(epochs)}
    return out


@torch.no_grad()
def evaluate(model, frames, clips, batch_size, n_sample_frames, frame_offset=1, seed=0, tokens=None, mean=0.5, std=0.5):
    """The loss terms of `calc_train_loss` over all `clips` of a device-resident frame table, without gradients, in eval mode, through the
    engine's inference path -> {TERMS name: a Python float}, each the mean over the clips.  Batches of `batch_size` clips in order (the last one
    ragged); the sums stay on the device and are downloaded once at the end.  Batch i draws from `_step_seed(seed, i)`: StoSAVi's kernel noise
    is `model.seeded_noise` of it, passed as `noise=`; the Gumbel noise of the dVAE and of STEVE's image loss is `gumbel_seed`.  STEVE's token
    loss comes from the forward of `train.head_cross_entropy` (no logits) unless its image loss needs them."""
    from .. import engine, train
    from ..video_prediction import _check_clips, _step_seed, _token_table
    kind = _kind(model)
    _check_frames(frames, model, 'evaluate')
    T, f, B = int(n_sample_frames), int(frame_offset), int(batch_size)
    if T < 1 or f < 1 or B < 1:
        raise ValueError(f'slotformer_amd.base_slots.evaluate: n_sample_frames, frame_offset, batch_size >= 1, got {n_sample_frames!r}, '
                         f'{frame_offset!r}, {batch_size!r}')
    clips = _check_clips(clips, frames.shape, T, f)
    M = clips.shape[0]
    if tokens is not None:
        if kind != 'steve':
            raise ValueError('slotformer_amd.base_slots.evaluate: tokens= are the targets of the STEVE token loss; this model has none')
        _token_table(tokens, frames, model, 'evaluate')
    require_device(frames, what='the frame table')
    dev = frames.device
    cv_all, cs_all = clips[:, 0].contiguous().to(dev), clips[:, 1].contiguous().to(dev)
    sums = {}
    was_training = model.training
    model.eval()
    for i, s in enumerate(range(0, M, B)):
        cv, cs = cv_all[s:s + B], cs_all[s:s + B]
        b = cv.numel()
        sd = _step_seed(seed, i)
        img = train.clip_frames(frames, cv, cs, f, 0, T, mean, std)
        if kind == 'savi':
            data = {'img': img, 'noise': model.seeded_noise(sd, b, T, dev) if model.kld_method != 'none' else None}
            terms = model.calc_train_loss(data, model(data))
        elif kind == 'dvae':
            data = {'img': img, 'gumbel_seed': sd}
            terms = model.calc_train_loss(data, model(data))
        else:
            ids = _steve_ids(model, tokens, img, cv, cs, T, f)
            slots = engine.savi_encode(model, img, prev_slots=None, noise=None)[0]
            if model.use_img_recon_loss:
                terms = model.calc_train_loss(None, model._decode_tokens(img, slots, ids, gumbel_seed=sd))
            else:
                dec = model.trans_decoder
                flat = ids.flatten(0, 1)
                hidden = train.slate_decoder_hidden(dec, slots.flatten(0, 1), flat[:, :-1].contiguous())
                terms = {'token_recon_loss': train.head_cross_entropy(hidden, dec.head, flat, weight_grad=True)[0]}
        for name, t in terms.items():
            sums[name] = sums.get(name, 0.) + t.double() * b
    model.train(was_training)
    names = sorted(sums)
    host = torch.stack([sums[k] for k in names]).cpu() / M
    return {k: float(v) for k, v in zip(names, host)}
