"""slotformer.video_prediction counterpart: exports build_model, and the loop that trains a rollouter on slots that live on the device -- `fit`
(the reference's nerv run of SlotFormerMethod: Adam, warm-up + cosine, the decaying step weights, optionally the image loss) and `evaluate`
(its eval branch) -- around `clip_index`, `clip_schedule` and `loss_decay_weights`.  The whole slot file of a dataset fits the HBM of one MI355X many
times over, so a batch is a list of (video, start) pairs and never a gathered copy."""
from types import SimpleNamespace

import torch

from .._call import require_device
from .models import build_model

MIN_FRAMES = 3   # datasets/clevrer.py:240: an object entering fewer than this many frames into the burn-in does not spoil a clip


def build_dataset(params, *a, **k):
    raise NotImplementedError('datasets are host-side I/O outside the hot path (SURVEY.md 2.1 row 13)')


def build_method(*a, **k):
    raise NotImplementedError('the nerv trainer is outside the hot path (SURVEY.md 2.1 row 12)')


def clip_index(num_videos, video_len, n_sample_frames, frame_offset, split, enter_times=None, warmup_len=None):
    """The (video, start) pairs CLEVRERDataset samples clips from (base_slots/datasets/clevrer.py:202-275) -> int32 [M, 2] on the host.
    A clip is n_sample_frames frames, frame_offset apart.  Without `enter_times`: 'train' takes every start at which a clip fits; 'val' / 'test'
    cut the video into blocks of n_sample_frames * frame_offset frames and take the frame_offset interleaved clips of each, so every frame is
    used once.  With `enter_times` (per video the frames at which an object enters the view; the dataset's filter_enter): a start is dropped when
    an object enters at a frame t with start + (warmup_len - MIN_FRAMES) * frame_offset < t <= the clip's last frame; 'train' keeps every other
    start, 'val' / 'test' walk blocks of half a clip's span and keep the first surviving start of each.  warmup_len: default 5, the dataset's."""
    V, T, n, f = int(num_videos), int(video_len), int(n_sample_frames), int(frame_offset)
    if split not in ('train', 'val', 'test'):
        raise ValueError(f"slotformer_amd.video_prediction: split is 'train', 'val' or 'test', got {split!r}")
    if V < 0 or n < 1 or f < 1 or T < 1:
        raise ValueError(f'slotformer_amd.video_prediction: num_videos >= 0, video_len, n_sample_frames, frame_offset >= 1, got {V}, {T}, {n}, {f}')
    if enter_times is not None and len(enter_times) != V:
        raise ValueError(f'slotformer_amd.video_prediction: {V} videos, enter_times of {len(enter_times)}')
    warmup = 5 if warmup_len is None else int(warmup_len)
    span = (n - 1) * f               # first to last frame of a clip
    n_starts = T - span              # starts 0 .. n_starts - 1 fit

    def spoiled(enter, start):
        lo, hi = start + (warmup - MIN_FRAMES) * f, start + span
        return any(lo < t <= hi for t in enter)

    pairs = []
    for v in range(V):
        enter = None if enter_times is None else [int(t) for t in enter_times[v]]
        if split == 'train':
            pairs += [(v, s) for s in range(max(n_starts, 0)) if enter is None or not spoiled(enter, s)]
        elif enter is None:
            block = n * f
            pairs += [(v, b + i) for b in range(0, T - block + 1, block) for i in range(f)]
        else:
            half = span // 2
            if half < 1:
                raise ValueError('slotformer_amd.video_prediction: the filtered val / test index needs clips that span at least 2 frames')
            for b in range(0, T - span, half):
                s = next((s for s in range(b, min(b + half, T - span)) if not spoiled(enter, s)), None)
                if s is not None:
                    pairs.append((v, s))
    return torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2)


def clip_schedule(num_clips, epochs, batch_size, seed, drop_last=True):
    """The batches `fit` trains on, in the style of physion_vqa.batch_schedule: per epoch one permutation of the clips from a generator seeded with
    `seed` (the epochs continue one stream), cut into batches of `batch_size`; the ragged last batch of an epoch is dropped (the reference's
    training loader) unless drop_last=False.  -> [epoch][batch] int32 index tensors on the host.  A function of its arguments alone."""
    M, E, B = int(num_clips), int(epochs), int(batch_size)
    if M < 1 or E < 0 or B < 1:
        raise ValueError(f'slotformer_amd.video_prediction: num_clips >= 1, epochs >= 0, batch_size >= 1, got {num_clips!r}, {epochs!r}, {batch_size!r}')
    gen = torch.Generator().manual_seed(int(seed))
    out = []
    for _ in range(E):
        batches = list(torch.randperm(M, generator=gen).to(torch.int32).split(B))
        if drop_last and batches and batches[-1].numel() < B:
            batches.pop()
        out.append(batches)
    return out


def loss_decay_factor(step, total_steps, decay_pct):
    """SlotFormerMethod._training_step_start (video_prediction/method.py:33-48): linear from 0.01 to 1 over the first decay_pct * total_steps
    steps, then 1.  decay_pct None (use_loss_decay off): 1."""
    if decay_pct is None:
        return 1.
    decay_steps = float(decay_pct) * int(total_steps)
    if step >= decay_steps:
        return 1.
    return 0.01 + step / decay_steps * 0.99


def loss_decay_weights(step, total_steps, decay_pct, S):
    """The per-step loss weights at training step `step` (slotformer.py:299-304): w = f**arange(S), w / w.sum() * S with f = loss_decay_factor
    -> float64 [S] on the host, or None (uniform) once the factor has reached 1."""
    f = loss_decay_factor(step, total_steps, decay_pct)
    if not f < 1.:
        return None
    w = torch.tensor(f, dtype=torch.float64)**torch.arange(int(S), dtype=torch.float64)
    return w / w.sum() * int(S)


def _check_clips(clips, table_shape, n_frames, frame_offset):
    clips = torch.as_tensor(clips).cpu()
    if clips.dim() != 2 or clips.shape[1] != 2 or clips.shape[0] < 1 or clips.is_floating_point():
        raise ValueError(f'slotformer_amd.video_prediction: clips are integer (video, start) pairs [M, 2], got {tuple(clips.shape)} {clips.dtype}')
    V, T = table_shape[:2]
    last = clips[:, 1].long() + (n_frames - 1) * frame_offset
    bad = (clips[:, 0] < 0) | (clips[:, 0] >= V) | (clips[:, 1] < 0) | (last >= T)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise ValueError(f'slotformer_amd.video_prediction: clip {i} = {tuple(clips[i].tolist())} with {n_frames} frames at offset {frame_offset} does '
                         f'not fit a table of {V} videos x {T} frames')
    return clips.to(torch.int32)


def _device_table(table):
    require_device(table, what='the slot table')
    return table


def _step_seed(seed, step):
    """The dropout seed of training step `step`: a function of (seed, step) alone, never 0."""
    return ((int(seed) * 0x9E3779B97F4A7C15 + (step + 1) * 0xD1B54A32D192ED03) % (2**62 - 1)) + 1


def _image_step(model, table, frames, cv, cs, frame_offset, hist, S, seed, grad_out, step_w, clip_len, mean, std, loss_w):
    """One forward of `fit` with the image loss (slotformer.py:272-281,313-326) as autograd nodes: the clip rollout, the frozen decoder on the
    predicted slots, and the two fused losses -> (pred, slot loss, image loss, slot stats, image stats).  Backward of their sum fills grad_out."""
    from .. import train
    r = model.rollouter
    pred = train.rollout_clips_with_grad(r, table, cv, cs, frame_offset, S, seed=seed, grad_out=grad_out)
    B = pred.shape[0]
    recon = train.decode_with_grad(model, pred.flatten(0, 1))[0]
    target = train.clip_frames(frames, cv, cs, frame_offset, hist, S, mean, std)
    slot_loss, slot_stats = train.clip_mse(pred, table, cv, cs, frame_offset, hist, step_w, clip_len, loss_w[0])
    img_loss, img_stats = train.clip_mse(recon.reshape(B, S, -1), target.reshape(B, S, -1), hist=hist, clip_len=clip_len, scale=loss_w[1])
    return pred, slot_loss, img_loss, slot_stats, img_stats


def _token_table(tokens, table, model, who):
    """The checks of a tokens= argument: an int16 / int64 device tensor [V, T, h*w] beside the slot table, for a model with a dVAE."""
    if not hasattr(model, 'dvae'):
        raise ValueError(f'slotformer_amd.video_prediction.{who}: tokens= is the target of the STEVE token loss; this model has no dVAE (its image '
                         'loss takes frames=)')
    hw = int(model.h) * int(model.w)
    if not torch.is_tensor(tokens) or tokens.dtype not in (torch.int16, torch.int64) or tokens.dim() != 3 or \
            tuple(tokens.shape[:2]) != tuple(table.shape[:2]) or tokens.shape[2] != hw or not tokens.is_contiguous():
        raise ValueError(f'slotformer_amd.video_prediction.{who}: tokens are contiguous int16 or int64 ids [{table.shape[0]}, {table.shape[1]}, {hw}], '
                         f'got {getattr(tokens, "dtype", type(tokens).__name__)} {tuple(getattr(tokens, "shape", ()))}')
    require_device(tokens, what='the token table')
    return tokens


def _frame_weights(clip_len, hist, S):
    """clip_len int32 [..., B] -> float32 [..., B * S]: 1 where step s of clip b counts (hist + s < clip_len[b], clip_mse's rule), else 0."""
    return (hist + torch.arange(S, device=clip_len.device) < clip_len[..., None]).float().flatten(-2)


def _clip_token_ids(tokens, cv, cs, frame_offset, hist, S):
    """The ids of the S predicted frames of every clip, picked from the token table on the device -> [B * S, h*w] in the table's dtype."""
    t = cs.long()[:, None] + (hist + torch.arange(S, device=cs.device)) * frame_offset
    return tokens[cv.long()[:, None], t].flatten(0, 1)


def _token_step(model, table, tokens, cv, cs, frame_offset, hist, S, seed, grad_out, step_w, clip_len, frame_w, loss_w):
    """One forward of `fit` with the STEVE token loss (steve_slotformer.py:124-161) as autograd nodes: the clip rollout, the frozen Transformer
    decoder on the predicted slots up to its final LayerNorm, and the vocabulary head fused with the cross-entropy against the table's ids -- no
    logits -> (pred, slot loss, token loss (weighted by loss_w[1]), slot stats, the token loss itself).  frame_w [B * S] or None: `_frame_weights`
    of clip_len.  Backward of the sum of the two losses fills grad_out."""
    from .. import train
    pred = train.rollout_clips_with_grad(model.rollouter, table, cv, cs, frame_offset, S, seed=seed, grad_out=grad_out)
    ids = _clip_token_ids(tokens, cv, cs, frame_offset, hist, S)
    hidden = train.slate_decoder_hidden(model.decoder, pred.flatten(0, 1), ids[:, :-1].contiguous())
    ce, _ = train.head_cross_entropy(hidden, model.decoder.head, ids, frame_w, ids.shape[1])
    slot_loss, slot_stats = train.clip_mse(pred, table, cv, cs, frame_offset, hist, step_w, clip_len, loss_w[0])
    return pred, slot_loss, ce * float(loss_w[1]), slot_stats, ce.detach()


def fit(model, table, clips, epochs, batch_size, lr, seed, frame_offset, warmup_pct=0.05, min_lr_ratio=0.01, clip_grad=None, loss_decay_pct=None,
        clip_len=None, frames=None, mean=0.5, std=0.5, loss_w=(1., 1.), resume=None, allreduce=False, stop_after=None, tokens=None):
    """Train `model.rollouter` in place on clips of a device-resident slot table [V, T, N, C] (SlotFormer, SingleStepSlotFormer, and
    STEVESlotFormer): the reference's SlotFormerMethod run -- Adam at `lr` with linear warm-up over warmup_pct of the steps
    and cosine decay to lr * min_lr_ratio, gradient clipping (`clip_grad`), the step weights of `loss_decay_weights` (`loss_decay_pct`), the
    vid_len truncation (`clip_len`: the length of every clip, [M]) and, with `frames` (uint8 [V, T, H, W, 3] at the decoder's resolution) and
    `model.use_img_recon_loss`, the image loss through the frozen decoder, the two terms weighted by `loss_w`.  A STEVESlotFormer takes its image
    term from `tokens` instead (int16 or int64 ids [V, T, h*w] on the device, what `extract_video_tokens(to_host=False)` returns and the token
    files hold): the cross-entropy of the frozen Transformer decoder against the ids of the predicted frames, its vocabulary head fused with
    the loss (`train.head_cross_entropy`), so that no step allocates anything of rows x vocabulary elements.

    clips: (video, start) pairs [M, 2] (`clip_index`); a clip is burn-in + model.rollout_len frames, frame_offset apart.  All host work happens
    before the loop: the clips are validated against the table, the whole schedule (`clip_schedule(M, epochs, batch_size, seed)`) and the whole
    [steps, S] weight table are uploaded, one FlatAdam is built over the rollouter's parameters.  A step is the clip forward, the fused loss --
    whose gradient the backward turns into the optimiser's bucket directly -- and `FlatAdam.step(gathered=True)`: no synchronisation, no `.item()`
    and no host-to-device copy inside an epoch, one seed -> one result, bit for bit.

    Returns {'loss': the mean slot loss of every epoch run [epochs run] (device), 'img_loss': the same for the image / token term or None, 'state':
    {'optimizer', 'step', 'seed', 'epochs'}}.  stop_after: run only that many epochs of the `epochs` the schedule is laid out for; `state` fed
    back as resume= (same seed, epochs and data) continues where that run stopped and ends where the straight run would have."""
    from .. import train
    _device_table(table)
    r = model.rollouter
    dev = table.device
    hist, S, f = train.burnin_len(r), int(model.rollout_len), int(frame_offset)
    clips = _check_clips(clips, table.shape, hist + S, f)
    M = clips.shape[0]
    use_img = frames is not None and bool(getattr(model, 'use_img_recon_loss', False))
    if use_img and not hasattr(model, 'decoder_pos_embedding'):
        raise NotImplementedError('slotformer_amd.video_prediction.fit: frames= is the image loss of the SAVi decoder; a STEVE model trains its token '
                                  'loss from tokens= (the ids of extract_video_tokens)')
    if tokens is not None:
        _token_table(tokens, table, model, 'fit')
    use_tok = tokens is not None and bool(getattr(model, 'use_img_recon_loss', False))
    if use_img and (tuple(frames.shape[:2]) != tuple(table.shape[:2]) or tuple(frames.shape[2:4]) != tuple(model.resolution)):
        raise ValueError(f'slotformer_amd.video_prediction.fit: frames are uint8 [{table.shape[0]}, {table.shape[1]}, {model.resolution[0]}, '
                         f'{model.resolution[1]}, 3], got {tuple(frames.shape)}')
    sched = clip_schedule(M, epochs, batch_size, seed)
    per_epoch = len(sched[0]) if sched else 0
    if sched and per_epoch == 0:
        raise ValueError(f'slotformer_amd.video_prediction.fit: {M} clips do not fill one batch of {batch_size}')
    total = per_epoch * len(sched)
    order = torch.stack([b for e in sched for b in e]).long() if total else torch.zeros(0, int(batch_size), dtype=torch.long)   # [total, B]
    sched_video = clips[:, 0][order].contiguous().to(dev)
    sched_start = clips[:, 1][order].contiguous().to(dev)
    sched_len = None
    if clip_len is not None:
        clip_len = torch.as_tensor(clip_len).cpu().to(torch.int32).flatten()
        if clip_len.numel() != M:
            raise ValueError(f'slotformer_amd.video_prediction.fit: {M} clips, clip_len of {clip_len.numel()}')
        sched_len = clip_len[order].contiguous().to(dev)
    sched_fw = _frame_weights(sched_len, hist, S) if use_tok and sched_len is not None else None   # [total, B * S]
    rows = [loss_decay_weights(s, total, loss_decay_pct, S) for s in range(total)]
    n_decay = sum(w is not None for w in rows)   # (the factor only grows: the decaying steps come first)
    w_table = torch.stack([w.float() for w in rows[:n_decay]]).to(dev) if n_decay else None

    params = train.rollouter_parameters(r) + train.learnable_tables(r)
    for p in train.rollouter_parameters(r):
        p.requires_grad_(True)
    opt = train.FlatAdam(params, lr=lr, allreduce=allreduce, clip_grad=clip_grad)
    first = 0
    if resume is not None:
        if int(resume['seed']) != int(seed) or int(resume['epochs']) != int(epochs):
            raise ValueError('slotformer_amd.video_prediction.fit: resume= continues a run of the same seed and epochs')
        first = int(resume['step'])
        if first % max(per_epoch, 1) or first > total:
            raise ValueError(f'slotformer_amd.video_prediction.fit: resume at step {first} is not an epoch boundary of this schedule')
        opt.load_state_dict(resume['optimizer'])
    e0 = first // per_epoch if per_epoch else 0
    e1 = len(sched) if stop_after is None else min(len(sched), e0 + int(stop_after))
    stats = torch.zeros(max(e1 - e0, 0), 1 + 2 * S, dtype=torch.float64, device=dev)
    img_stats = torch.zeros_like(stats) if use_img else None
    tok_sum = torch.zeros(stats.shape[0], dtype=torch.float64, device=dev) if use_tok else None
    warmup = float(warmup_pct) * total
    was_training = r.training
    r.train()
    ws = d_pred = None
    step = first
    for e in range(e0, e1):
        for _ in range(per_epoch):
            cv, cs = sched_video[step], sched_start[step]
            cl = None if sched_len is None else sched_len[step]
            sw = w_table[step] if step < n_decay else None
            sd = _step_seed(seed, step)
            if use_img:
                _, slot_loss, img_loss, st, ist = _image_step(model, table, frames, cv, cs, f, hist, S, sd, opt.grad, sw, cl, mean, std, loss_w)
                (slot_loss + img_loss).backward()
                stats[e - e0] += st
                img_stats[e - e0] += ist
            elif use_tok:
                fw = None if sched_fw is None else sched_fw[step]
                _, slot_loss, tok_loss, st, ce = _token_step(model, table, tokens, cv, cs, f, hist, S, sd, opt.grad, sw, cl, fw, loss_w)
                (slot_loss + tok_loss).backward()
                stats[e - e0] += st
                tok_sum[e - e0] += ce
            else:
                with torch.no_grad():
                    p_drop = float(r.transformer_encoder.layers[0].dropout.p)
                    pred, plan, ws = train._clips_forward(r, table, cv, cs, f, S, p_drop, sd, ws)
                    if d_pred is None:
                        d_pred = torch.empty_like(pred)
                    train.clip_mse_launch(pred, table, cv, cs, f, hist, sw, cl, loss_w[0], d_pred, stats[e - e0])
                    # (what the backward reads from a forward node; `ws` stays ours, so the next step's forward takes it again)
                    ctx = SimpleNamespace(r=r, plan=plan, ws=ws, args=(pred.shape[0], S, p_drop, sd), params=tuple(params))
                    train._rollout_backward(ctx, d_pred, None, opt.grad)
            opt.lr = train.warmup_cosine_lr(step, total, warmup, lr, lr * float(min_lr_ratio))
            opt.step(gathered=True)
            step += 1
    r.train(was_training)
    n = float(max(per_epoch, 1))
    sd_opt = opt.state_dict()
    sd_opt['state'] = {i: {k: v.clone() for k, v in s.items()} for i, s in sd_opt['state'].items()}
    return {'loss': (stats[:, 0] / (n * (float(loss_w[0]) or 1.))).float(),
            'img_loss': (img_stats[:, 0] / (n * (float(loss_w[1]) or 1.))).float() if use_img else (tok_sum / n).float() if use_tok else None,
            'state': {'optimizer': sd_opt, 'step': step, 'seed': int(seed), 'epochs': int(epochs)}}


@torch.no_grad()
def evaluate(model, table, clips, batch_size, frame_offset, clip_len=None, tokens=None):
    """The reference's eval branch (slotformer.py:291-295,318) over all `clips` of a device-resident slot table, without gradients and without
    dropout: -> {'slot_recon_loss': the mean squared error over every counted element, 'slot_recon_loss_1' .. '_k', k = min(6, rollout_len): the
    same per rollout step} as Python floats.  Batches of `batch_size` clips in order (the last one ragged); the sums stay on the device and are
    downloaded once at the end.  clip_len [M]: the vid_len truncation.  tokens (a STEVESlotFormer with use_img_recon_loss; the table of `fit`):
    adds 'img_recon_loss', the mean token cross-entropy over every counted frame."""
    from .. import train
    _device_table(table)
    r = model.rollouter
    dev = table.device
    hist, S, f = train.burnin_len(r), int(model.rollout_len), int(frame_offset)
    clips = _check_clips(clips, table.shape, hist + S, f)
    M = clips.shape[0]
    if int(batch_size) < 1:
        raise ValueError(f'slotformer_amd.video_prediction: batch_size >= 1, got {batch_size!r}')
    cv_all, cs_all = clips[:, 0].contiguous().to(dev), clips[:, 1].contiguous().to(dev)
    cl_all = None
    if clip_len is not None:
        cl_all = torch.as_tensor(clip_len).to(torch.int32).flatten().to(dev)
        if cl_all.numel() != M:
            raise ValueError(f'slotformer_amd.video_prediction.evaluate: {M} clips, clip_len of {cl_all.numel()}')
    if tokens is not None:
        _token_table(tokens, table, model, 'evaluate')
    use_tok = tokens is not None and bool(getattr(model, 'use_img_recon_loss', False))
    stats = torch.zeros(1 + 2 * S, dtype=torch.float64, device=dev)
    tok_stats = torch.zeros(2, dtype=torch.float64, device=dev)
    fw_all = _frame_weights(cl_all, hist, S).reshape(M, S) if use_tok and cl_all is not None else None
    ws = None
    for s in range(0, M, int(batch_size)):
        e = min(s + int(batch_size), M)
        pred, _, ws = train._clips_forward(r, table, cv_all[s:e], cs_all[s:e], f, S, 0., 0, ws)
        train.clip_mse_launch(pred, table, cv_all[s:e], cs_all[s:e], f, hist, None, None if cl_all is None else cl_all[s:e], 1., None, stats)
        if use_tok:
            ids = _clip_token_ids(tokens, cv_all[s:e], cs_all[s:e], f, hist, S)
            hidden = train.slate_decoder_hidden(model.decoder, pred.flatten(0, 1), ids[:, :-1].contiguous())
            tok_stats += train.head_cross_entropy(hidden, model.decoder.head, ids, None if fw_all is None else fw_all[s:e].reshape(-1), ids.shape[1])[1]
    h = stats.cpu()
    sums, counts = h[1:1 + S], h[1 + S:]
    out = {'slot_recon_loss': float(sums.sum() / counts.sum())}
    if use_tok:
        th = tok_stats.cpu()
        out['img_recon_loss'] = float(th[0] / th[1])
    for k in range(min(6, S)):
        out[f'slot_recon_loss_{k + 1}'] = float(sums[k] / counts[k])
    return out
