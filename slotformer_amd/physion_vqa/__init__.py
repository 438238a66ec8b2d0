"""slotformer.physion_vqa counterpart: build_model, and the two drivers around the readout -- `fit` (the reference's nerv training run of
readout_physion_params.py) and `evaluate` (test_physion_vqa.py) -- on a device-resident slots tensor."""
import math

import torch

from .models import build_model, PhysionReadout
from .. import ops

TEST_THRESHS = (0.4, 0.45, 0.5, 0.55, 0.6, 0.65)   # test_physion_vqa.py --threshs


def build_dataset(params, *a, **k):
    raise NotImplementedError('datasets are host-side I/O outside the hot path (SURVEY.md 2.1 row 13)')


def build_method(*a, **k):
    raise NotImplementedError('the nerv trainer is outside the hot path (SURVEY.md 2.1 row 12)')


def batch_schedule(num_videos, epochs, batch_size, seed):
    """The batches `fit` trains on: per epoch one permutation of the videos from a generator seeded with `seed` (the epochs continue one stream),
    cut into batches of `batch_size`; the last batch of an epoch may be ragged.  -> [epoch][batch] int32 tensors on the host.  A function of its
    arguments alone."""
    if int(num_videos) < 1 or int(epochs) < 0 or int(batch_size) < 1:
        raise ValueError(f'slotformer_amd.physion_vqa: num_videos >= 1, epochs >= 0, batch_size >= 1, got {num_videos!r}, {epochs!r}, {batch_size!r}')
    gen = torch.Generator().manual_seed(int(seed))
    return [list(torch.randperm(int(num_videos), generator=gen).to(torch.int32).split(int(batch_size))) for _ in range(int(epochs))]


def step_seed(seed, step):
    """The dropout seed of optimiser step `step` of a `fit` run seeded with `seed`: the run's seed in the high word, the step in the low one
    (one rule for every `fit` whose layers drop: phyre_planning, clevrer_vqa)."""
    return ((int(seed) & 0xffffffff) << 32) | (int(step) & 0xffffffff)


def _head(readout):
    return readout.linear1.weight, readout.linear1.bias, readout.linear2.weight, readout.linear2.bias


def fit(readout, slots, labels, epochs, batch_size, lr, seed, video_len=75):
    """Train `readout` in place on slots [V,T,N,C] and labels [V] that live on the device (readout_physion_params.py: Adam, cosine decay to 0
    without warm-up, batches of 64, the first 75 frames).  A batch is picked by `video_index` (`batch_schedule`), never gathered; a step is the
    forward, the score (loss and dL/dlogit) and the backward -- which writes the four gradients into one flat buffer the parameters' `.grad`
    are views of -- and the `FlatAdam` step.  Everything is deterministic: one seed, one result, bit for bit.  Returns the mean loss of every
    epoch, [epochs] on the device."""
    from ..train import FlatAdam, warmup_cosine_lr
    readout._check(slots)
    dev = slots.device
    labels = torch.as_tensor(labels, device=dev).float().flatten()
    V = slots.shape[0]
    if labels.numel() != V:
        raise ValueError(f'slotformer_amd.physion_vqa: {V} videos, {labels.numel()} labels')
    params = list(_head(readout))
    for p in params:
        p.requires_grad_(True)
    opt = FlatAdam(params, lr=lr)
    grad = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=dev)
    off = 0
    for p in params:   # (the bucket order of FlatAdam is the order of ops.physion_readout_bwd's buffer)
        p.grad = grad[off:off + p.numel()].view_as(p)
        off += p.numel()
    sched = batch_schedule(V, epochs, batch_size, seed)
    total = sum(len(e) for e in sched)
    step, losses = 0, []
    readout.train()
    with torch.no_grad():
        for batches in sched:
            epoch_loss = torch.zeros((), dtype=torch.float32, device=dev)
            for idx in batches:
                idx = idx.to(dev)
                W1, b1, w2, b2 = _head(readout)
                logits, t_star, _, pairs = ops.physion_readout_fwd(slots, W1, b1, w2, b2, readout.agg_func, video_index=idx, video_len=video_len,
                                                                   want_pairs=readout.agg_func == 'max')
                loss, g, _, _ = ops.physion_readout_score(logits, labels[idx.long()])
                ops.physion_readout_bwd(slots, W1, b1, w2, g, t_star, readout.agg_func, pair_star=pairs, video_index=idx, video_len=video_len,
                                        out=grad)
                opt.lr = warmup_cosine_lr(step, total, 0, lr, 0.)
                opt.step()
                step += 1
                epoch_loss += loss[0] * (idx.numel() / V)
            losses.append(epoch_loss)
    return torch.stack(losses) if losses else torch.zeros(0, device=dev)


def _stack_heads(models, agg_func, dev):
    """A PhysionReadout, a state dict, or a list of either -> (N, agg, W1 [K,F,2C], b1 [K,F], w2 [K,F], b2 [K]) on the device."""
    if isinstance(models, (PhysionReadout, dict)):
        models = [models]
    models = list(models)
    if not models:
        raise ValueError('slotformer_amd.physion_vqa: no readout to evaluate')
    sds = []
    for m in models:
        if isinstance(m, PhysionReadout):
            agg_func = m.agg_func
            m = m.state_dict()
        sds.append(m.get('state_dict', m))   # (a checkpoint file's dict holds the weights under 'state_dict', test_physion_vqa.py:30)
    pairs2 = sds[0]['comb_idx'].numel()
    N = (1 + math.isqrt(1 + 4 * pairs2)) // 2
    cat = lambda k: torch.stack([sd[k].detach().to(dev).float() for sd in sds])
    K = len(sds)
    return N, agg_func, cat('linear1.weight'), cat('linear1.bias'), cat('linear2.weight').reshape(K, -1), cat('linear2.bias').reshape(K)


@torch.no_grad()
def evaluate(readout_or_state_dicts, slots, labels, task_idx=None, threshs=TEST_THRESHS, batch_size=128, video_len=75, agg_func='max'):
    """test_physion_vqa.py for K checkpoints x the thresholds in ONE pass over the slots: every batch is one forward launch over all K heads and
    one score launch that adds to int32 counters.  slots [V,T,N,C] and labels [V] (task_idx [V]: the per-task table) on the device;
    readout_or_state_dicts: a PhysionReadout, a state dict, or a list of them (`agg_func` names the aggregate of bare state dicts).
    Returns {'acc': [K, thresholds] float64 (host), 'task_acc': [K, tasks, thresholds] or None, 'best': (k, threshold index) as the reference's
    two nested argmax pick it -- the first best threshold, and at it the first best checkpoint -- 'best_acc', 'counts', 'task_counts'}."""
    if not (torch.is_tensor(slots) and slots.is_cuda):
        raise RuntimeError('slotformer_amd: PhysionReadout runs on a HIP device only; there is no CPU fallback')
    dev = slots.device
    N, agg, W1, b1, w2, b2 = _stack_heads(readout_or_state_dicts, agg_func, dev)
    C, F = W1.shape[2] // 2, W1.shape[1]
    if not ops.physion_readout_ok(N, C, F):
        raise NotImplementedError(f'PhysionReadout(num_slots={N}, slot_size={C}, feats_dim={F}) has no kernel: {ops.READOUT_LIMITS}')
    if tuple(slots.shape[2:]) != (N, C):
        raise ValueError(f'slotformer_amd.physion_vqa: slots are [V, T, {N}, {C}], got {tuple(slots.shape)}')
    if int(batch_size) < 1:
        raise ValueError(f'slotformer_amd.physion_vqa: batch_size >= 1, got {batch_size!r}')
    V = slots.shape[0]
    labels = torch.as_tensor(labels, device=dev).float().flatten()
    n_tasks = 0
    if task_idx is not None:
        task_idx = torch.as_tensor(task_idx, device=dev).to(torch.int32).flatten()
        n_tasks = int(task_idx.max().item()) + 1
    counts = task_counts = None
    for s in range(0, V, int(batch_size)):
        idx = torch.arange(s, min(s + int(batch_size), V), dtype=torch.int32, device=dev)
        logits = ops.physion_readout_fwd(slots, W1, b1, w2, b2, agg, video_index=idx, video_len=video_len)[0]
        _, _, counts, task_counts = ops.physion_readout_score(logits, labels[s:s + idx.numel()], threshs=threshs,
                                                              task_idx=None if task_idx is None else task_idx[s:s + idx.numel()],
                                                              n_tasks=n_tasks, want_loss=False, want_grad=False, counts=counts, task_counts=task_counts)
    counts_h = counts.cpu()
    acc = counts_h.double() / V
    task_acc = None
    if task_counts is not None:
        per_task = torch.bincount(task_idx.long().cpu(), minlength=n_tasks).double().clamp(min=1)
        task_acc = task_counts.cpu().double() / per_task[None, :, None]
    # test_physion_vqa.py: per threshold the first best checkpoint (main), then the first best threshold (__main__)
    best_k = counts_h.argmax(0)   # (integers: ties are exact; torch's argmax returns the first maximum)
    best_per_thresh = counts_h.max(0).values
    ti = int(best_per_thresh.argmax())
    return {'acc': acc, 'task_acc': task_acc, 'best': (int(best_k[ti]), ti), 'best_acc': float(acc[best_k[ti], ti]), 'counts': counts_h,
            'task_counts': None if task_counts is None else task_counts.cpu()}
