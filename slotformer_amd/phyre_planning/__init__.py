"""slotformer.phyre_planning counterpart: build_model, the two drivers around the classifier -- `fit` (the reference's nerv training run of
readout_phyre_params-fold0.py) and `evaluate` -- on a device-resident slots tensor, the frame table the planning driver feeds the classifier
with, and AUCCESS (test_phyre_planning.py: collect_results) from a table of confidences.  The planning driver itself is `harness.phyre_plan`."""
import numpy as np
import torch

from .models import build_model, PHYREReadout
from .models.readout import ACC_THRESHS
from ..physion_vqa import batch_schedule, step_seed   # noqa: F401  (one rule for the batches and the dropout seeds of every fit)
from .. import ops

# phyre.SimulationStatus, as the simulation caches store it
INVALID_INPUT = 0
NOT_SOLVED = -1
SOLVED = 1          # (anything > 0 counts as solved: UNSTABLY_SOLVED 1, STABLY_SOLVED 2)
INVALID_CONF = -1.  # the confidence test_phyre_planning.py pads invalid actions with
MAX_ATTEMPTS = 100  # AUCCESS looks at the first 100 attempts


def build_dataset(params, *a, **k):
    raise NotImplementedError('datasets are host-side I/O outside the hot path (SURVEY.md 2.1 row 13)')


def build_method(*a, **k):
    raise NotImplementedError('the nerv trainer is outside the hot path (SURVEY.md 2.1 row 12); the training kernels of PHYREReadout are reached through '
                              'phyre_planning.fit / train.phyre_readout_with_grad; a trainer object is not built')


def fit(readout, slots, labels, epochs, batch_size=256, lr=1e-3, seed=0, warmup_steps_pct=0.1, sel=None):
    """Train `readout` in place on slots [V, T_all, N, C] and labels [V] that live on the device (readout_phyre_params-fold0.py: Adam at 1e-3,
    10 % linear warm-up then cosine decay to 0, batches of 256, dropout 0.1 from nn.TransformerEncoderLayer).  A batch is picked by `video_index`
    (`physion_vqa.batch_schedule` on `seed`), never gathered; a step is the training forward (one launch per layer), the score (loss and
    dL/dlogit), the backward (one launch per layer for the activation gradients) -- which writes every gradient straight into the optimiser's flat
    bucket -- and one `FlatAdam` launch.  The dropout masks of step k come from `step_seed(seed, k)`.  Nothing is uploaded, downloaded or waited
    for inside an epoch, and everything is deterministic: one seed, one result, bit for bit.  sel: the frame table (default readout.sel_slots).
    Leaves the module in eval() with its cached plans dropped, so the next `logits_of` sees the trained weights.  Returns the mean loss of every
    epoch, [epochs] on the device."""
    from .. import plans
    from ..train import FlatAdam, warmup_cosine_lr, phyre_readout_parameters, phyre_readout_model, phyre_learnable_pe
    if not torch.is_tensor(slots) or slots.dim() != 4 or tuple(slots.shape[2:]) != (readout.num_slots, readout.slot_size):
        raise ValueError(f'slotformer_amd.phyre_planning: slots are a [V, T, {readout.num_slots}, {readout.slot_size}] tensor, got '
                         f'{tuple(getattr(slots, "shape", ()))}')
    dev = slots.device
    V, T_all = slots.shape[:2]
    labels = torch.as_tensor(labels, device=dev).float().flatten()
    if labels.numel() != V:
        raise ValueError(f'slotformer_amd.phyre_planning: {V} videos, {labels.numel()} labels')
    sel = list(readout.sel_slots) if sel is None else [int(s) for s in sel]
    if len(sel) != readout.T or any(s < -1 or s >= T_all for s in sel):
        raise IndexError(f'slotformer_amd.phyre_planning: frame table {sel} ({readout.T} entries of -1 or a frame number) on slots of {T_all} frames')
    sched = batch_schedule(V, epochs, batch_size, seed)   # (raises for batch_size < 1; its indices are a permutation of range(V): in range)
    total = sum(len(e) for e in sched)
    if not (slots.is_cuda and readout.CLS.is_cuda):   # (what the host can check comes first, so that it is checked without a device too)
        raise RuntimeError('slotformer_amd: PHYREReadout trains on a HIP device only; there is no CPU fallback')
    params = phyre_readout_parameters(readout)
    for p in params:
        p.requires_grad_(True)
    opt = FlatAdam(params, lr=lr)
    model, keep = phyre_readout_model(readout)   # (after FlatAdam: the parameters now live in its bucket)
    p_drop = float(readout.transformer_encoder.layers[0].dropout.p)
    pe = phyre_learnable_pe(readout)
    batches = [[idx.to(dev) for idx in e] for e in sched]             # every index tensor goes up before the first step
    targets = [[labels[idx.long()] for idx in e] for e in batches]
    warm = int(round(float(warmup_steps_pct) * total))
    step, losses, ws = 0, [], None
    readout.train()
    with torch.no_grad():
        for e_idx, e_lab in zip(batches, targets):
            epoch_loss = torch.zeros((), dtype=torch.float32, device=dev)
            for idx, lab in zip(e_idx, e_lab):
                s = step_seed(seed, step)
                logits, ws, _, _ = ops.phyre_readout_train_fwd(model, slots, sel, video_index=idx, p=p_drop, seed=s, ws=ws)
                loss, g, _, _ = ops.physion_readout_score(logits, lab)
                ops.phyre_readout_train_bwd(model, slots, sel, g, ws, video_index=idx, p=p_drop, seed=s, learnable_pe=pe, out=opt.grad)
                opt.lr = warmup_cosine_lr(step, total, warm, lr, 0.)
                opt.step(gathered=True)
                step += 1
                epoch_loss += loss[0] * (idx.numel() / V)
            losses.append(epoch_loss)
    del keep
    readout.eval()
    plans.invalidate(readout)
    return torch.stack(losses) if losses else torch.zeros(0, device=dev)


@torch.no_grad()
def evaluate(readout, slots, labels, batch_size=512):
    """calc_eval_loss over a whole set: slots [V, T_all, N, C] and labels [V] on the device -> {'loss', 'acc_0.10', ..., 'acc_0.90'} (floats).
    Every batch is the eval-mode forward and one score launch that adds its hits to int32 counters on the device; the loss sum and the counts
    come back in ONE download at the end."""
    if int(batch_size) < 1:
        raise ValueError(f'slotformer_amd.phyre_planning: batch_size >= 1, got {batch_size!r}')
    V = slots.shape[0]
    if torch.as_tensor(labels).numel() != V:
        raise ValueError(f'slotformer_amd.phyre_planning: {V} videos, {torch.as_tensor(labels).numel()} labels')
    if not (torch.is_tensor(slots) and slots.is_cuda):
        raise RuntimeError('slotformer_amd: PHYREReadout runs on a HIP device only; there is no CPU fallback')
    dev = slots.device
    labels = torch.as_tensor(labels, device=dev).float().flatten()
    was_training = readout.training
    readout.eval()
    counts = None
    loss_sum = torch.zeros(1, dtype=torch.float32, device=dev)
    try:
        for s in range(0, V, int(batch_size)):
            idx = torch.arange(s, min(s + int(batch_size), V), dtype=torch.int32, device=dev)
            logits = readout.logits_of(slots, video_index=idx)[0]
            loss, _, counts, _ = ops.physion_readout_score(logits, labels[s:s + idx.numel()], threshs=ACC_THRESHS, want_grad=False, counts=counts)
            loss_sum += loss * (idx.numel() / V)
    finally:
        readout.train(was_training)
    host = torch.cat([loss_sum, counts[0].float()]).cpu()
    out = {'loss': float(host[0])}
    for i, thresh in enumerate(ACC_THRESHS):
        out[f'acc_{thresh:.2f}'] = float(host[1 + i]) / V
    return out


def frame_table(sel_slots, reference_indexing=True):
    """sel_slots -> for every entry the frame of a rollout buffer [slot0, pred_0, pred_1, ...] the classifier reads, or -1 for a frame of zeros.

    reference_indexing=True: what test_phyre_planning.py really feeds the classifier.  It pads the first frame's slots with zeros to
    vid_len = max(sel_slots) + 1 frames, and SingleStepSlotFormer.forward then classifies cat(gt_slots, pred_slots) -- gt_slots being the
    vid_len - 1 PADDED ZERO frames, pred_slots the vid_len - 1 predictions.  Index s < vid_len - 1 is therefore a frame of zeros and index
    s >= vid_len - 1 is prediction s - (vid_len - 1), i.e. buffer frame s - (vid_len - 1) + 1: sel_slots [0, 3] reads [zeros, pred_0] = [-1, 1].
    reference_indexing=False: the indices into [slot0, predictions] the classifier was trained on (rollout_phyre_slots.py): the table is
    sel_slots itself."""
    sel = [int(s) for s in sel_slots]
    if not sel or min(sel) < 0:
        raise ValueError(f'slotformer_amd.phyre_planning: sel_slots are frame numbers >= 0, got {list(sel_slots)!r}')
    if not reference_indexing:
        return sel
    n_zero = max(sel)   # vid_len - 1
    return [-1 if s < n_zero else s - n_zero + 1 for s in sel]


def auccess_from_ranks(first_rank, actions=None):
    """The host step of AUCCESS in float64: first_rank [tasks] (the 0-based place of the first solved action in a task's ranking; `actions`,
    the length of a task's row, where the task has no solved action) -> {'auccess', 'success_rate' [100], 'first_rank'}.
    success_at[task, k-1] = first_rank < k for k = 1..100 -- also for tasks with fewer than 100 valid actions --, success_rate = its mean over the
    tasks, w_k = log(k+1) - log(k), auccess = 100 sum(w s) / sum(w).  actions (optional): a rank >= actions never succeeds, which matters only
    for rows shorter than 100 actions."""
    ranks = np.asarray(first_rank, dtype=np.int64).reshape(-1)
    if ranks.size == 0:
        raise ValueError('slotformer_amd.phyre_planning: no task to score')
    k = np.arange(1, MAX_ATTEMPTS + 1)
    success_at = ranks[:, None] < k[None, :]
    if actions is not None:
        success_at &= ranks[:, None] < int(actions)
    s = success_at.astype(np.float64).sum(0) / ranks.size
    w = np.log(k + 1.0) - np.log(k.astype(np.float64))
    return {'auccess': float(np.sum(w * s) / np.sum(w) * 100.), 'success_rate': s, 'first_rank': ranks}


@torch.no_grad()
def auccess(conf, status):
    """AUCCESS of conf [tasks, actions] (predicted success confidences) against status [tasks, actions] (INVALID_INPUT 0, NOT_SOLVED -1,
    solved > 0) -> {'auccess', 'success_rate' [100], 'first_rank' [tasks]}.  Tensors or arrays; they are moved to the device, where one
    workgroup per task finds the place of the first solved action among the valid actions ranked by falling confidence
    (`ops.phyre_auccess_ranks`); only that [tasks] vector comes back for the 100-step host part (`auccess_from_ranks`).

    Ties: a solved action wins ties (first_rank counts only the valid actions STRICTLY above the best solved one).  The reference ranks with
    `np.argsort(conf)[::-1]`, which leaves the order of equal confidences unspecified, so on ties its result is one of several; without ties
    the two agree exactly.  Invalid actions are left out, whatever confidence they carry."""
    if not torch.cuda.is_available():
        raise RuntimeError('slotformer_amd: AUCCESS ranks run on a HIP device only; there is no CPU fallback')
    dev = conf.device if torch.is_tensor(conf) and conf.is_cuda else torch.device('cuda', torch.cuda.current_device())
    conf = torch.as_tensor(conf).to(dev, torch.float32)
    status = torch.as_tensor(status).to(dev)
    return auccess_from_ranks(ops.phyre_auccess_ranks(conf, status).cpu().numpy(), actions=conf.shape[1])
