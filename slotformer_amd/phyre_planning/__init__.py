"""slotformer.phyre_planning counterpart: build_model, the frame table the planning driver feeds the classifier with, and AUCCESS
(test_phyre_planning.py: collect_results) from a table of confidences.  Inference and planning only; the driver itself is
`harness.phyre_plan`."""
import numpy as np
import torch

from .models import build_model, PHYREReadout
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
    raise NotImplementedError('the nerv trainer is outside the hot path (SURVEY.md 2.1 row 12); the training kernels of PHYREReadout are not built')


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
