"""Mask post-processing and the metrics of the video-prediction evaluation (reference: vp_utils.py:20-344, called by test_vp.py:68-163).

Every function has the reference's name and signature.  Device float32 / integer tensors go to the HIP library (csrc/vp_metrics.hip); everything
else -- CPU tensors, NumPy arrays, other dtypes -- takes the plain torch / NumPy path below, which needs neither skimage nor torchvision and uses
scipy only where it is importable.  `pred_eval_step_device` is the form to chain behind `harness.extract_and_rollout(decoder=...)`: no
synchronisation, no host round trip, every score of every step as a device tensor.

Two documented differences to the reference: box precision / recall of a frame without a present ground-truth box or without a predicted box is
NaN (the reference divides by zero), and the device `masks_to_boxes` ignores ids >= num_boxes where the reference's one_hot raises."""
import colorsys

import numpy as np
import torch

from slotformer_amd._call import scratch, stream   # (absolute: this file is also loaded under the reference's package name)

FG_THRE = 0.5
# the colours of the slots in visualisations (test_vp.py:137): 16 hues, a golden-ratio walk round the colour circle
PALETTE = [tuple(int(round(255 * c)) for c in colorsys.hsv_to_rgb((0.33 + 0.618034 * i) % 1., 0.85 if i % 2 == 0 else 0.55, 1. if i % 3 else 0.8))
           for i in range(16)]
PALETTE_np = np.array(PALETTE, dtype=np.uint8)
PALETTE_torch = torch.from_numpy(PALETTE_np).float() / 255. * 2. - 1.
NUM_CLASSES = 16   # the decoder's slot limit (engine.savi_decode): what the device kernels count
METRICS = ('mse', 'psnr', 'ssim', 'ari', 'fari', 'miou', 'ap', 'ar')


def postproc_mask(batch_masks):
    """[B,T,N,1,H,W] soft masks -> int64 [B,T,H,W]: the slot whose peak score is smallest is the
    background; pixels whose best score is below FG_THRE are assigned to it, everything else is an
    argmax over slots."""
    if batch_masks.is_cuda and batch_masks.dtype == torch.float32 and batch_masks.shape[2] <= 255:
        # device tensors: two launches of the HIP library (per-(frame, slot) maxima, then the rule per pixel); the same comparisons
        import ctypes as C  # noqa: F401
        from .. import _lib
        B, T, N, _, H, W = batch_masks.shape
        mk = batch_masks.detach().contiguous()
        out = torch.empty(B, T, H, W, dtype=torch.int64, device=mk.device)
        maxima = torch.empty(B * T * N, dtype=torch.int32, device=mk.device)
        _lib.check(_lib.lib().sf_postproc_mask_f32(mk.data_ptr(), out.data_ptr(), None, float(FG_THRE), maxima.data_ptr(), B * T, N, H * W,
                                                   stream(mk)))
        return out
    m = batch_masks.clone()
    B, T, N, _, H, W = m.shape
    m = m.reshape(B * T, N, H * W)
    bg_idx = m.max(-1)[0].argmin(-1)
    weak = m.max(1)[0] < FG_THRE
    is_bg = torch.zeros(B * T, N, dtype=torch.bool, device=m.device)
    is_bg[torch.arange(B * T, device=m.device), bg_idx] = True
    m[is_bg.unsqueeze(-1) & weak.unsqueeze(1)] = 1.
    return m.argmax(1).reshape(B, T, H, W)


# ---- the library calls -------------------------------------------------------------------------------------------------------------------------

def _lib():
    from slotformer_amd import _lib as L
    return L


def _is_dev_f32(*ts):
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in ts)


def _is_dev_ids(*ts):
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype in (torch.int64, torch.uint8) for t in ts)


def _ws(dev, F, H, W, slot='vp'):
    from slotformer_amd import engine
    return engine.workspace_for(dev, (slot, ), _lib().lib().sf_vp_metrics_workspace_bytes, F, H, W, at_least=256)


def _dev_image_scores(x, y, to_rgb):
    """x, y [F,3,H,W] device float32 -> (mse, psnr, ssim) [3,F] float64 on the device."""
    L = _lib()
    x, y = x.contiguous(), y.contiguous()
    F, _, H, W = x.shape
    out = torch.empty(3, F, dtype=torch.float64, device=x.device)
    ws = _ws(x.device, F, H, W)
    L.check(L.lib().sf_vp_image_metrics_f32(x.data_ptr(), y.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), F, H, W,
                                            int(to_rgb), ws.data_ptr(), ws.numel(), stream(x)))
    return out


def _dev_mask_scores(gt, pm, H, W):
    """gt [F,H*W] int64, pm [F,H*W] int64 / uint8 on the device -> (ari, fari, miou) [3,F] float64, the flag word [1] int32, tables [F,16,16] int32."""
    L = _lib()
    gt, pm = gt.contiguous(), pm.contiguous()
    if gt.dtype != torch.int64:
        gt = gt.long()
    F = gt.shape[0]
    out = torch.empty(3, F, dtype=torch.float64, device=gt.device)
    flag = torch.empty(1, dtype=torch.int32, device=gt.device)
    tables = torch.empty(F, NUM_CLASSES, NUM_CLASSES, dtype=torch.int32, device=gt.device)
    L.check(L.lib().sf_vp_mask_metrics(gt.data_ptr(), pm.data_ptr(), int(pm.dtype == torch.uint8), tables.data_ptr(), None, out[0].data_ptr(),
                                       out[1].data_ptr(), out[2].data_ptr(), flag.data_ptr(), F, H, W, NUM_CLASSES, None, 0, stream(gt)))
    return out, flag, tables


def _dev_bbox_scores(pres, gtb, pb, ovthresh=0.5):
    """pres [F,N] bool, gtb [F,N,4], pb [F,M,4] on the device -> (precision, recall) [2,F] float64."""
    L = _lib()
    pres = (pres if pres.dtype == torch.bool else pres.bool()).contiguous().view(torch.uint8)
    gtb, pb = gtb.float().contiguous(), pb.float().contiguous()
    F, N = pres.shape
    out = torch.empty(2, F, dtype=torch.float64, device=gtb.device)
    L.check(L.lib().sf_vp_bbox_pr_f32(gtb.data_ptr(), pres.data_ptr(), pb.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), F, N, pb.shape[1],
                                      float(ovthresh), stream(gtb)))
    return out


def _dev_boxes(masks, F, H, W, num_boxes):
    L = _lib()
    masks = masks.contiguous()
    boxes = torch.empty(F, num_boxes, 4, dtype=torch.float32, device=masks.device)
    L.check(L.lib().sf_masks_to_boxes(masks.data_ptr(), int(masks.dtype == torch.uint8), boxes.data_ptr(), None, F, H, W, num_boxes, stream(masks)))
    return boxes


# ---- boxes -------------------------------------------------------------------------------------------------------------------------------------

def masks_to_boxes_w_empty_mask(binary_masks):
    """binary_masks [B,H,W] -> [B,4] float [min x, min y, max x, max y] of the nonzero pixels, -1 for an empty mask."""
    B, H, W = binary_masks.shape
    if torch.is_tensor(binary_masks) and binary_masks.is_cuda and binary_masks.dtype in (torch.int64, torch.uint8, torch.bool) and H * W > 0:
        m = binary_masks.view(torch.uint8) if binary_masks.dtype == torch.bool else binary_masks
        if B == 0:
            return torch.empty(0, 4, device=m.device)
        return _dev_boxes(m, B, H, W, 2)[:, 1].contiguous()   # ids 0 / 1: the box of id 1 (other values are ignored)
    m = torch.as_tensor(binary_masks) != 0
    rows, cols = m.any(-1).to(torch.uint8), m.any(-2).to(torch.uint8)   # [B,H], [B,W] (argmax below wants numbers)
    out = torch.full((B, 4), -1., device=m.device)
    has = rows.any(-1).bool()
    x1, x2 = cols.argmax(-1), W - 1 - cols.flip(-1).argmax(-1)
    y1, y2 = rows.argmax(-1), H - 1 - rows.flip(-1).argmax(-1)
    out[has] = torch.stack([x1, y1, x2, y2], -1).float()[has]
    return out


def masks_to_boxes(masks, num_boxes=7):
    """masks [B,T,H,W] ids (after argmax) -> [B,T,num_boxes,4] boxes [x1,y1,x2,y2] of every id, -1 for an id without a pixel."""
    B, T, H, W = masks.shape
    if _is_dev_ids(masks) and num_boxes <= NUM_CLASSES and masks.numel() > 0:
        return _dev_boxes(masks, B * T, H, W, num_boxes).view(B, T, num_boxes, 4)
    masks = torch.as_tensor(masks).long()
    onehot = masks.unsqueeze(2) == torch.arange(num_boxes, device=masks.device).view(1, 1, -1, 1, 1)
    if bool(((masks < 0) | (masks >= num_boxes)).any()):
        raise RuntimeError('masks_to_boxes: an id outside [0, num_boxes)')
    return masks_to_boxes_w_empty_mask(onehot.flatten(0, 2)).reshape(B, T, num_boxes, 4)


# ---- image metrics (inputs already in [0, 1], as pred_eval_step hands them after to_rgb_from_tensor) --------------------------------------------

def _np64(x):
    return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float64)


def mse_metric(x, y):
    """x/y: [B,C,H,W]: squared error summed over H and W, averaged over batch and channels."""
    if _is_dev_f32(x, y) and x.shape[1] == 3 and min(x.shape[2:]) >= 11 and x.shape[0] > 0:
        return _dev_image_scores(x, y, False)[0].mean().item()
    return ((x - y)**2).sum(-1).sum(-1).mean()


def psnr_metric(x, y):
    """x/y: [B,C,H,W]: peak signal-to-noise ratio at data range 1 per sample, averaged."""
    if _is_dev_f32(x, y) and x.shape[1] == 3 and min(x.shape[2:]) >= 11 and x.shape[0] > 0:
        return _dev_image_scores(x, y, False)[1].mean().item()
    x, y = _np64(x), _np64(y)
    with np.errstate(divide='ignore'):
        return np.mean([10. * np.log10(1. / np.mean((x[i] - y[i])**2)) for i in range(x.shape[0])])


def _gauss_taps(sigma=1.5, truncate=3.5):
    r = int(truncate * sigma + 0.5)
    w = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma)**2)
    return w / w.sum(), r


def _gauss_filter(a, w, r):
    """Separable filter over the last two axes with scipy's `reflect` boundary (d c b a | a b c d = NumPy's 'symmetric')."""
    a = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(r, r), (r, r)], mode='symmetric')
    H, W = a.shape[-2] - 2 * r, a.shape[-1] - 2 * r
    a = sum(w[k] * a[..., k:k + H, :] for k in range(2 * r + 1))
    return sum(w[k] * a[..., :, k:k + W] for k in range(2 * r + 1))


def _ssim_planes(x, y, data_range):
    """SSIM of [..., H, W] planes: Gaussian weights sigma 1.5 (11 taps), K1 0.01, K2 0.03, population covariance, the map cropped by the radius."""
    w, r = _gauss_taps()
    C1, C2 = (0.01 * data_range)**2, (0.03 * data_range)**2
    ux, uy = _gauss_filter(x, w, r), _gauss_filter(y, w, r)
    vx = _gauss_filter(x * x, w, r) - ux * ux
    vy = _gauss_filter(y * y, w, r) - uy * uy
    vxy = _gauss_filter(x * y, w, r) - ux * uy
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return S[..., r:-r, r:-r]


def ssim_metric(x, y):
    """x/y: [B,C,H,W]: structural similarity of the x 255 images (Gaussian window, channels averaged) per sample, averaged."""
    if _is_dev_f32(x, y) and x.shape[1] == 3 and min(x.shape[2:]) >= 11 and x.shape[0] > 0:
        return _dev_image_scores(x, y, False)[2].mean().item()
    x, y = _np64(x) * 255., _np64(y) * 255.
    return np.mean([_ssim_planes(x[i], y[i], 255.).mean() for i in range(x.shape[0])])


def perceptual_dist(x, y, loss_fn):
    """x/y: [B,C,H,W]"""
    return loss_fn(x, y).mean()


# ---- mask metrics ------------------------------------------------------------------------------------------------------------------------------

def _contingency(true_ids, pred_ids):
    """[B, P] ids -> int64 counts [B, C, K]."""
    t, p = torch.as_tensor(true_ids).long().cpu(), torch.as_tensor(pred_ids).long().cpu()
    C, K = int(t.max()) + 1 if t.numel() else 1, int(p.max()) + 1 if p.numel() else 1
    B = t.shape[0]
    flat = (torch.arange(B).view(B, 1) * C + t) * K + p
    return torch.bincount(flat.reshape(-1), minlength=B * C * K).view(B, C, K)


def _ari_from_table(N):
    """adjusted Rand index of float64 count tables [B, C, K]; 1 where the denominator is 0."""
    A, Bs = N.sum(-1), N.sum(-2)
    npts = A.sum(-1)
    rindex = (N * (N - 1)).sum((-1, -2))
    aindex, bindex = (A * (A - 1)).sum(-1), (Bs * (Bs - 1)).sum(-1)
    expected = aindex * bindex / torch.clamp(npts * (npts - 1), min=1)
    den = (aindex + bindex) / 2 - expected
    return torch.where(den != 0, (rindex - expected) / torch.where(den != 0, den, torch.ones_like(den)), torch.ones_like(den))


def adjusted_rand_index(true_ids, pred_ids, ignore_background=False):
    """true_ids / pred_ids [B,T,H,W] (or [B,H,W]) integer ids -> the adjusted Rand index of the two clusterings of each batch entry's pixels,
    [B]; ignore_background leaves out the pixels whose true id is 0.  1 where the denominator is 0.  Counted in integers and evaluated in float64
    (the reference evaluates in float32 on counts up to 2.7e8 and returns float32)."""
    if true_ids.dim() == 3:
        true_ids = true_ids.unsqueeze(1)
    if pred_ids.dim() == 3:
        pred_ids = pred_ids.unsqueeze(1)
    B, T, H, W = true_ids.shape
    if _is_dev_ids(pred_ids) and true_ids.is_cuda and true_ids.dtype == torch.int64 and true_ids.numel() > 0:
        out, flag, _ = _dev_mask_scores(true_ids.reshape(B, -1), pred_ids.reshape(B, -1), T * H, W)   # a video as one tall frame
        if int(flag.item()) == 0:   # (ids of 16 and above: the host path counts them)
            return out[1 if ignore_background else 0]
    N = _contingency(true_ids.reshape(B, -1), pred_ids.reshape(B, -1)).double()
    if ignore_background:
        N = N[:, 1:]
    return _ari_from_table(N).to(true_ids.device)


def ARI_metric(x, y):
    """x/y: [B,H,W], both are seg_masks after argmax."""
    assert 'int' in str(x.dtype)
    assert 'int' in str(y.dtype)
    return adjusted_rand_index(x, y).mean().item()


def fARI_metric(x, y):
    """x/y: [B,H,W], both are seg_masks after argmax."""
    assert 'int' in str(x.dtype)
    assert 'int' in str(y.dtype)
    return adjusted_rand_index(x, y, ignore_background=True).mean().item()


def _max_assignment(w):
    """Largest total of an assignment of the rows of w [n, m] (n <= m) to distinct columns: (total, columns)."""
    n, m = w.shape
    try:
        from scipy.optimize import linear_sum_assignment
        r, c = linear_sum_assignment(w, maximize=True)
        return float(w[r, c].sum()), c
    except ImportError:
        pass
    # the Hungarian method with potentials on the costs -w (rows and columns counted from 1; match[j] = the row of column j)
    INF = float('inf')
    u, v, match, way = [0.] * (n + 1), [0.] * (m + 1), [0] * (m + 1), [0] * (m + 1)
    for i in range(1, n + 1):
        match[0], j0 = i, 0
        minv, used = [INF] * (m + 1), [False] * (m + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = match[j0], INF, 0
            for j in range(1, m + 1):
                if not used[j]:
                    cur = -w[i0 - 1, j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(m + 1):
                if used[j]:
                    u[match[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if match[j0] == 0:
                break
        while j0:
            match[j0] = match[way[j0]]
            j0 = way[j0]
    cols = np.zeros(n, dtype=np.int64)
    for j in range(1, m + 1):
        if match[j]:
            cols[match[j] - 1] = j - 1
    return float(sum(w[i, cols[i]] for i in range(n))), cols


def _miou_from_table(N):
    """float64 counts [C, K] (row 0 = background) -> the Hungarian mIoU over the foreground rows 1 .. C-1; NaN without one."""
    present = np.nonzero(N.sum(1) > 0)[0]
    n = int(present.max()) if len(present) else 0   # the width of the reference's one_hot of THIS frame, less the background
    if n == 0:
        return float('nan')
    fg = N[1:n + 1]
    iou = fg / ((fg.sum(1, keepdims=True) + N.sum(0, keepdims=True) - fg) + 1e-8)
    if iou.shape[1] < n:   # fewer predicted ids than objects: the unmatched objects score 0
        iou = np.concatenate([iou, np.zeros((n, n - iou.shape[1]))], 1)
    return _max_assignment(iou)[0] / n


def hungarian_miou(gt_mask, pred_mask):
    """both mask: [H*W] after argmax, 0 is gt background index: the best one-to-one matching of the ground-truth objects 1 .. N (N = the largest
    id present) to predicted ids by IoU, its total divided by N."""
    if _is_dev_ids(pred_mask) and gt_mask.is_cuda and gt_mask.dtype == torch.int64 and gt_mask.numel() > 0:
        out, flag, _ = _dev_mask_scores(gt_mask.view(1, -1), pred_mask.view(1, -1), 1, gt_mask.numel())
        if int(flag.item()) == 0:
            return out[2, 0].item()
    return _miou_from_table(_contingency(gt_mask.reshape(1, -1), pred_mask.reshape(1, -1))[0].double().numpy())


def miou_metric(gt_mask, pred_mask):
    """both mask: [B,H,W], both are seg_masks after argmax."""
    assert 'int' in str(gt_mask.dtype)
    assert 'int' in str(pred_mask.dtype)
    B, H, W = gt_mask.shape
    if _is_dev_ids(pred_mask) and gt_mask.is_cuda and gt_mask.dtype == torch.int64 and gt_mask.numel() > 0:
        out, flag, _ = _dev_mask_scores(gt_mask.reshape(B, -1), pred_mask.reshape(B, -1), H, W)
        if int(flag.item()) == 0:
            return out[2].mean().item()
    tabs = _contingency(gt_mask.reshape(B, -1), pred_mask.reshape(B, -1)).double().numpy()
    return np.mean([_miou_from_table(tabs[i]) for i in range(B)])


# ---- box metrics -------------------------------------------------------------------------------------------------------------------------------

def bbox_precision_recall(gt_pres_mask, gt_bbox, pred_bbox, ovthresh=0.5):
    """gt_pres_mask [N] bool, gt_bbox [N,4], pred_bbox [M,4]: every present ground-truth box, in order, takes the predicted box (x1 >= 0) of
    largest IoU -- the first on ties -- and is a true positive when that IoU reaches ovthresh and the box is still free.  Returns
    (tp / predicted boxes, tp / present boxes); (nan, nan) when either count is 0."""
    if _is_dev_f32(gt_bbox, pred_bbox) and gt_pres_mask.is_cuda and 1 <= gt_bbox.shape[0] <= 64 and 1 <= pred_bbox.shape[0] <= 64:
        out = _dev_bbox_scores(gt_pres_mask.view(1, -1), gt_bbox.unsqueeze(0), pred_bbox.unsqueeze(0), ovthresh).cpu()
        return out[0, 0].item(), out[1, 0].item()
    g = torch.as_tensor(gt_bbox).detach().double().cpu()[torch.as_tensor(gt_pres_mask).bool().cpu()]
    p = torch.as_tensor(pred_bbox).detach().double().cpu()
    p = p[p[:, 0] >= 0.]
    N, M = g.shape[0], p.shape[0]
    if N == 0 or M == 0:
        return float('nan'), float('nan')
    wh = (torch.min(g[:, None, 2:], p[None, :, 2:]) - torch.max(g[:, None, :2], p[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area_g, area_p = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]), (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    iou = inter / (area_g[:, None] + area_p[None, :] - inter)
    tp, used = 0, [False] * M
    for i in range(N):
        j = int(iou[i].argmax())
        if iou[i, j].item() >= ovthresh and not used[j]:
            tp += 1
            used[j] = True
    return tp / float(M), tp / float(N)


def batch_bbox_precision_recall(gt_pres_mask, gt_bbox, pred_bbox):
    """bbox_precision_recall over a batch ([B,N], [B,N,4], [B,M,4]), averaged."""
    if _is_dev_f32(gt_bbox, pred_bbox) and gt_pres_mask.is_cuda and gt_bbox.shape[0] > 0 and 1 <= gt_bbox.shape[1] <= 64 and \
            1 <= pred_bbox.shape[1] <= 64:
        out = _dev_bbox_scores(gt_pres_mask, gt_bbox, pred_bbox).mean(1).cpu()
        return out[0].item(), out[1].item()
    prs = [bbox_precision_recall(gt_pres_mask[i], gt_bbox[i], pred_bbox[i]) for i in range(gt_pres_mask.shape[0])]
    return np.mean([a for a, _ in prs]), np.mean([r for _, r in prs])


# ---- the evaluation step -----------------------------------------------------------------------------------------------------------------------

_STEP_BUFFERS = {}


def _device_step_ok(gt, pred, gt_mask, pred_mask, gt_pres_mask, gt_bbox, pred_bbox, eval_traj):
    if not (_is_dev_f32(gt, pred) and gt.dim() == 5 and gt.shape[2] == 3 and min(gt.shape[3:]) >= 11 and gt.shape[0] > 0 and gt.shape[1] > 0):
        return False
    if not eval_traj:
        return True
    return (_is_dev_ids(pred_mask) and torch.is_tensor(gt_mask) and gt_mask.is_cuda and gt_mask.dtype == torch.int64 and
            _is_dev_f32(gt_bbox, pred_bbox) and torch.is_tensor(gt_pres_mask) and gt_pres_mask.is_cuda and
            1 <= gt_bbox.shape[2] <= 64 and 1 <= pred_bbox.shape[2] <= 64)


def _is_device_lpips(fn):
    from slotformer_amd.lpips import LPIPS
    return isinstance(fn, LPIPS)


def _step_on_device(gt, pred, gt_mask, pred_mask, gt_pres_mask, gt_bbox, pred_bbox, eval_traj, lpips=None):
    """The launches of pred_eval_step_device; returns the shape's buffers.  With `lpips` (slotformer_amd.lpips.LPIPS) the buffers of the shape
    carry the perceptual distance as well: its per-step means [T] behind the flag word (inside 'head', so they ride in the same download), its
    per-video scores [B,T] and the float32 scores of the B * T pairs at the end; everything before them lies where it lies without."""
    assert gt.shape == pred.shape
    L = _lib()
    lib = L.lib()
    B, T, _, H, W = gt.shape
    F = B * T
    dev = gt.device
    key = (dev.index, B, T, H, W, bool(eval_traj)) + (('lpips', ) if lpips is not None else ())
    buf = _STEP_BUFFERS.get(key)
    if buf is None:
        K = len(METRICS)
        P = T if lpips is not None else 0   # doubles of the perceptual distance's means, behind the flag word
        # one allocation: the means [K,T] and the flag word lie together (pred_eval_step downloads them in one copy), the per-video scores behind
        raw = torch.zeros((K * T + 1 + P + K * F) * 8 + (F * 12 if lpips is not None else 0), dtype=torch.uint8, device=dev)
        head = raw[:(K * T + 1 + P) * 8]
        buf = {'raw': raw, 'head': head, 'mean': head[:K * T * 8].view(torch.float64).view(K, T),
               'flag': head[K * T * 8:(K * T + 1) * 8].view(torch.int32)[:1],
               'per': raw[(K * T + 1 + P) * 8:(K * T + 1 + P + K * F) * 8].view(torch.float64).view(K, B, T),
               'ws': scratch(lib.sf_vp_metrics_workspace_bytes, F, H, W, device=dev, at_least=256)}
        if lpips is not None:
            tail = raw[(K * T + 1 + P + K * F) * 8:]
            buf['lp_mean'] = head[(K * T + 1) * 8:].view(torch.float64)
            buf['lp_per'] = tail[:F * 8].view(torch.float64).view(B, T)
            buf['lp_scores'] = tail[F * 8:].view(torch.float32)
        _STEP_BUFFERS[key] = buf
    per, ws, st = buf['per'], buf['ws'], stream(gt)
    gt, pred = gt.contiguous(), pred.contiguous()
    L.check(lib.sf_vp_image_metrics_f32(gt.data_ptr(), pred.data_ptr(), per[0].data_ptr(), per[1].data_ptr(), per[2].data_ptr(), F, H, W, 1,
                                        ws.data_ptr(), ws.numel(), st))
    if eval_traj:
        assert gt_mask.shape == pred_mask.shape == (B, T, H, W) and gt_pres_mask.dim() == 3 and gt_bbox.dim() == pred_bbox.dim() == 4
        gm, pm = gt_mask.contiguous(), pred_mask.contiguous()
        L.check(lib.sf_vp_mask_metrics(gm.data_ptr(), pm.data_ptr(), int(pm.dtype == torch.uint8), None, None, per[3].data_ptr(), per[4].data_ptr(),
                                       per[5].data_ptr(), buf['flag'].data_ptr(), F, H, W, NUM_CLASSES, ws.data_ptr(), ws.numel(), st))
        pres = (gt_pres_mask if gt_pres_mask.dtype == torch.bool else gt_pres_mask.bool()).contiguous().view(torch.uint8)
        gb, pb = gt_bbox.contiguous(), pred_bbox.contiguous()
        L.check(lib.sf_vp_bbox_pr_f32(gb.data_ptr(), pres.data_ptr(), pb.data_ptr(), per[6].data_ptr(), per[7].data_ptr(), F, gb.shape[2], pb.shape[2],
                                      0.5, st))
    L.check(lib.sf_vp_mean_over_videos_f64(per.data_ptr(), buf['mean'].data_ptr(), len(METRICS), B, T, st))
    if lpips is not None:
        lpips.distances(gt.view(F, 3, H, W), pred.view(F, 3, H, W), out=buf['lp_scores'])
        L.check(lib.sf_lpips_mean_over_videos_f32(buf['lp_scores'].data_ptr(), buf['lp_per'].data_ptr(), buf['lp_mean'].data_ptr(), B, T, st))
    return buf


@torch.no_grad()
def pred_eval_step_device(gt, pred, gt_mask=None, pred_mask=None, gt_pres_mask=None, gt_bbox=None, pred_bbox=None, eval_traj=True, lpips=None):
    """pred_eval_step without its host half: gt / pred [B,T,3,H,W] device float32 in [-1, 1] (e.g. the `recon` of
    `harness.extract_and_rollout(decoder=...)`), gt_mask [B,T,H,W] int64, pred_mask [B,T,H,W] int64 or uint8 (its `seg`), gt_pres_mask [B,T,N]
    bool, gt_bbox [B,T,N,4], pred_bbox [B,T,M,4] float32.  Returns float64 device tensors: 'mse', 'psnr', 'ssim', 'ari', 'fari', 'miou', 'ap', 'ar'
    [T] (the mean over the videos of every step) and '<name>_per_video' [B,T]; 'id_out_of_range' [1] int32 is nonzero when a mask id lay outside
    [0, 16) (such pixels are left out).  With eval_traj=False the five trajectory scores are zeros.

    Six launches on torch's current stream, whatever B and T; no synchronisation and no host round trip, so the call can be captured into a graph.
    The result tensors and the workspace are kept per shape: nothing is allocated after the first call of a shape, and the next call of that shape
    overwrites them (copy what must outlive it).

    lpips: a `slotformer_amd.lpips.LPIPS` on the frames' device (H, W >= 16).  The result then has 'percept_dist' [T] and 'percept_dist_per_video'
    [B,T] as well -- the perceptual distance of the B * T pairs from one batched pass through the network, chunked by the module's `chunk` -- at
    the price of its launches (about twenty per chunk)."""
    if lpips is not None and not (_is_device_lpips(lpips) and torch.is_tensor(gt) and gt.dim() == 5 and min(gt.shape[3:]) >= 16):
        raise RuntimeError('pred_eval_step_device: lpips= takes a slotformer_amd.lpips.LPIPS and frames of at least 16 x 16')
    if not _device_step_ok(gt, pred, gt_mask, pred_mask, gt_pres_mask, gt_bbox, pred_bbox, eval_traj):
        raise RuntimeError('pred_eval_step_device: device float32 frames [B,T,3,H,W] with H, W >= 11 (and, with eval_traj, device int64 / uint8 masks, '
                           'bool presence and float32 boxes, at most 64 per frame) are required; pred_eval_step takes everything else')
    buf = _step_on_device(gt, pred, gt_mask, pred_mask, gt_pres_mask, gt_bbox, pred_bbox, eval_traj, lpips)
    out = {m: buf['mean'][i] for i, m in enumerate(METRICS)}
    out.update({m + '_per_video': buf['per'][i] for i, m in enumerate(METRICS)})
    if lpips is not None:
        out['percept_dist'], out['percept_dist_per_video'] = buf['lp_mean'], buf['lp_per']
    out['id_out_of_range'] = buf['flag']
    return out


@torch.no_grad()
def pred_eval_step(gt, pred, lpips_fn, gt_mask=None, pred_mask=None, gt_pres_mask=None, gt_bbox=None, pred_bbox=None, eval_traj=True):
    """gt / pred [B,T,C,H,W] in [-1, 1]; masks [B,T,H,W]; gt_pres_mask [B,T,N]; boxes [B,T,N/M,4].  Every metric for every time step: a dict of
    nine lists of T Python floats ('mse', 'ssim', 'psnr', 'percept_dist', 'ari', 'fari', 'miou', 'ap', 'ar').  'percept_dist' is lpips_fn applied per
    step, 0.0 without one; eval_traj=False gives zeros for the mask and box metrics.  Device inputs are scored by the library with ONE download at
    the end; a mask id outside [0, 16) raises there.  When lpips_fn is a `slotformer_amd.lpips.LPIPS` and the frames are device float32 of at
    least 16 x 16, 'percept_dist' of all T steps comes from one batched call over the B * T pairs, its per-step means are taken on the device and
    ride in that one download; any other callable is applied per step as before."""
    assert len(gt.shape) == len(pred.shape) == 5
    assert gt.shape == pred.shape
    assert gt.shape[2] == 3
    if eval_traj:
        assert len(gt_mask.shape) == len(pred_mask.shape) == 4
        assert gt_mask.shape == pred_mask.shape
        assert len(gt_pres_mask.shape) == 3
        assert len(gt_bbox.shape) == len(pred_bbox.shape) == 4
    T = gt.shape[1]
    on_device = _device_step_ok(gt, pred, gt_mask, pred_mask, gt_pres_mask, gt_bbox, pred_bbox, eval_traj)
    fused = on_device and lpips_fn is not None and _is_device_lpips(lpips_fn) and min(gt.shape[3:]) >= 16
    percept = None if fused else [0. if lpips_fn is None else float(perceptual_dist(gt[:, t], pred[:, t], lpips_fn)) for t in range(T)]
    if on_device:
        # the one copy: [8,T] means + the flag word (+ the [T] means of the perceptual distance)
        head = _step_on_device(gt, pred, gt_mask, pred_mask, gt_pres_mask, gt_bbox, pred_bbox, eval_traj, lpips_fn if fused else None)['head'].cpu()
        nm = len(METRICS) * T * 8
        if int(head[nm:nm + 8].view(torch.int32)[0]):
            raise RuntimeError('pred_eval_step: a mask id outside [0, 16)')
        mean = head[:nm].view(torch.float64).view(len(METRICS), T)
        out = {m: [float(v) for v in mean[i]] for i, m in enumerate(METRICS)}
        out['percept_dist'] = [float(v) for v in head[nm + 8:].view(torch.float64)] if fused else percept
        return out
    out = {m: [] for m in METRICS}
    out['percept_dist'] = percept
    from slotformer_amd.base_slots.models import to_rgb_from_tensor
    rgb_gt, rgb_pred = to_rgb_from_tensor(gt).cpu().numpy(), to_rgb_from_tensor(pred).cpu().numpy()
    for t in range(T):
        if eval_traj:
            out['ari'].append(float(ARI_metric(gt_mask[:, t], pred_mask[:, t])))
            out['fari'].append(float(fARI_metric(gt_mask[:, t], pred_mask[:, t])))
            out['miou'].append(float(miou_metric(gt_mask[:, t], pred_mask[:, t])))
            ap, ar = batch_bbox_precision_recall(gt_pres_mask[:, t], gt_bbox[:, t], pred_bbox[:, t])
            out['ap'].append(float(ap))
            out['ar'].append(float(ar))
        else:
            for m in ('ari', 'fari', 'miou', 'ap', 'ar'):
                out[m].append(0.)
        out['mse'].append(float(mse_metric(rgb_gt[:, t], rgb_pred[:, t])))
        out['psnr'].append(float(psnr_metric(rgb_gt[:, t], rgb_pred[:, t])))
        out['ssim'].append(float(ssim_metric(rgb_gt[:, t], rgb_pred[:, t])))
    return out
