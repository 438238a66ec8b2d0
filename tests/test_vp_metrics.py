"""CPU: the video-prediction metrics of slotformer_amd/video_prediction/vp_utils.py (reference vp_utils.py:44-344) -- the host path of every public
function against float64 restatements written here, against the reference's own results on seeded blob masks (tests/golden/vp_metrics.npz,
tools/gen_golden_vp_metrics.py), the argument errors of the new entry points, and the drop-in import.  The restatements and input generators
are shared with tests/test_vp_metrics_gpu.py."""
import itertools

import numpy as np
import pytest
import torch

import golden_util as gu

NCLS = 16


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------------

def blob_masks(rs, F, H, W, n_obj, n_pred, gt_ids=None, permute=True):
    """Ground truth: n_obj discs (ids 1 .. n_obj, or gt_ids) on background 0, every one with at least one visible pixel.  Prediction: the same
    discs shifted and resized a little, relabelled through a random injection into n_pred classes (objects beyond n_pred - 1 merge into others).
    Returns int64 [F,H,W] x 2."""
    gt_ids = list(range(1, n_obj + 1)) if gt_ids is None else list(gt_ids)
    yy, xx = np.mgrid[0:H, 0:W]
    gt, pm = np.zeros((F, H, W), np.int64), np.zeros((F, H, W), np.int64)
    for f in range(F):
        while True:
            g, p = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
            labels = rs.permutation(n_pred) if permute else np.arange(n_pred)
            for k, gid in enumerate(gt_ids):
                cy, cx, r = rs.uniform(2, H - 2), rs.uniform(2, W - 2), rs.uniform(0.06, 0.16) * min(H, W) + 1.5
                g[(yy - cy)**2 + (xx - cx)**2 <= r * r] = gid
                dy, dx, dr = rs.uniform(-1.5, 1.5), rs.uniform(-1.5, 1.5), rs.uniform(-1., 1.)
                p[(yy - cy - dy)**2 + (xx - cx - dx)**2 <= (r + dr)**2] = labels[(k + 1) % n_pred]
            p[p == 0] = labels[0]
            if all((g == gid).any() for gid in gt_ids):
                break
        gt[f], pm[f] = g, p
    return gt, pm


def smooth_frames(rs, F, H, W, noise=0.1):
    """gt: smooth random colour fields + texture, reaching a little outside [-1, 1] (so the clamp of to_rgb acts); pred = gt + noise.  float32 [F,3,H,W]."""
    yy, xx = np.mgrid[0:H, 0:W] / float(max(H, W))
    gt = np.zeros((F, 3, H, W))
    for f in range(F):
        for c in range(3):
            a = rs.uniform(-1, 1, 6)
            gt[f, c] = 0.6 * np.sin(6 * a[0] * yy + 5 * a[1] * xx + 3 * a[2]) + 0.5 * a[3] + 0.25 * rs.standard_normal((H, W)) * abs(a[4])
    pred = gt + noise * rs.standard_normal(gt.shape)
    return gt.astype(np.float32), pred.astype(np.float32)


def boxes_of(mask, nb):
    """masks_to_boxes restated: int mask [H,W] -> float32 [nb,4]."""
    out = -np.ones((nb, 4), np.float32)
    for k in range(nb):
        ys, xs = np.nonzero(mask == k)
        if len(ys):
            out[k] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


# ---- float64 restatements ----------------------------------------------------------------------------------------------------------------------

def gauss_taps(dtype=np.float64):
    w = np.exp(-0.5 * (np.arange(-5, 6) / 1.5)**2)
    return (w / w.sum()).astype(dtype)


def image_scores(gt, pred, dtype=np.float64, direct=False):
    """MSE / PSNR / SSIM per frame of [F,3,H,W] frames in [-1, 1], every step in `dtype`: the to_rgb map, the separable 11-tap Gaussian (the five
    quantities x, y, xx, yy, xy; along x, then along y) on the reflect-padded planes, SSIM at data range 1, crop 5.  direct: the 11 x 11 window
    applied in one go instead.  With dtype float32 this is what float32 itself costs the algorithm."""
    dt = dtype
    half, one, zero = dt(0.5), dt(1), dt(0)
    x = np.clip(gt.astype(dt) * half + half, zero, one)
    y = np.clip(pred.astype(dt) * half + half, zero, one)
    F, _, H, W = x.shape
    d = x - y
    sse = (d * d).reshape(F, -1).sum(1, dtype=dt)
    mse = sse / dt(3)
    with np.errstate(divide='ignore'):
        psnr = dt(10) * np.log10(one / (sse / dt(3 * H * W)))
    w = gauss_taps(dt)

    def filt(a):
        a = np.pad(a, [(0, 0), (0, 0), (5, 5), (5, 5)], mode='symmetric')
        if direct:
            out = np.zeros((F, 3, H, W), dt)
            for i in range(11):
                for j in range(11):
                    out += (w[i] * w[j]) * a[:, :, i:i + H, j:j + W]
            return out
        h = np.zeros((F, 3, H + 10, W), dt)
        for k in range(11):
            h += w[k] * a[:, :, :, k:k + W]
        v = np.zeros((F, 3, H, W), dt)
        for k in range(11):
            v += w[k] * h[:, :, k:k + H, :]
        return v

    C1, C2 = dt(0.01)**2, dt(0.03)**2
    ux, uy = filt(x), filt(y)
    vx, vy, vxy = filt(x * x) - ux * ux, filt(y * y) - uy * uy, filt(x * y) - ux * uy
    S = ((dt(2) * ux * uy + C1) * (dt(2) * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    ssim = S[:, :, 5:-5, 5:-5].reshape(F, -1).mean(1, dtype=dt)
    return mse.astype(np.float64), psnr.astype(np.float64), ssim.astype(np.float64)


def table_of(g, p):
    """16 x 16 integer contingency table of two id arrays (ids outside [0, 16) left out)."""
    g, p = np.asarray(g).reshape(-1).astype(np.int64), np.asarray(p).reshape(-1).astype(np.int64)
    ok = (g >= 0) & (g < NCLS) & (p >= 0) & (p < NCLS)
    return np.bincount(g[ok] * NCLS + p[ok], minlength=NCLS * NCLS).reshape(NCLS, NCLS)


def ari_of(table, fg=False):
    N = table[1:].astype(np.float64) if fg else table.astype(np.float64)
    A, B = N.sum(1), N.sum(0)
    n = A.sum()
    rindex, aindex, bindex = (N * (N - 1)).sum(), (A * (A - 1)).sum(), (B * (B - 1)).sum()
    expected = aindex * bindex / max(n * (n - 1), 1.)
    den = (aindex + bindex) / 2 - expected
    return (rindex - expected) / den if den != 0 else 1.


def best_assignment(w):
    """Largest total of an assignment of the rows of w to distinct columns, exactly: by exhaustive permutation up to 7 x 7, else by a dynamic
    programme over column subsets."""
    n, m = w.shape
    if n <= 7 and m <= 7:
        if n > m:
            w, n, m = w.T, m, n
        return max(sum(w[i, c[i]] for i in range(n)) for c in itertools.permutations(range(m), n))
    if n > m:
        w, n, m = w.T, m, n
    masks = np.arange(1 << m)
    pop = np.array([bin(k).count('1') for k in range(1 << m)])
    dp = np.full(1 << m, -np.inf)
    dp[0] = 0.
    for i in range(n):
        new = np.full(1 << m, -np.inf)
        src = masks[pop == i]
        for j in range(m):
            s = src[(src >> j) & 1 == 0]
            new[s | (1 << j)] = np.maximum(new[s | (1 << j)], dp[s] + w[i, j])   # (distinct s give distinct targets)
        dp = new
    return dp[pop == n].max()


def miou_of(table):
    t = table.astype(np.float64)
    present = np.nonzero(t.sum(1) > 0)[0]
    N = int(present.max()) if len(present) else 0
    if N == 0:
        return float('nan')
    fg = t[1:N + 1]
    iou = fg / ((fg.sum(1, keepdims=True) + t.sum(0, keepdims=True) - fg) + 1e-8)
    iou = iou[:, t.sum(0) > 0]   # an absent predicted id is a zero column: worth what no match is worth
    if iou.shape[1] < N:
        iou = np.concatenate([iou, np.zeros((N, N - iou.shape[1]))], 1)
    return best_assignment(iou) / N


def pr_of(pres, gtb, pb, thr=0.5):
    g = [b for b, k in zip(np.asarray(gtb, np.float64), np.asarray(pres)) if k]
    p = [b for b in np.asarray(pb, np.float64) if b[0] >= 0]
    if not g or not p:
        return float('nan'), float('nan')
    used, tp = set(), 0
    for a in g:
        best, bj = -1., -1
        for j, b in enumerate(p):
            iw, ih = max(min(a[2], b[2]) - max(a[0], b[0]), 0.), max(min(a[3], b[3]) - max(a[1], b[1]), 0.)
            inter = iw * ih
            with np.errstate(invalid='ignore', divide='ignore'):
                v = np.float64(inter) / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)
            if np.isnan(v):   # two empty boxes: the first NaN is the row's maximum (torch.argmax) and never reaches the threshold
                best, bj = -1., j
                break
            if v > best:
                best, bj = v, j
        if best >= thr and bj not in used:
            tp += 1
            used.add(bj)
    return tp / len(p), tp / len(g)


def mask_case(seed, F, H, W, n_obj, n_pred, **kw):
    """Blob masks + the boxes test_vp.py would hand over: ground-truth boxes of ids 1 .. n_obj (all present, plus one absent row), predicted boxes
    of all n_pred classes.  Every frame has a foreground object, a present box and a predicted box."""
    rs = np.random.RandomState(seed)
    gt, pm = blob_masks(rs, F, H, W, n_obj, n_pred, **kw)
    ids = kw.get('gt_ids') or list(range(1, n_obj + 1))
    gtb = np.stack([np.concatenate([boxes_of(gt[f], NCLS)[ids], -np.ones((1, 4), np.float32)]) for f in range(F)])
    pres = np.concatenate([np.ones((F, len(ids)), bool), np.zeros((F, 1), bool)], 1)
    pb = np.stack([boxes_of(pm[f], n_pred) for f in range(F)])
    return gt, pm, pres, gtb, pb


def mask_scores(gt, pm, pres, gtb, pb):
    F = gt.shape[0]
    tabs = [table_of(gt[f], pm[f]) for f in range(F)]
    pr = [pr_of(pres[f], gtb[f], pb[f]) for f in range(F)]
    return {'ari': np.array([ari_of(t) for t in tabs]), 'fari': np.array([ari_of(t, True) for t in tabs]),
            'miou': np.array([miou_of(t) for t in tabs]), 'ap': np.array([a for a, _ in pr]), 'ar': np.array([r for _, r in pr])}


# ---- tests -------------------------------------------------------------------------------------------------------------------------------------

def test_alias_exposes_what_test_vp_imports():
    import slotformer.video_prediction.vp_utils as v
    for name in ('pred_eval_step', 'postproc_mask', 'masks_to_boxes', 'PALETTE_torch', 'masks_to_boxes_w_empty_mask', 'mse_metric', 'psnr_metric',
                 'ssim_metric', 'adjusted_rand_index', 'ARI_metric', 'fARI_metric', 'hungarian_miou', 'miou_metric', 'bbox_precision_recall',
                 'batch_bbox_precision_recall', 'perceptual_dist', 'pred_eval_step_device', 'FG_THRE'):
        assert hasattr(v, name), name
    assert v.PALETTE_torch.shape[1] == 3 and v.PALETTE_torch.shape[0] >= 13 and float(v.PALETTE_torch.abs().max()) <= 1.


def test_restatements_agree_with_each_other():
    """The separable and the direct 11 x 11 form of the SSIM restatement; permutation and subset programme of the assignment."""
    rs = np.random.RandomState(3)
    gt, pred = smooth_frames(rs, 2, 23, 31)
    a, b = image_scores(gt, pred), image_scores(gt, pred, direct=True)
    for u, v in zip(a, b):
        assert np.abs(u - v).max() <= 1e-12 * max(1., np.abs(u).max())
    for n, m in ((3, 5), (6, 7), (7, 7)):
        w = rs.rand(n, m)
        big = np.concatenate([w, np.zeros((n, 2))], 1)   # 9 columns: the subset programme
        assert abs(best_assignment(w) - best_assignment(big)) <= 1e-12


def test_ssim_restatement_against_scipy():
    ndi = pytest.importorskip('scipy.ndimage')
    rs = np.random.RandomState(4)
    gt, pred = smooth_frames(rs, 2, 37, 53)
    x, y = np.clip(gt.astype(np.float64) * 0.5 + 0.5, 0, 1) * 255., np.clip(pred.astype(np.float64) * 0.5 + 0.5, 0, 1) * 255.

    def filt(a):
        return np.stack([[ndi.gaussian_filter(p, 1.5, truncate=3.5, mode='reflect') for p in fr] for fr in a])

    C1, C2 = (0.01 * 255)**2, (0.03 * 255)**2
    ux, uy = filt(x), filt(y)
    vx, vy, vxy = filt(x * x) - ux * ux, filt(y * y) - uy * uy, filt(x * y) - ux * uy
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    want = S[:, :, 5:-5, 5:-5].reshape(2, -1).mean(1)
    assert np.abs(image_scores(gt, pred)[2] - want).max() <= 1e-10


@pytest.mark.parametrize('H,W', [(64, 64), (37, 53)])
def test_host_image_metrics(H, W):
    from slotformer_amd.video_prediction import vp_utils as v
    rs = np.random.RandomState(5)
    gt, pred = smooth_frames(rs, 3, H, W)
    mse, psnr, ssim = image_scores(gt, pred)
    x, y = np.clip(gt.astype(np.float64) * 0.5 + 0.5, 0, 1), np.clip(pred.astype(np.float64) * 0.5 + 0.5, 0, 1)   # what pred_eval_step hands over
    assert abs(v.mse_metric(x, y) - mse.mean()) <= 1e-5 * mse.mean()
    assert abs(v.mse_metric(torch.from_numpy(x), torch.from_numpy(y)).item() - mse.mean()) <= 1e-5 * mse.mean()
    assert abs(v.psnr_metric(x, y) - psnr.mean()) <= 1e-9
    assert abs(v.ssim_metric(x, y) - ssim.mean()) <= 1e-9
    assert abs(v.ssim_metric(torch.from_numpy(x), torch.from_numpy(y)) - ssim.mean()) <= 1e-9
    assert v.psnr_metric(x, x) == np.inf and abs(v.ssim_metric(x, x) - 1.) <= 1e-12
    assert abs(float(v.perceptual_dist(torch.from_numpy(x), torch.from_numpy(y), lambda a, b: (a - b).abs().mean((1, 2, 3)))) - np.abs(x - y).mean()) < 1e-6


@pytest.mark.parametrize('n_obj,n_pred', [(1, 2), (3, 7), (6, 4), (9, 12), (15, 16)])
def test_host_mask_and_box_metrics(n_obj, n_pred, monkeypatch):
    from slotformer_amd.video_prediction import vp_utils as v
    gt, pm, pres, gtb, pb = mask_case(100 + n_obj, 3, 48, 40, n_obj, n_pred)
    want = mask_scores(gt, pm, pres, gtb, pb)
    tg, tp = torch.from_numpy(gt), torch.from_numpy(pm)
    assert np.abs(v.adjusted_rand_index(tg, tp).numpy() - want['ari']).max() <= 1e-12
    assert np.abs(v.adjusted_rand_index(tg, tp, ignore_background=True).numpy() - want['fari']).max() <= 1e-12
    assert abs(v.ARI_metric(tg, tp) - want['ari'].mean()) <= 1e-12 and abs(v.fARI_metric(tg, tp.to(torch.uint8)) - want['fari'].mean()) <= 1e-12
    assert abs(v.miou_metric(tg, tp) - want['miou'].mean()) <= 1e-12
    assert abs(v.hungarian_miou(tg[0].flatten(), tp[0].flatten()) - want['miou'][0]) <= 1e-12
    with monkeypatch.context() as mp:   # the assignment without scipy
        import sys
        mp.setitem(sys.modules, 'scipy.optimize', None)
        assert abs(v.miou_metric(tg, tp) - want['miou'].mean()) <= 1e-12
    # boxes
    got = v.masks_to_boxes(tp.unsqueeze(0), n_pred)
    assert got.shape == (1, 3, n_pred, 4) and np.array_equal(got[0].numpy(), pb)
    assert np.array_equal(v.masks_to_boxes_w_empty_mask(torch.from_numpy(pm == 0).long()).numpy(), pb[:, 0])
    ap, ar = v.batch_bbox_precision_recall(torch.from_numpy(pres), torch.from_numpy(gtb), torch.from_numpy(pb))
    assert abs(ap - want['ap'].mean()) <= 1e-12 and abs(ar - want['ar'].mean()) <= 1e-12
    p0, r0 = v.bbox_precision_recall(torch.from_numpy(pres[0]), torch.from_numpy(gtb[0]), torch.from_numpy(pb[0]))
    assert abs(p0 - want['ap'][0]) <= 1e-12 and abs(r0 - want['ar'][0]) <= 1e-12


def test_host_edge_rules():
    from slotformer_amd.video_prediction import vp_utils as v
    z = torch.zeros(1, 12, 12, dtype=torch.int64)
    assert v.ARI_metric(z, z) == 1. and v.fARI_metric(z, z) == 1.          # denominators of 0
    assert np.isnan(v.miou_metric(z, z))                                     # no foreground pixel
    gt, pm, pres, gtb, pb = mask_case(7, 1, 24, 24, 2, 3, gt_ids=[2, 5])    # absent ids in the middle of the range
    assert abs(v.miou_metric(torch.from_numpy(gt), torch.from_numpy(pm)) - miou_of(table_of(gt[0], pm[0]))) <= 1e-12
    assert abs(miou_of(table_of(gt[0], gt[0])) - 2. / 5.) <= 1e-9            # two perfect objects out of a one_hot width of five
    nan = v.bbox_precision_recall(torch.zeros(2, dtype=torch.bool), torch.from_numpy(gtb[0][:2]), torch.from_numpy(pb[0]))
    assert np.isnan(nan[0]) and np.isnan(nan[1])
    nan = v.bbox_precision_recall(torch.ones(2, dtype=torch.bool), torch.from_numpy(gtb[0][:2]), -torch.ones(3, 4))
    assert np.isnan(nan[0]) and np.isnan(nan[1])
    with pytest.raises(RuntimeError):
        v.masks_to_boxes(torch.full((1, 1, 4, 4), 9), 7)


def test_pred_eval_step_host():
    from slotformer_amd.video_prediction import vp_utils as v
    B, T, H, W = 2, 3, 32, 24
    rs = np.random.RandomState(8)
    gt, pred = smooth_frames(rs, B * T, H, W)
    gm, pm, pres, gtb, pb = mask_case(9, B * T, H, W, 3, 5)
    t5 = lambda a: torch.from_numpy(a).view(B, T, *a.shape[1:])   # noqa: E731
    args = dict(gt_mask=t5(gm), pred_mask=t5(pm), gt_pres_mask=t5(pres), gt_bbox=t5(gtb), pred_bbox=t5(pb))
    out = v.pred_eval_step(t5(gt).double(), t5(pred).double(), None, **args)   # (float64 frames: the to_rgb map of the host path rounds nothing)
    assert sorted(out) == sorted(['mse', 'ssim', 'psnr', 'percept_dist', 'ari', 'fari', 'miou', 'ap', 'ar'])
    assert all(len(x) == T and all(type(f) is float for f in x) for x in out.values()) and out['percept_dist'] == [0.] * T
    img = image_scores(gt, pred)
    want = dict(zip(('mse', 'psnr', 'ssim'), img), **mask_scores(gm, pm, pres, gtb, pb))
    for k, val in want.items():
        tol = 1e-5 * np.abs(val).max() if k == 'mse' else 1e-9
        assert np.abs(np.array(out[k]) - val.reshape(B, T).mean(0)).max() <= tol, k
    out2 = v.pred_eval_step(t5(gt).double(), t5(pred).double(), lambda a, b: (a - b).abs().mean((1, 2, 3)), eval_traj=False)
    assert all(out2[k] == [0.] * T for k in ('ari', 'fari', 'miou', 'ap', 'ar')) and out2['mse'] == out['mse']
    assert abs(out2['percept_dist'][1] - np.abs(gt.reshape(B, T, -1)[:, 1] - pred.reshape(B, T, -1)[:, 1]).mean()) < 1e-6
    with pytest.raises(RuntimeError):
        v.pred_eval_step_device(t5(gt), t5(pred), **args)   # host tensors: pred_eval_step is the entry that takes them


def test_reference_fixture_host_path():
    """The reference's own adjusted_rand_index / miou_metric / mse_metric on seeded blob masks and frames: ours within twice the distance the
    reference's float32 arithmetic keeps from the float64 restatement, and to that restatement within rounding."""
    from slotformer_amd.video_prediction import vp_utils as v
    g = gu.load_golden('vp_metrics')
    for res in (64, 128):
        gt, pm = fixture_masks(res)
        tabs = [table_of(a, b) for a, b in zip(gt, pm)]
        tg, tp = torch.from_numpy(gt), torch.from_numpy(pm)
        for name, ours, f64 in (('ari', v.adjusted_rand_index(tg, tp).numpy(), np.array([ari_of(t) for t in tabs])),
                                ('fari', v.adjusted_rand_index(tg, tp, ignore_background=True).numpy(), np.array([ari_of(t, True) for t in tabs]))):
            ref, dist = g[f'{name}_{res}'], float(g[f'{name}_{res}_ref_minus_f64'])
            assert np.abs(ref - f64).max() <= dist * (1 + 1e-9)
            assert np.abs(ours - ref).max() <= 2 * dist, (name, res)
            assert np.abs(ours - f64).max() <= 1e-12
        f64 = np.mean([miou_of(t) for t in tabs])
        assert abs(v.miou_metric(tg, tp) - g[f'miou_{res}']) <= 2 * float(g[f'miou_{res}_ref_minus_f64']) and abs(v.miou_metric(tg, tp) - f64) <= 1e-12
        x, y = fixture_frames(res)
        ours = float(v.mse_metric(x, y))
        assert abs(ours - g[f'mse_{res}']) <= 2 * float(g[f'mse_{res}_ref_minus_f64'])


def fixture_masks(res):
    """The seeded masks of tests/golden/vp_metrics.npz (8 frames per resolution, 1 .. 6 objects)."""
    rs = np.random.RandomState(1000 + res)
    parts = [blob_masks(rs, 2, res, res, n, m) for n, m in ((1, 3), (3, 7), (5, 7), (6, 5))]
    return np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])


def fixture_frames(res):
    """The seeded frames of the fixture, in [0, 1] (what mse_metric takes)."""
    gt, pred = smooth_frames(np.random.RandomState(2000 + res), 4, res, res)
    return np.clip(gt * 0.5 + 0.5, 0, 1), np.clip(pred * 0.5 + 0.5, 0, 1)


def test_entry_points_reject_bad_arguments():
    """Argument errors are negative codes with a message, raised before any device work."""
    import ctypes as C
    from slotformer_amd import _lib
    lib = _lib.lib()

    def err():
        return lib.sf_last_error_string().decode()

    one = C.c_void_p(16)
    assert lib.sf_vp_metrics_workspace_bytes(4, 64, 64) > 0 and lib.sf_vp_metrics_workspace_bytes(4, 10, 64) == 0
    assert lib.sf_vp_metrics_workspace_bytes(1600, 128, 128) >= 1600 * 256 * 4 + 1600 * 3 * 16 * 16
    assert lib.sf_vp_image_metrics_f32(None, one, one, one, one, 1, 64, 64, 1, one, 1 << 30, None) < 0 and 'null pointer' in err()
    assert lib.sf_vp_image_metrics_f32(one, one, one, one, one, 1, 10, 64, 1, one, 1 << 30, None) < 0 and 'at least 11' in err()
    assert lib.sf_vp_image_metrics_f32(one, one, one, one, one, 1, 64, 7, 1, one, 1 << 30, None) < 0 and 'at least 11' in err()
    assert lib.sf_vp_image_metrics_f32(one, one, one, one, one, 4, 64, 64, 1, one, 16, None) < 0 and 'workspace' in err()
    assert lib.sf_vp_mask_metrics(one, None, 0, None, None, one, one, one, one, 1, 8, 8, 16, one, 1 << 30, None) < 0 and 'null pointer' in err()
    assert lib.sf_vp_mask_metrics(one, one, 0, None, None, one, one, one, one, 1, 8, 8, 17, one, 1 << 30, None) < 0 and '16 classes' in err()
    assert lib.sf_vp_mask_metrics(one, one, 1, None, None, one, one, one, one, 4, 8, 8, 16, None, 0, None) < 0 and 'workspace' in err()
    assert lib.sf_masks_to_boxes(one, 0, None, None, 1, 8, 8, 7, None) < 0 and 'null pointer' in err()
    assert lib.sf_masks_to_boxes(one, 0, one, None, 1, 8, 8, 17, None) < 0 and '16 classes' in err()
    assert lib.sf_vp_bbox_pr_f32(one, one, None, one, one, 1, 4, 4, 0.5, None) < 0 and 'null pointer' in err()
    assert lib.sf_vp_bbox_pr_f32(one, one, one, one, one, 1, 65, 4, 0.5, None) < 0 and '64 boxes' in err()
    assert lib.sf_vp_mean_over_videos_f64(one, None, 8, 2, 3, None) < 0 and 'null pointer' in err()
    assert lib.sf_vp_mean_over_videos_f64(one, one, 8, 0, 3, None) < 0
