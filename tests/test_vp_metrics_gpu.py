"""GPU: the video-prediction metrics kernels (csrc/vp_metrics.hip) through vp_utils -- pred_eval_step_device / pred_eval_step on device tensors
against the float64 restatements of tests/test_vp_metrics.py, the reference fixture, the host path, and the harness's decoded frames.

Tolerances: everything that comes from the integer tables (boxes, ARI, FG-ARI, mIoU, precision / recall) holds to the restatement within 1e-12.
MSE / PSNR / SSIM are computed in float32 per pixel: the same algorithm is evaluated in float32 NumPy and in float64 on the case's own frames,
and the device may lie twice that distance from the float64 result."""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import test_vp_metrics as R

pytestmark = pytest.mark.gpu

IMG, TAB = ('mse', 'psnr', 'ssim'), ('ari', 'fari', 'miou', 'ap', 'ar')
GROUPS = {'64': (3, 4, 64, 64, [(1, 2, None), (3, 7, None), (7, 4, None), (15, 16, None), (9, 12, None), (3, 16, [2, 5, 9])]),
          '128': (3, 4, 128, 128, [(2, 3, None), (6, 7, None), (12, 9, None), (15, 16, None), (4, 2, None), (4, 11, [1, 7, 8, 14])]),
          'ragged': (2, 3, 37, 53, [(1, 2, None), (3, 4, None), (6, 7, None)])}


def _pad(a, n):
    return np.concatenate([a, -np.ones((a.shape[0], n - a.shape[1], 4), np.float32)], 1)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs (NumPy) + the float64 scores per frame + the image tolerances of a case; computed once, never modified."""
    B, T, H, W, groups = GROUPS[name]
    per = B * T // len(groups)
    rs = np.random.RandomState(len(name) * 77 + H)
    gt, pred = R.smooth_frames(rs, B * T, H, W)
    parts = [R.mask_case(500 + 31 * i + H, per, H, W, n, m, **({'gt_ids': ids} if ids else {})) for i, (n, m, ids) in enumerate(groups)]
    gm, pm = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    pres = np.concatenate([np.concatenate([p[2], np.zeros((per, 16 - p[2].shape[1]), bool)], 1) for p in parts])
    gtb, pb = np.concatenate([_pad(p[3], 16) for p in parts]), np.concatenate([_pad(p[4], 16) for p in parts])
    # frame 0 equals its ground truth: PSNR inf, SSIM 1, ARI 1
    pred[0], pm[0] = gt[0], gm[0]
    pb[0] = R.boxes_of(pm[0], 16)
    assert all((gm[f] > 0).any() and pres[f].any() and (pb[f][:, 0] >= 0).any() for f in range(B * T))   # no frame falls under a NaN rule
    want = dict(zip(IMG, R.image_scores(gt, pred)), **R.mask_scores(gm, pm, pres, gtb, pb))
    f32 = dict(zip(IMG, R.image_scores(gt, pred, np.float32)))
    fin = np.isfinite(want['psnr'])
    tol = {k: 2 * float(np.abs(f32[k][fin] - want[k][fin]).max()) for k in IMG}
    assert want['psnr'][0] == np.inf and f32['psnr'][0] == np.inf and abs(want['ssim'][0] - 1) < 1e-12 and want['ari'][0] == 1.
    return dict(B=B, T=T, H=H, W=W, gt=gt, pred=pred, gm=gm, pm=pm, pres=pres, gtb=gtb, pb=pb, want=want, tol=tol)


def dev_args(c, dev, seg_dtype=torch.int64):
    B, T = c['B'], c['T']
    t = lambda a: torch.from_numpy(a).view(B, T, *a.shape[1:]).to(dev)   # noqa: E731
    return dict(gt=t(c['gt']), pred=t(c['pred']), gt_mask=t(c['gm']), pred_mask=t(c['pm']).to(seg_dtype), gt_pres_mask=t(c['pres']),
                gt_bbox=t(c['gtb']), pred_bbox=t(c['pb']))


def check_scores(got, want, tol, B, T, label):
    """got: '<name>_per_video' [B,T] / '<name>' [T] arrays; want: float64 per frame."""
    for k in IMG + TAB:
        w = want[k].reshape(B, T)
        g = np.asarray(got[k + '_per_video'])
        bound = tol[k] if k in IMG else 1e-12
        fin = np.isfinite(w)
        print(f'{label} {k}: max |device - float64| = {np.abs(g[fin] - w[fin]).max():.3e}, bound {bound:.3e}')
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), (label, k)
        assert np.abs(g[fin] - w[fin]).max() <= bound, (label, k)
        m = np.asarray(got[k])
        with np.errstate(invalid='ignore'):
            wm = w.mean(0)
        fin = np.isfinite(wm)
        assert np.array_equal(np.isnan(m), np.isnan(wm)) and np.abs(m[fin] - wm[fin]).max() <= bound * (1 + 1e-9) + 1e-15, (label, k, 'mean')


@pytest.mark.parametrize('seg_dtype', [torch.int64, torch.uint8])
@pytest.mark.parametrize('name', list(GROUPS))
def test_device_scores_against_float64(dev, name, seg_dtype):
    from slotformer_amd.video_prediction import vp_utils as v
    c = case(name)
    args = dev_args(c, dev, seg_dtype)
    out = v.pred_eval_step_device(**args)
    assert int(out['id_out_of_range'].item()) == 0
    check_scores({k: t.cpu().numpy() for k, t in out.items()}, c['want'], c['tol'], c['B'], c['T'], f'{name}/{seg_dtype}')
    # boxes and tables are integers: exact
    boxes = v.masks_to_boxes(args['pred_mask'], 16).cpu().numpy().reshape(-1, 16, 4)
    assert np.array_equal(boxes, np.stack([R.boxes_of(m, 16) for m in c['pm']]))
    assert np.array_equal(v.masks_to_boxes(args['pred_mask'], 7).cpu().numpy().reshape(-1, 7, 4)[1], R.boxes_of(np.where(c['pm'][1] < 7, c['pm'][1], -1), 7))
    _, flag, tables = v._dev_mask_scores(args['gt_mask'].flatten(0, 1).flatten(1), args['pred_mask'].flatten(0, 1).flatten(1), c['H'], c['W'])
    assert np.array_equal(tables.cpu().numpy(), np.stack([R.table_of(a, b) for a, b in zip(c['gm'], c['pm'])]))
    # the per-frame functions on device tensors (images in [0, 1])
    x, y = (args['gt'][:, 0] * 0.5 + 0.5).clamp(0, 1), (args['pred'][:, 0] * 0.5 + 0.5).clamp(0, 1)
    w = {k: c['want'][k].reshape(c['B'], c['T'])[:, 0] for k in IMG + TAB}
    if np.isfinite(w['psnr']).all():
        assert abs(v.psnr_metric(x, y) - w['psnr'].mean()) <= c['tol']['psnr']
    assert abs(v.mse_metric(x, y) - w['mse'].mean()) <= c['tol']['mse'] and abs(v.ssim_metric(x, y) - w['ssim'].mean()) <= c['tol']['ssim']
    gm0, pm0 = args['gt_mask'][:, 0], args['pred_mask'][:, 0]
    assert abs(v.ARI_metric(gm0, pm0) - w['ari'].mean()) <= 1e-12 and abs(v.fARI_metric(gm0, pm0) - w['fari'].mean()) <= 1e-12
    assert abs(v.miou_metric(gm0, pm0) - w['miou'].mean()) <= 1e-12
    assert abs(v.hungarian_miou(gm0[1].flatten(), pm0[1].flatten()) - w['miou'][1]) <= 1e-12
    ap, ar = v.batch_bbox_precision_recall(args['gt_pres_mask'][:, 0], args['gt_bbox'][:, 0], args['pred_bbox'][:, 0])
    assert abs(ap - w['ap'].mean()) <= 1e-12 and abs(ar - w['ar'].mean()) <= 1e-12


def test_nan_rules(dev):
    """One frame per rule: no foreground pixel (mIoU), no present ground-truth box, no predicted box (precision / recall)."""
    from slotformer_amd.video_prediction import vp_utils as v
    B, T, H, W = 1, 3, 24, 32
    rs = np.random.RandomState(11)
    gt, pred = R.smooth_frames(rs, 3, H, W)
    gm, pm, pres, gtb, pb = R.mask_case(12, 3, H, W, 2, 3)
    gm[0] = 0
    pres[1] = False
    pb[2] = -1
    want = dict(zip(IMG, R.image_scores(gt, pred)), **R.mask_scores(gm, pm, pres, gtb, pb))
    assert np.isnan(want['miou'][0]) and np.isnan(want['ap'][1]) and np.isnan(want['ar'][2]) and want['fari'][0] == 1.
    f32 = dict(zip(IMG, R.image_scores(gt, pred, np.float32)))
    tol = {k: 2 * float(np.abs(f32[k] - want[k]).max()) for k in IMG}
    c = dict(B=B, T=T, H=H, W=W, gt=gt, pred=pred, gm=gm, pm=pm, pres=pres, gtb=gtb, pb=pb)
    out = v.pred_eval_step_device(**dev_args(c, dev))
    check_scores({k: t.cpu().numpy() for k, t in out.items()}, want, tol, B, T, 'nan-rules')


def test_reference_fixture_device_path(dev):
    from slotformer_amd.video_prediction import vp_utils as v
    g = gu.load_golden('vp_metrics')
    for res in (64, 128):
        gt, pm = R.fixture_masks(res)
        tabs = [R.table_of(a, b) for a, b in zip(gt, pm)]
        tg, tp = torch.from_numpy(gt).to(dev), torch.from_numpy(pm).to(dev)
        for name, fg in (('ari', False), ('fari', True)):
            ours = v.adjusted_rand_index(tg, tp.to(torch.uint8) if fg else tp, ignore_background=fg).cpu().numpy()
            assert ours.dtype == np.float64
            assert np.abs(ours - g[f'{name}_{res}']).max() <= 2 * float(g[f'{name}_{res}_ref_minus_f64'])
            assert np.abs(ours - np.array([R.ari_of(t, fg) for t in tabs])).max() <= 1e-12
        ours = v.miou_metric(tg, tp)
        assert abs(ours - g[f'miou_{res}']) <= 2 * float(g[f'miou_{res}_ref_minus_f64']) and abs(ours - np.mean([R.miou_of(t) for t in tabs])) <= 1e-12
        x, y = R.fixture_frames(res)
        ours = v.mse_metric(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
        assert abs(ours - g[f'mse_{res}']) <= 2 * float(g[f'mse_{res}_ref_minus_f64'])


def test_pred_eval_step_drop_in(dev):
    """pred_eval_step on device inputs = pred_eval_step on the same inputs on the CPU."""
    from slotformer_amd.video_prediction import vp_utils as v
    c = case('64')
    args = dev_args(c, dev, torch.uint8)
    cpu = {k: t.cpu() for k, t in args.items()}
    lp = lambda a, b: (a - b).abs().mean((1, 2, 3))   # noqa: E731
    for lpips_fn, traj in ((None, True), (lp, True), (lp, False)):
        kw = {} if traj else {'eval_traj': False}
        a = v.pred_eval_step(lpips_fn=lpips_fn, **(args if traj else {k: args[k] for k in ('gt', 'pred')}), **kw)
        b = v.pred_eval_step(lpips_fn=lpips_fn, **(cpu if traj else {k: cpu[k] for k in ('gt', 'pred')}), **kw)
        assert sorted(a) == sorted(b) and all(len(x) == c['T'] and all(type(f) is float for f in x) for x in a.values())
        for k in IMG + TAB:
            x, y = np.array(a[k]), np.array(b[k])
            fin = np.isfinite(y)
            assert np.array_equal(x[~fin], y[~fin]) and np.abs(x[fin] - y[fin]).max() <= (c['tol'][k] if k in IMG else 1e-12), (k, traj)
        assert np.abs(np.array(a['percept_dist']) - np.array(b['percept_dist'])).max() <= (1e-6 if lpips_fn else 0.)
        if not traj:
            assert all(a[k] == [0.] * c['T'] for k in TAB)


def test_device_step_is_deterministic_and_capturable(dev):
    """Two calls give the same bits; the call captures into a graph on one stream (so it neither synchronises nor allocates) and replays to them."""
    from slotformer_amd.video_prediction import vp_utils as v
    c = case('ragged')
    args = dev_args(c, dev, torch.uint8)
    first = {k: t.clone() for k, t in v.pred_eval_step_device(**args).items()}
    second = v.pred_eval_step_device(**args)
    for k, t in first.items():
        assert torch.equal(t.view(torch.uint8), second[k].view(torch.uint8)), k
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        v.pred_eval_step_device(**args)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = v.pred_eval_step_device(**args)
    for t in out.values():
        t.view(torch.uint8).fill_(0xff)
    graph.replay()
    torch.cuda.synchronize(dev)
    for k, t in first.items():
        assert torch.equal(t.view(torch.uint8), out[k].view(torch.uint8)), k


def test_out_of_range_id_sets_the_flag(dev):
    from slotformer_amd.video_prediction import vp_utils as v
    c = case('ragged')
    args = dev_args(c, dev)
    args['pred_mask'] = args['pred_mask'].clone()
    args['pred_mask'][1, 2, 5, 7] = 16
    out = v.pred_eval_step_device(**args)
    assert int(out['id_out_of_range'].item()) == 1
    gm, pm = c['gm'].copy(), c['pm'].copy()
    pm[5, 5, 7] = 16   # (frame 1 * T + 2): the pixel is left out
    assert abs(out['ari_per_video'][1, 2].item() - R.ari_of(R.table_of(gm[5], pm[5]))) <= 1e-12
    with pytest.raises(RuntimeError):
        v.pred_eval_step(lpips_fn=None, **args)
    args['pred_mask'][1, 2, 5, 7] = 0
    assert int(v.pred_eval_step_device(**args)['id_out_of_range'].item()) == 0


@torch.no_grad()
def test_behind_extract_and_rollout(dev):
    """The decoded frames and uint8 segmentation of harness.extract_and_rollout, scored where they lie, equal the host path on the downloads."""
    from slotformer_amd import harness
    from slotformer_amd.base_slots import build_model
    from slotformer_amd.video_prediction import vp_utils as v
    from slotformer_amd.video_prediction.models import SlotRollouter
    B, T, Hn, res = 3, 6, 4, 64
    torch.manual_seed(21)
    savi = build_model(gu.ParamsView(gu.savi_cfg(res, 7, iters=2, kernel_mlp=False, pred='mlp', rnn=False, kld='var-0.01'))).eval().to(dev)
    savi.testing = True
    roll = SlotRollouter(**gu.C2_ROLL['rollout_dict']).eval().to(dev)
    rs = np.random.RandomState(41)
    V = 2 * B
    vids = torch.from_numpy((rs.rand(V, T, 3, res, res) * 2 - 1).astype(np.float32)).to(dev)
    nz = torch.from_numpy(rs.standard_normal((V, T, 7, 128)).astype(np.float32)).to(dev)
    _, dec = harness.extract_and_rollout(savi, roll, vids, Hn, batch_size=B, noises=nz, decoder=savi)
    assert dec['seg'].dtype == torch.uint8
    gt = torch.from_numpy((rs.rand(V, Hn, 3, res, res) * 2 - 1).astype(np.float32))
    gm, _, pres, gtb, _ = R.mask_case(77, V * Hn, res, res, 4, 7)
    t = lambda a: torch.from_numpy(a).view(V, Hn, *a.shape[1:])   # noqa: E731
    pred_bbox = v.masks_to_boxes(dec['seg'], 7)
    out = v.pred_eval_step_device(gt.to(dev), dec['recon'], t(gm).to(dev), dec['seg'], t(pres).to(dev), t(gtb).to(dev), pred_bbox)
    recon, seg = dec['recon'].cpu(), dec['seg'].cpu()
    assert torch.equal(pred_bbox.cpu(), v.masks_to_boxes(seg.long(), 7))
    host = v.pred_eval_step(gt, recon, None, t(gm), seg.long(), t(pres), t(gtb), pred_bbox.cpu())
    f64, f32 = R.image_scores(gt.flatten(0, 1).numpy(), recon.flatten(0, 1).numpy()), R.image_scores(gt.flatten(0, 1).numpy(), recon.flatten(0, 1).numpy(), np.float32)
    tol = {k: 2 * float(np.abs(a - b).max()) for k, a, b in zip(IMG, f32, f64)}
    for k in IMG + TAB:
        x, y = out[k].cpu().numpy(), np.array(host[k])
        fin = np.isfinite(y)
        print(f'end to end {k}: max |device - host| = {np.abs(x[fin] - y[fin]).max() if fin.any() else 0.:.3e}')
        assert np.array_equal(np.isnan(x), np.isnan(y)) and (not fin.any() or np.abs(x[fin] - y[fin]).max() <= (tol[k] if k in IMG else 1e-12)), k
    harness.release_pipelines()
