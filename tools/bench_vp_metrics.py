#!/usr/bin/env python
"""Time the video-prediction metrics on the device: pred_eval_step_device at 32 videos x 50 predicted frames x 128 x 128 with 7 slots, its image
kernel and its mask kernels by themselves, and the same scores through torch operations on the same GPU.

    python tools/bench_vp_metrics.py [--videos 32 --frames 50 --res 128] [--out profiles/vp_metrics.md]

Method: every shape is warmed up; a window of calls is bracketed by two events; windows are repeated until at least one second has been timed
and the median window is reported.  Bytes are the bytes the algorithm must move (each input once, outputs once), computed from the shapes; the
roof is the 6.3 TB/s a float4 copy reaches on this part.  Needs a GPU; there is no fallback."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
COPY_ROOF = 6.3e12


def timed(fn, min_seconds=1.0, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    per_window = max(1, int(0.1 / max(e0.elapsed_time(e1) * 1e-3, 1e-6)))
    windows, total = [], 0.
    while total < min_seconds or len(windows) < 5:
        e0.record()
        for _ in range(per_window):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        windows.append(ms / per_window)
        total += ms * 1e-3
    return float(np.median(windows)), float(np.min(windows)), float(np.max(windows)), len(windows) * per_window


def torch_image_scores(gt, pred):
    """MSE / PSNR / SSIM per frame in torch operations (float32, grouped separable convolutions)."""
    import torch.nn.functional as F_
    x, y = (gt * 0.5 + 0.5).clamp(0, 1), (pred * 0.5 + 0.5).clamp(0, 1)
    n, _, H, W = x.shape
    sse = ((x - y)**2).flatten(1).sum(1)
    w = torch.exp(-0.5 * (torch.arange(-5, 6, device=x.device, dtype=torch.float32) / 1.5)**2)
    w = w / w.sum()
    q = torch.cat([x, y, x * x, y * y, x * y], 1)                       # [n,15,H,W]; only the cropped map is needed: no padding
    q = F_.conv2d(q, w.view(1, 1, 1, 11).expand(15, 1, 1, 11), groups=15)
    q = F_.conv2d(q, w.view(1, 1, 11, 1).expand(15, 1, 11, 1), groups=15)
    ux, uy, uxx, uyy, uxy = q.split(3, 1)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    S = ((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
    return sse / 3, 10 * torch.log10(1 / (sse / (3 * H * W))), S.flatten(1).mean(1)


def torch_mask_scores(gm, pm, pres, gtb, pb):
    """ARI / FG-ARI on the device from a bincount table (float64); mIoU and the boxes' precision / recall as the host path does them, after one
    download of the tables and boxes (torch has no assignment solver)."""
    from slotformer_amd.video_prediction import vp_utils as v
    n = gm.shape[0]
    flat = (torch.arange(n, device=gm.device).view(n, 1) * 16 + gm.flatten(1)) * 16 + pm.flatten(1).long()
    tab = torch.bincount(flat.flatten(), minlength=n * 256).view(n, 16, 16).double()
    ari, fari = v._ari_from_table(tab), v._ari_from_table(tab[:, 1:])
    tabs = tab.cpu().numpy()
    miou = [v._miou_from_table(t) for t in tabs]
    pr = [v.bbox_precision_recall(a, b, c) for a, b, c in zip(pres.cpu(), gtb.cpu(), pb.cpu())]
    return ari, fari, miou, pr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--videos', type=int, default=32)
    ap.add_argument('--frames', type=int, default=50)
    ap.add_argument('--res', type=int, default=128)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_vp_metrics needs a GPU'
    from slotformer_amd import _lib
    from slotformer_amd.video_prediction import vp_utils as v
    import test_vp_metrics as R
    dev = torch.device('cuda:0')
    B, T, H = a.videos, a.frames, a.res
    F = B * T
    rs = np.random.RandomState(0)
    g8, p8 = R.smooth_frames(rs, 8, H, H)
    gm8, pm8, pres8, gtb8, pb8 = R.mask_case(1, 8, H, H, 6, 7)
    rep = lambda x: torch.from_numpy(np.concatenate([x] * ((F + 7) // 8))[:F]).to(dev)   # noqa: E731
    gt, pred = rep(g8) + 0.01 * torch.randn(F, 3, H, H, device=dev), rep(p8)
    gm, pm, pres, gtb, pb = rep(gm8), rep(pm8).to(torch.uint8), rep(pres8), rep(gtb8), rep(pb8)
    v5 = lambda x: x.view(B, T, *x.shape[1:])   # noqa: E731
    args = dict(gt=v5(gt), pred=v5(pred), gt_mask=v5(gm), pred_mask=v5(pm), gt_pres_mask=v5(pres), gt_bbox=v5(gtb), pred_bbox=v5(pb))
    lib = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    ws = torch.empty(lib.sf_vp_metrics_workspace_bytes(F, H, H), dtype=torch.uint8, device=dev)
    o = torch.empty(8, F, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def image():
        _lib.check(lib.sf_vp_image_metrics_f32(gt.data_ptr(), pred.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), F, H, H, 1,
                                               ws.data_ptr(), ws.numel(), st))

    def masks():
        _lib.check(lib.sf_vp_mask_metrics(gm.data_ptr(), pm.data_ptr(), 1, None, None, o[3].data_ptr(), o[4].data_ptr(), o[5].data_ptr(),
                                          flag.data_ptr(), F, H, H, 16, ws.data_ptr(), ws.numel(), st))
        _lib.check(lib.sf_vp_bbox_pr_f32(gtb.data_ptr(), pres.view(torch.uint8).data_ptr(), pb.data_ptr(), o[6].data_ptr(), o[7].data_ptr(), F,
                                         gtb.shape[1], pb.shape[1], 0.5, st))

    img_bytes = 2 * F * 3 * H * H * 4 + 3 * F * 8
    mask_bytes = F * H * H * (8 + 1) + F * (gtb.shape[1] * 17 + pb.shape[1] * 16) + 5 * F * 8
    rows = []
    for name, fn, nbytes in (('pred_eval_step_device (all six launches)', lambda: v.pred_eval_step_device(**args), img_bytes + mask_bytes),
                             ('image kernel (MSE, PSNR, SSIM)', image, img_bytes), ('mask kernels (ARI, FG-ARI, mIoU, AP/AR)', masks, mask_bytes)):
        med, lo, hi, calls = timed(fn)
        rows.append((name, med, lo, hi, calls, nbytes, nbytes / (med * 1e-3) / COPY_ROOF))
    t_img = timed(lambda: torch_image_scores(gt, pred), min_seconds=1.0, warmup=2)
    t_mask = timed(lambda: torch_mask_scores(gm, pm, pres, gtb, pb), min_seconds=1.0, warmup=1)
    # the two paths agree (float32 image scores; the table scores exactly)
    image()
    masks()
    ti = torch_image_scores(gt, pred)
    tm = torch_mask_scores(gm, pm, pres, gtb, pb)
    agree = {'mse': float(((o[0] - ti[0]).abs() / o[0]).max()), 'psnr': float((o[1] - ti[1]).abs().max()), 'ssim': float((o[2] - ti[2]).abs().max()),
             'ari': float((o[3] - tm[0]).abs().max()), 'miou': float(np.abs(o[5].cpu().numpy() - np.array(tm[2])).max())}
    lines = [f'shape: {B} videos x {T} frames x {H} x {H}, 7 slots (uint8 segmentation), {F} frames per call; device {torch.cuda.get_device_name(0)}', '',
             '| call | ms per batch (median) | min .. max of windows | calls timed | bytes moved | fraction of the 6.3 TB/s copy roof |', '|---|---|---|---|---|---|']
    for name, med, lo, hi, calls, nbytes, frac in rows:
        lines.append(f'| {name} | {med:.4f} | {lo:.4f} .. {hi:.4f} | {calls} | {nbytes / 1e6:.1f} MB | {frac:.3f} |')
    lines += ['', '| torch path on the same GPU | ms per batch (median) | ratio to the kernel |', '|---|---|---|',
              f'| image scores (float32 grouped convolutions) | {t_img[0]:.3f} | {t_img[0] / rows[1][1]:.1f}x |',
              f'| mask scores (bincount table, ARI on the device; assignment and boxes on the host) | {t_mask[0]:.3f} | {t_mask[0] / rows[2][1]:.1f}x |', '',
              'largest difference between the two paths on this input: ' + ', '.join(f'{k} {x:.2e}' for k, x in agree.items())]
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
