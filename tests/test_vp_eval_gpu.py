"""GPU: harness.evaluate_video_prediction (the loop of test_vp.py on the device) against the same loop written out here with the existing
`pred_eval_step` per batch -- one download per batch -- and the AverageMeter arithmetic on the host.

Both sides run the same kernels on the same inputs and sum in float64 in the same order (sum += mean * B per batch, one division at the end), so
every entry agrees within 1e-12 relative -- the only difference allowed is a fused multiply-add in the last bit -- and NaNs sit in the same
places.  The NaN entries come from a ground-truth frame without objects: no present box (precision and recall of that step are NaN) and no
foreground pixel (so is its mIoU).  A decoded segmentation always holds at least one id, so a frame without a PREDICTED box cannot be produced
through the decoder."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import annotation_cases as AC
import golden_util as gu

pytestmark = pytest.mark.gpu

V, HIST, ROLL, RES, BATCH = 5, 6, 4, 64, 2
TRAJ = ('ari', 'fari', 'miou', 'ap', 'ar')
KEYS = ('mse', 'psnr', 'ssim', 'percept_dist') + TRAJ
SRC = (40, 60)   # the annotations' frame size


@functools.lru_cache(maxsize=None)
def setup():
    """The model (on the CPU: moved by the tests), slots, frames, annotations and the host ground truth; built once, never modified."""
    from slotformer_amd import annotations as a
    from slotformer_amd.base_slots import build_model as bb
    from slotformer_amd.ingest import FrameIngest
    from slotformer_amd.video_prediction import build_model as bv
    torch.manual_seed(2024)
    scfg = gu.savi_cfg(RES, 6)
    savi = bb(gu.ParamsView(scfg))
    path = os.path.join(tempfile.mkdtemp(), 'savi.pth')
    torch.save({'state_dict': savi.state_dict()}, path)
    rcfg = gu.rollout_cfg(6, 128, HIST, 128, 4, 8, 512, rollout_len=ROLL, res=RES)
    rcfg['dec_dict'] = dict(scfg['dec_dict'], dec_ckp_path=path)
    model = bv(gu.ParamsView(rcfg)).eval()
    rs = np.random.RandomState(99)
    T = HIST + ROLL
    slots = torch.from_numpy(rs.standard_normal((V, T, 6, 128)).astype(np.float32))
    frames = torch.from_numpy((rs.rand(V, T, 3, RES, RES) * 2 - 1).astype(np.float32))
    h, w = SRC
    anno = []
    for v in range(V):
        clip = []
        for t in range(T):
            objs = []
            for _ in range(rs.randint(1, 6)):
                y0, x0 = rs.randint(0, h - 4), rs.randint(0, w - 4)
                objs.append(AC.encode(AC.rect(h, w, y0, y0 + rs.randint(2, h // 2), x0, x0 + rs.randint(2, w // 2))))
            clip.append(objs)
        anno.append(clip)
    anno[3][HIST + 1] = []   # a scored frame without objects: no present box, no foreground pixel
    gt = a.ground_truth(anno, FrameIngest((RES, RES)))
    assert tuple(gt['mask'].shape) == (V, T, RES, RES)
    return model, slots, frames, anno, gt


def host_loop(model, slots, frames, gt, dev, eval_traj=True, lpips=None):
    """test_vp.py:139-163, 211-219 with pred_eval_step per batch and AverageMeter on the host"""
    from slotformer_amd import engine
    from slotformer_amd.video_prediction import vp_utils as v
    sums = {k: [0.0] * ROLL for k in KEYS}
    count = 0
    for s in range(0, V, BATCH):
        e = min(s + BATCH, V)
        B = e - s
        clip = torch.zeros(B, HIST + ROLL, 6, 128, device=dev)
        clip[:, :HIST] = slots[s:e, :HIST].to(dev)
        engine.rollout(model.rollouter, clip, HIST, ROLL)
        recon, _, _, seg = engine.savi_decode(model, clip[:, HIST:].reshape(B * ROLL, 6, 128), want=('seg', ), seg_dtype=torch.uint8)
        recon, seg = recon.view(B, ROLL, 3, RES, RES), seg.view(B, ROLL, RES, RES)
        kw = dict(eval_traj=False)
        if eval_traj:
            kw = dict(gt_mask=gt['mask'][s:e, HIST:].to(dev), pred_mask=seg, gt_pres_mask=gt['pres_mask'][s:e, HIST:].to(dev),
                      gt_bbox=gt['bbox'][s:e, HIST:].to(dev), pred_bbox=v.masks_to_boxes(seg, model.num_slots))
        step = v.pred_eval_step(frames[s:e, HIST:].to(dev).contiguous(), recon, lpips, **kw)
        for k in KEYS:
            for t in range(ROLL):
                sums[k][t] += step[k][t] * B      # AverageMeter.update(val, n): sum += val * n
        count += B
    return {k: np.array([x / count for x in sums[k]]) for k in KEYS}


def check_equal(got, want):
    for k in KEYS:
        g, w = got[k], want[k]
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == (ROLL, ), k
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (k, g, w)
        inf = np.isinf(w)
        assert np.array_equal(g[inf], w[inf]), k
        fin = ~nan & ~inf
        err = np.abs(g[fin] - w[fin]) / np.maximum(np.abs(w[fin]), 1e-300)
        print(f'{k}: max relative difference {err.max() if fin.any() else 0.:.3e}')
        assert (err <= 1e-12).all(), (k, g, w)


@torch.no_grad()
def test_loop_equals_pred_eval_step_per_batch(dev):
    from slotformer_amd import harness
    model, slots, frames, anno, gt = setup()
    model = model.to(dev)
    want = host_loop(model, slots, frames, gt, dev)
    assert np.isnan(want['ap'][1]) and np.isnan(want['ar'][1]) and np.isnan(want['miou'][1]) and not np.isnan(want['ap'][[0, 2, 3]]).any()
    assert (want['percept_dist'] == 0).all() and np.isfinite(want['mse']).all()
    from_anno = harness.evaluate_video_prediction(model, slots, frames, batch_size=BATCH, annotations=anno)
    assert list(from_anno) == list(KEYS) + ['num_videos'] and from_anno['num_videos'] == V
    check_equal(from_anno, want)
    from_gt = harness.evaluate_video_prediction(model, slots, frames, batch_size=BATCH, gt=gt)
    for k in KEYS:
        assert np.array_equal(from_anno[k], from_gt[k], equal_nan=True), k
    # device-resident inputs and an explicit rollout_len give the same numbers
    on_dev = harness.evaluate_video_prediction(model, slots.to(dev), frames.to(dev), rollout_len=ROLL, batch_size=BATCH, annotations=anno)
    for k in KEYS:
        assert np.array_equal(from_anno[k], on_dev[k], equal_nan=True), k


@torch.no_grad()
def test_without_trajectory_scores(dev):
    from slotformer_amd import harness
    model, slots, frames, anno, gt = setup()
    model = model.to(dev)
    want = host_loop(model, slots, frames, gt, dev, eval_traj=False)
    for got in (harness.evaluate_video_prediction(model, slots, frames, batch_size=BATCH, annotations=anno, eval_traj=False),
                harness.evaluate_video_prediction(model, slots, frames, batch_size=BATCH)):
        check_equal(got, want)
        assert all((got[k] == 0).all() for k in TRAJ) and (got['mse'] > 0).all()


@torch.no_grad()
def test_perceptual_distance_rides_along(dev):
    """lpips=: the per-step means of the device LPIPS are accumulated like the other scores (pred_eval_step takes them from the same launches)"""
    import lpips_cases as lc
    from slotformer_amd import harness
    from slotformer_amd.lpips import LPIPS
    model, slots, frames, anno, gt = setup()
    model = model.to(dev)
    net = LPIPS()
    net.load_state_dict(lc.seeded_weights(0))
    net = net.to(dev)
    want = host_loop(model, slots, frames, gt, dev, lpips=net)
    assert (want['percept_dist'] > 0).all()
    check_equal(harness.evaluate_video_prediction(model, slots, frames, batch_size=BATCH, annotations=anno, lpips=net), want)


@torch.no_grad()
def test_raw_frames_through_ingest(dev):
    """ingest=: the raw uint8 clips, resized and normalised per batch on the device, give what the float frames of the same ingest give"""
    from slotformer_amd import harness
    from slotformer_amd.ingest import FrameIngest
    model, slots, _, anno, _ = setup()
    model = model.to(dev)
    rs = np.random.RandomState(3)
    raw = torch.from_numpy(rs.randint(0, 256, (V, HIST + ROLL, SRC[0], SRC[1], 3)).astype(np.uint8))
    ing = FrameIngest((RES, RES))
    got = harness.evaluate_video_prediction(model, slots, raw, batch_size=BATCH, ingest=ing, annotations=anno)
    want = harness.evaluate_video_prediction(model, slots, ing(raw.to(dev)), batch_size=BATCH, annotations=anno)
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), k


@torch.no_grad()
def test_out_of_range_id_raises_at_the_end(dev):
    from slotformer_amd import harness
    model, slots, frames, _, gt = setup()
    model = model.to(dev)
    bad = dict(gt, mask=gt['mask'].clone())
    bad['mask'][4, HIST + 2, 5, 7] = 16   # in the last, ragged batch
    with pytest.raises(RuntimeError, match='outside'):
        harness.evaluate_video_prediction(model, slots, frames, batch_size=BATCH, gt=bad)
