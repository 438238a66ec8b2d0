"""Measure the device ground truth and the video-prediction evaluation loop on an MI355X.

    python tools/bench_vp_eval.py [--seconds 1.0] [--videos 32] [--json PATH]

(a) `annotations.ground_truth` of a CLEVRER-shaped clip batch -- 8 x 48 frames, 320 x 480 source, 6 objects per frame, 64 x 64 out -- on the
    device (from the packed record, already uploaded: the two launches + one synchronise) against the host path the reference's dataset takes:
    a dense NumPy decode of every object, the background channel, `FrameIngest.process_mask` on the CPU, boxes, compact, pad, argmax.  The
    one-time host parse + pack of the run lengths is reported by itself: both paths need the runs parsed.
(b) `harness.evaluate_video_prediction` against the same loop written with `vp_utils.pred_eval_step` per batch (one download per batch) and the
    AverageMeter arithmetic on the host: the CLEVRER SlotFormer at 64 x 64 (7 slots of 128, burn-in 6, rollout 42), seeded weights and inputs,
    batches of 8, ground truth given as ready device tensors to both (so the difference is the loop, not the ground truth).

The paths of a measurement ALTERNATE call by call in one process after a warm-up of each, until each has --seconds of timed work and at least
three calls (a path that has them drops out); host clock around work that ends in a device synchronise; medians and min - max.  Prints one
JSON line per measurement.  There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from slotformer_amd import annotations as ann  # noqa: E402
from slotformer_amd import configs, engine, harness  # noqa: E402
from slotformer_amd.ingest import FrameIngest  # noqa: E402
from slotformer_amd.video_prediction import vp_utils  # noqa: E402


def blob_masks(rs, n, h, w):
    """n ellipses, as dense masks"""
    yy, xx = np.mgrid[:h, :w]
    out = []
    for _ in range(n):
        cy, cx, ry, rx = rs.randint(0, h), rs.randint(0, w), rs.randint(8, h // 4), rs.randint(8, w // 4)
        out.append((((yy - cy) / ry)**2 + ((xx - cx) / rx)**2 <= 1).astype(np.uint8))
    return out


def clevrer_annotations(B, T, h, w, n_obj, seed=0):
    rs = np.random.RandomState(seed)
    pool = [[ann.rle_of_mask(m) for m in blob_masks(rs, n_obj, h, w)] for _ in range(16)]   # 16 distinct frames, repeated
    return [[pool[(b * T + t) % len(pool)] for t in range(T)] for b in range(B)]


def dense_decode(obj):
    h, w = obj['size']
    runs = ann.rle_counts(obj)
    ends = np.cumsum(runs)
    flat = np.zeros(h * w, np.uint8)
    for j in range(1, len(runs), 2):
        flat[ends[j - 1]:ends[j]] = 1
    return np.ascontiguousarray(flat.reshape(w, h).T)


def host_ground_truth(frames, ingest, num):
    """what the reference's dataset does per frame, on the CPU (datasets/clevrer.py:101-125)"""
    masks, press, boxes = [], [], []
    for clip in frames:
        for f in clip:
            m = np.stack([dense_decode(o) for o in f], 0).astype(np.int32)
            m = np.concatenate([np.logical_not(np.any(m, axis=0))[None], m], 0)
            t = ingest.process_mask(m)
            obj = t[1:]
            obj = obj[obj.sum([-1, -2]) > 0]
            box = vp_utils.masks_to_boxes_w_empty_mask(obj)
            pad, pres = torch.zeros(num, 4), torch.zeros(num, dtype=torch.bool)
            pad[:box.shape[0]], pres[:box.shape[0]] = box, True
            masks.append(t.argmax(0))
            press.append(pres)
            boxes.append(pad)
    return torch.stack(masks), torch.stack(press), torch.stack(boxes)


def alternate(paths, seconds, sync):
    """paths: name -> callable.  Warm each, then alternate until every path has `seconds` of timed work."""
    for fn in paths.values():
        fn()
        fn()
    sync()
    times = {k: [] for k in paths}
    while any(sum(v) < seconds or len(v) < 3 for v in times.values()):
        for k, fn in paths.items():
            if sum(times[k]) >= seconds and len(times[k]) >= 3:
                continue   # (a path a thousand times slower than its neighbour has its second long before)
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[k].append(time.perf_counter() - t0)
    return {k: dict(median_ms=round(float(np.median(v)) * 1e3, 4), min_ms=round(min(v) * 1e3, 4), max_ms=round(max(v) * 1e3, 4), calls=len(v))
            for k, v in times.items()}


def build_model(dev):
    from slotformer_amd.base_slots import build_model as bb
    from slotformer_amd.video_prediction import build_model as bv
    torch.manual_seed(0)
    scfg = configs.savi_cfg(64, 7, iters=2, kernel_mlp=False, pred='mlp', rnn=False, kld='var-0.01')
    savi = bb(configs.ParamsView(scfg))
    path = os.path.join(tempfile.mkdtemp(), 'savi.pth')
    torch.save({'state_dict': savi.state_dict()}, path)
    rcfg = configs.rollout_cfg(7, 128, 6, 256, 4, 8, 1024, rollout_len=42, res=64)
    rcfg['dec_dict'] = dict(scfg['dec_dict'], dec_ckp_path=path)
    return bv(configs.ParamsView(rcfg)).eval().to(dev)


@torch.no_grad()
def per_batch_loop(model, slots, frames, gt, batch_size, L_):
    """the loop at the API before evaluate_video_prediction: pred_eval_step per batch, AverageMeter on the host"""
    dev, hist = model.device, model.history_len
    V, _, N, C = slots.shape
    sums, count = {}, 0
    for s in range(0, V, batch_size):
        e = min(s + batch_size, V)
        B = e - s
        clip = torch.empty(B, hist + L_, N, C, device=dev)
        clip[:, :hist].copy_(slots[s:e, :hist], non_blocking=True)
        engine.rollout(model.rollouter, clip, hist, L_)
        recon, _, _, seg = engine.savi_decode(model, clip[:, hist:].reshape(B * L_, N, C), want=('seg', ), seg_dtype=torch.uint8)
        R = recon.shape[-1]
        recon, seg = recon.view(B, L_, 3, R, R), seg.view(B, L_, R, R)
        step = vp_utils.pred_eval_step(frames[s:e, hist:hist + L_].to(dev, non_blocking=True).contiguous(), recon, None,
                                       gt['mask'][s:e, hist:hist + L_].to(dev), seg, gt['pres_mask'][s:e, hist:hist + L_].to(dev),
                                       gt['bbox'][s:e, hist:hist + L_].to(dev), vp_utils.masks_to_boxes(seg, model.num_slots))
        for k, vals in step.items():
            acc = sums.setdefault(k, [0.0] * L_)
            for t in range(L_):
                acc[t] += vals[t] * B
        count += B
    return {k: np.array(v) / count for k, v in sums.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--videos', type=int, default=32)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_vp_eval: needs a HIP device; nothing is measured without one')
    dev = torch.device('cuda:0')
    sync = lambda: torch.cuda.synchronize(dev)   # noqa: E731
    lines = []

    # (a) ground truth
    B, T, h, w, n_obj, res = 8, 48, 320, 480, 6, 64
    frames = clevrer_annotations(B, T, h, w, n_obj)
    ing = FrameIngest((res, res))
    t0 = time.perf_counter()
    packed = ann.pack_frames(frames)
    pack_ms = (time.perf_counter() - t0) * 1e3
    packed.on(dev)
    got = ann.ground_truth(packed, ing, device=dev)
    hm, hp, hb = host_ground_truth(frames, ing, 7)
    equal = bool(torch.equal(got['mask'].cpu().flatten(0, 1), hm) and torch.equal(got['pres_mask'].cpu().flatten(0, 1), hp) and
                 torch.equal(got['bbox'].cpu().flatten(0, 1), hb))
    r = alternate({'device': lambda: ann.ground_truth(packed, ing, device=dev, check=False),
                   'host_dense': lambda: host_ground_truth(frames, ing, 7),
                   'host_from_runs': lambda: ann.ground_truth(packed, ing)}, args.seconds, sync)
    lines.append(dict(measurement='ground_truth_8x48_320x480_to_64x64', frames=B * T, runs=int(len(packed.run_ends)), parse_pack_ms=round(pack_ms, 2),
                      device_equals_host=equal, **{f'{k}_{m}': v for k, d in r.items() for m, v in d.items()}))

    # (b) the loop
    model = build_model(dev)
    V, hist, L_ = args.videos, 6, 42
    rs = np.random.RandomState(1)
    slots = torch.from_numpy(rs.standard_normal((V, hist + L_, 7, 128)).astype(np.float32)).to(dev)
    vids = torch.from_numpy((rs.rand(V, hist + L_, 3, res, res) * 2 - 1).astype(np.float32)).to(dev)
    anno = clevrer_annotations(V, hist + L_, h, w, n_obj, seed=2)
    gt = {k: v.to(dev) for k, v in ann.ground_truth(anno, ing).items()}
    a = harness.evaluate_video_prediction(model, slots, vids, batch_size=8, gt=gt)
    b = per_batch_loop(model, slots, vids, gt, 8, L_)
    worst = max(float(np.nanmax(np.abs(a[k] - b[k]) / np.maximum(np.abs(b[k]), 1e-300))) for k in vp_utils.METRICS)
    r = alternate({'device_loop': lambda: harness.evaluate_video_prediction(model, slots, vids, batch_size=8, gt=gt),
                   'per_batch_download': lambda: per_batch_loop(model, slots, vids, gt, 8, L_)}, args.seconds, sync)
    # with annotations= the call also parses and packs V * 42 frames of run-length strings on the host (Python): timed by itself, three calls
    with_anno = []
    for _ in range(3):
        sync()
        t0 = time.perf_counter()
        harness.evaluate_video_prediction(model, slots, vids, batch_size=8, annotations=anno)
        with_anno.append(round((time.perf_counter() - t0) * 1e3, 2))
    lines.append(dict(measurement=f'loop_V{V}_b8_6+42_64x64', max_rel_difference=worst, device_loop_from_annotations_ms=with_anno,
                      **{f'{k}_{m}': v for k, d in r.items() for m, v in d.items()}))
    lines.append(dict(measurement='environment', device=torch.cuda.get_device_name(0), torch=torch.__version__))
    for ln in lines:
        print(json.dumps(ln))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            for ln in lines:
                f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
