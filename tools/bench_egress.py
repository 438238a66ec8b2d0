"""Egress measurements (profiles/egress.md).   python tools/bench_egress.py [--batches 20] [--skip-pipeline] [--json PATH]

(a) the three kernels of csrc/egress.hip alone at 32 x 50 frames of 128 x 128 and of 64 x 64: sf_egress_frames_u8 (HWC and CHW), sf_egress_grid (the
    slot-decomposition grid of 7 slots, uint8 HWC) and sf_egress_draw_boxes (7 boxes per frame): microseconds, and bytes moved / time as a fraction
    of the rate of a device-to-device copy that moves the same number of bytes, measured in the same run (the convention of profiles/ingest.md).
    Inputs rotate through enough buffers to exceed the 256 MiB last-level cache.
(b) the decode pipeline at C2 with and without 'recon_u8' into pinned memory: EncodeRolloutPipeline.run(decoded=...) -- without the key the parent
    path unchanged (float32 'recon' for the whole run on the device) -- same process, alternating, median of five; and the rate of a plain pinned
    download of the uint8 bytes of one run, so that the expected cost (bytes / host-link rate) stands beside the measured difference.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def time_us(fn, n_bufs, iters=40, warmup=8):
    """median microseconds of fn(i % n_bufs) by device events, one launch per measurement"""
    for i in range(warmup):
        fn(i % n_bufs)
    torch.cuda.synchronize()
    ts = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i % n_bufs)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def _row(rows, case, t, moved, dev):
    n_bufs = max(2, -(-(300 << 20) // moved))
    ca = [torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(n_bufs)]
    cb = [torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(n_bufs)]
    t_copy = time_us(lambda i: cb[i].copy_(ca[i]), n_bufs)
    rows.append({'case': case, 'us': round(t, 1), 'bytes_moved': moved, 'GB_per_s': round(moved / t / 1e3, 1), 'copy_us': round(t_copy, 1),
                 'copy_GB_per_s': round(moved / t_copy / 1e3, 1), 'fraction_of_copy_rate': round(t_copy / t, 3)})
    print(rows[-1], flush=True)


def kernels_alone(dev):
    from slotformer_amd import egress
    F, N = 32 * 50, 7
    rows = []
    for R in (128, 64):
        px = F * R * R
        # (a1) frames: 12 bytes read + 3 written per pixel
        moved = px * 15
        nb = max(2, -(-(300 << 20) // moved))
        xs = [torch.rand(F, 3, R, R, device=dev) * 2 - 1 for _ in range(nb)]
        for layout in ('hwc', 'chw'):
            outs = [torch.empty((F, R, R, 3) if layout == 'hwc' else (F, 3, R, R), dtype=torch.uint8, device=dev) for _ in range(nb)]
            t = time_us(lambda i: egress.frames_to_uint8(xs[i], layout=layout, out=outs[i]), nb)
            _row(rows, f'frames_u8 {layout} {F} x {R}x{R}', t, moved, dev)
        # (a3) boxes: reads and writes only the groups an outline touches; the figure is the time alone, bytes = the frames once
        u8 = [torch.randint(0, 256, (F, 3, R, R), dtype=torch.uint8, device=dev) for _ in range(nb)]
        lo = torch.rand(F, N, 2, device=dev) * (R / 2)
        boxes = torch.cat([lo, lo + 8 + torch.rand(F, N, 2, device=dev) * (R / 2 - 8)], -1).contiguous()
        t = time_us(lambda i: egress.draw_boxes_(u8[i], boxes), nb)
        _row(rows, f'draw_boxes {N} per frame {F} x {R}x{R}', t, px * 3, dev)
        del xs, u8
        # (a2) the slot-decomposition grid of a 50-frame video x 32 videos as one T = 1600 launch: (2 + N) * 12 + N * 4 bytes read per pixel
        T = F // 4                                        # (a quarter of the frames: the slot tensors are N times the frames)
        CH, CW, _, _, _ = egress.grid_shape(N + 2, R, R, N + 2, 2, 0)
        moved = T * R * R * ((2 + N) * 12 + N * 4) + T * CH * CW * 3
        nb = max(2, -(-(300 << 20) // moved))
        sets = [(torch.rand(T, 3, R, R, device=dev) * 2 - 1, torch.rand(T, 3, R, R, device=dev) * 2 - 1, torch.rand(T, N, 3, R, R, device=dev) * 2 - 1,
                 torch.softmax(torch.randn(T, N, 1, R, R, device=dev), 1)) for _ in range(nb)]
        tiles = [[egress.Img(a), egress.Img(b), egress.Slots(r, m, 1.)] for a, b, r, m in sets]
        t = time_us(lambda i: egress.video_grid(tiles[i], nrow=N + 2, pad_value=0., dtype=torch.uint8, layout='hwc'), nb)
        _row(rows, f'grid {N + 2} tiles uint8 hwc {T} x {R}x{R}', t, moved, dev)
        del sets, tiles
    return rows


def pipeline_pair(dev, n):
    import bench
    from slotformer_amd import engine
    from slotformer_amd.pipeline import EncodeRolloutPipeline
    cfg = bench.bench_configs()['C2']
    savi, roll = bench.build_models(dev, cfg)[:2]
    B, T, H = cfg[3], cfg[4], cfg[5]
    R = engine.decoder_plan(savi).struct.resolution
    imgs = [torch.rand(B, T, 3, R, R, device=dev) * 2 - 1 for _ in range(n)]
    pipe = EncodeRolloutPipeline(savi, roll, B, T, H, decoder=savi)
    dec = {'float32 on device': {'recon': torch.empty(n, B, H, 3, R, R, device=dev), 'seg': torch.empty(n, B, H, R, R, dtype=torch.uint8, device=dev)},
           'recon_u8 pinned': {'recon_u8': torch.empty(n, B, H, R, R, 3, dtype=torch.uint8).pin_memory(),
                               'seg': torch.empty(n, B, H, R, R, dtype=torch.uint8).pin_memory()}}

    def call(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.run(imgs, decoded=dec[kind])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    try:
        for kind in list(dec) * 2:     # warm-up: graphs, buffers
            call(kind)
        ms = {k: [] for k in dec}
        for _ in range(5):
            for kind in ms:
                ms[kind].append(call(kind))
        res = {'config': 'C2', 'batches': n, 'videos_per_batch': B, 'decoded_frames': n * B * H, 'resolution': R}
        for kind, v in ms.items():
            med = statistics.median(v)
            res[kind] = {'ms': [round(x, 2) for x in v], 'median_ms': round(med, 2), 'spread_ms': round(max(v) - min(v), 2)}
        # the download alone: the uint8 frames + segmentations of one run, device -> pinned
        src = torch.empty(n * B * H * R * R * 4, dtype=torch.uint8, device=dev)
        dst = torch.empty(src.numel(), dtype=torch.uint8).pin_memory()
        t = time_us(lambda i: dst.copy_(src, non_blocking=True), 1, iters=5, warmup=2)
        res['download'] = {'bytes': src.numel(), 'us': round(t, 1), 'GB_per_s': round(src.numel() / t / 1e3, 2), 'expected_extra_ms': round(t / 1e3, 2)}
    finally:
        pipe.close()
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--skip-pipeline', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = {'kernels_alone': kernels_alone(dev)}
    if not a.skip_pipeline:
        res['pipeline'] = pipeline_pair(dev, a.batches)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
