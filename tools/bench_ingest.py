"""Ingest measurements (profiles/ingest.md).   python tools/bench_ingest.py [--batches 20] [--skip-pipeline] [--json PATH]

(a) sf_ingest_frames_u8 alone at 32 x 6 frames: 320 x 480 -> 128 x 128 (CLEVRER), 128 x 128 -> 128 x 128 and 256 x 256 colour indices -> 128 x 128
    (PHYRE), both resampling modes: microseconds, and bytes moved / time as a fraction of the rate of a device-to-device copy that moves the same
    number of bytes, measured in the same run.  Inputs rotate through enough buffers to exceed the 256 MiB last-level cache.
(b) harness.extract_and_rollout(to_host=True) at C2 from pinned float32 frames (the path without ingest) against pinned uint8 128 x 128 frames with
    ingest=, same process, alternating, median of five; then one traced run of each (SF_PIPE_TRACE) for the encode lane's time per batch.
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


def kernel_alone(dev):
    from slotformer_amd.ingest import FrameIngest
    F = 32 * 6
    rows = []
    pal = torch.randint(0, 256, (7, 3), dtype=torch.uint8)
    for name, shape, palette in (('320x480 -> 128x128 (CLEVRER)', (320, 480, 3), None), ('128x128 -> 128x128', (128, 128, 3), None),
                                 ('256x256 indices -> 128x128 (PHYRE)', (256, 256), pal)):
        in_bytes = F * int(torch.tensor(shape).prod())
        out_bytes = F * 3 * 128 * 128 * 4
        moved = in_bytes + out_bytes
        n_bufs = max(2, -(-(300 << 20) // moved))
        hi = 7 if palette is not None else 256
        srcs = [torch.randint(0, hi, (F, ) + shape, dtype=torch.uint8, device=dev) for _ in range(n_bufs)]
        outs = [torch.empty(F, 3, 128, 128, device=dev) for _ in range(n_bufs)]
        # the copy that moves the same bytes: moved / 2 read + moved / 2 written
        ca = [torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(n_bufs)]
        cb = [torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(n_bufs)]
        t_copy = time_us(lambda i: cb[i].copy_(ca[i]), n_bufs)
        for aa in (False, True):
            ing = FrameIngest((128, 128), antialias=aa, palette=palette)
            t = time_us(lambda i: ing.ingest(srcs[i], out=outs[i]), n_bufs)
            rows.append({'case': name, 'antialias': aa, 'us': round(t, 1), 'bytes_moved': moved, 'GB_per_s': round(moved / t / 1e3, 1),
                         'copy_us': round(t_copy, 1), 'copy_GB_per_s': round(moved / t_copy / 1e3, 1), 'fraction_of_copy_rate': round(t_copy / t, 3)})
            print(rows[-1], flush=True)
        del srcs, outs, ca, cb
    return rows


def pipeline_pair(dev, n):
    import bench
    from slotformer_amd import harness
    from slotformer_amd.ingest import FrameIngest
    cfg = bench.bench_configs()['C2']
    savi, roll = bench.build_models(dev, cfg)[:2]
    B, T, H = cfg[3], cfg[4], cfg[5]
    u8 = torch.randint(0, 256, (n * B, T, 128, 128, 3), dtype=torch.uint8).pin_memory()
    ing = FrameIngest((128, 128))
    f32 = ing.ingest(u8.to(dev)).cpu().pin_memory()      # the same pictures, as today's callers hand them over

    def call(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == 'float32':
            out = harness.extract_and_rollout(savi, roll, f32, H, batch_size=B, to_host=True)
        else:
            out = harness.extract_and_rollout(savi, roll, u8, H, batch_size=B, to_host=True, ingest=ing)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for kind in ('float32', 'uint8+ingest', 'float32', 'uint8+ingest'):   # warm-up: graphs, rings, tables
        call(kind)
    ms = {'float32': [], 'uint8+ingest': []}
    outs = {}
    for _ in range(5):
        for kind in ms:
            t, outs[kind] = call(kind)
            ms[kind].append(t)
    res = {'config': 'C2', 'batches': n, 'videos_per_batch': B, 'frames': n * B * (T + H)}
    for kind, v in ms.items():
        med = statistics.median(v)
        res[kind] = {'ms': [round(x, 2) for x in v], 'median_ms': round(med, 2), 'spread_ms': round(max(v) - min(v), 2),
                     'k_frames_per_s': round(n * B * (T + H) / med, 1)}
    # one traced run each: the encode lane's period in the steady state (batches behind the fill)
    os.environ['SF_PIPE_TRACE'] = '1'
    try:
        for kind in ms:
            call(kind)
            tl = next(iter(harness._PIPES.values()))[2].timeline
            ends = tl['encode_end_ms']
            steady = [b - a for a, b in zip(ends[len(ends) // 2:-1], ends[len(ends) // 2 + 1:])]
            res[kind]['encode_end_ms'] = [round(x, 2) for x in ends]
            res[kind]['rollout_end_ms'] = [round(x, 2) for x in tl['rollout_end_ms']]
            res[kind]['encode_period_ms_second_half'] = round(statistics.median(steady), 3) if steady else None
    finally:
        os.environ.pop('SF_PIPE_TRACE', None)
        harness.release_pipelines()
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--skip-pipeline', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = {'kernel_alone': kernel_alone(dev)}
    if not a.skip_pipeline:
        res['pipeline'] = pipeline_pair(dev, a.batches)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
