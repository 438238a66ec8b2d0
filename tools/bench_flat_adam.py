"""The optimiser step alone, with gradient clipping, at the parameter counts of StoSAVi, SlotFormer (CLEVRER) and STEVE (Physion):

  (a) what clipping costs without FlatAdam's own: torch.nn.utils.clip_grad_norm_(params, 0.05), then FlatAdam.step()
  (b) FlatAdam(..., clip_grad=0.05).step()  -- gather + sf_grad_clip_coef_f32 + sf_adam_flat_groups_f32

on the same gradients (restored before every step, outside the timed window), HIP events around each step, the two
alternating, median of --steps steps after --warmup.  Also the two library kernels on their own (events around a run of
back-to-back launches) with their bytes per second: 4 bytes per element for the norm, 28 for the update (parameter and the two
moments read and written, gradient read).

  python tools/bench_flat_adam.py [--steps 40] [--warmup 5] [--out profiles/flat_adam.md]

Prints one JSON line and writes the table.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

import golden_util as gu  # noqa: E402

HBM_BYTES_PER_S = 8e12   # what the project prices HBM at
CLIP = 0.05


def model_shapes():
    """name -> the shapes of the trainable parameters (built on the CPU: only the shapes are used)."""
    from slotformer_amd.base_slots import build_model
    from bench_train import build as build_slotformer
    from bench_train_steve import physion_cfg
    out = {}
    out['StoSAVi (CLEVRER)'] = [tuple(p.shape) for p in build_model(gu.ParamsView(gu.TRAIN_SAVI)).parameters() if p.requires_grad]
    m, _ = build_slotformer(torch.device('cpu'), 10)
    out['SlotFormer-C2 (CLEVRER)'] = [tuple(p.shape) for p in m.parameters() if p.requires_grad]
    out['STEVE (Physion)'] = [tuple(p.shape) for p in build_model(gu.ParamsView(physion_cfg())).parameters() if p.requires_grad]
    return out


def _params(shapes, dev, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).to(dev)) for s in shapes]


def _timed(fn, restore):
    restore()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3   # us


def bench_model(shapes, dev, steps, warmup):
    from slotformer_amd import train, _lib
    pa, pb = _params(shapes, dev, 1), _params(shapes, dev, 1)
    n = sum(p.numel() for p in pa)
    g = torch.Generator(device='cpu').manual_seed(2)
    master = [(torch.randn(s, generator=g) * 0.1).to(dev) for s in shapes]
    for ps in (pa, pb):
        for p, m in zip(ps, master):
            p.grad = m.clone()
    opt_a = train.FlatAdam(pa, lr=1e-4)
    opt_b = train.FlatAdam(pb, lr=1e-4, clip_grad=CLIP)

    def restore(ps):
        def f():
            torch._foreach_copy_([p.grad for p in ps], master)
        return f

    def step_a():
        torch.nn.utils.clip_grad_norm_(pa, CLIP)
        opt_a.step()

    ta, tb = [], []
    for i in range(warmup + steps):
        a, b = _timed(step_a, restore(pa)), _timed(opt_b.step, restore(pb))
        if i >= warmup:
            ta.append(a)
            tb.append(b)
    # the two kernels alone, back to back
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    grp = (_lib.sf_adam_group * 1)()
    grp[0].begin, grp[0].lr = 0, 1e-4
    reps = 50

    def run(fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    t_norm = run(lambda: _lib.check(lib.sf_grad_clip_coef_f32(opt_b.grad.data_ptr(), n, CLIP, opt_b._clip_out.data_ptr(),
                                                              opt_b._clip_ws.data_ptr(), opt_b._clip_ws.numel(), st)))
    t_adam = run(lambda: _lib.check(lib.sf_adam_flat_groups_f32(opt_b.flat.data_ptr(), opt_b.grad.data_ptr(), opt_b.exp_avg.data_ptr(),
                                                                opt_b.exp_avg_sq.data_ptr(), n, 7, grp, 1, 0.9, 0.999, 1e-8,
                                                                opt_b._clip_out.data_ptr() + 4, st)))
    t_plain = run(lambda: _lib.check(lib.sf_adam_flat_f32(opt_a.flat.data_ptr(), opt_a.grad.data_ptr(), opt_a.exp_avg.data_ptr(),
                                                          opt_a.exp_avg_sq.data_ptr(), n, 7, 1e-4, 0.9, 0.999, 1e-8, st)))
    return {'tensors': len(shapes), 'elements': n, 'a_us': round(statistics.median(ta), 1), 'b_us': round(statistics.median(tb), 1),
            'a_min_us': round(min(ta), 1), 'b_min_us': round(min(tb), 1), 'norm_us': round(t_norm, 2), 'adam_groups_us': round(t_adam, 2),
            'adam_plain_us': round(t_plain, 2), 'norm_bytes_per_s': 4 * n / (t_norm * 1e-6), 'adam_bytes_per_s': 28 * n / (t_adam * 1e-6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flat_adam.md'))
    a = ap.parse_args()
    if a.steps < 30:
        raise SystemExit('at least 30 timed steps')
    if not torch.cuda.is_available():
        raise SystemExit('bench_flat_adam needs a HIP device: it measures, and there is nothing to measure without one')
    dev = torch.device('cuda:0')
    res = {name: bench_model(shapes, dev, a.steps, a.warmup) for name, shapes in model_shapes().items()}
    lines = ['# FlatAdam: the optimiser step with gradient clipping', '',
             f'`python tools/bench_flat_adam.py --steps {a.steps} --warmup {a.warmup}` on {torch.cuda.get_device_name(0)}: HIP events around each',
             'step, (a) and (b) alternating on the same gradients, median (minimum) of the timed steps, microseconds.', '',
             '- (a) `torch.nn.utils.clip_grad_norm_(params, 0.05)` then `FlatAdam.step()`',
             '- (b) `FlatAdam(..., clip_grad=0.05).step()`: gather, `sf_grad_clip_coef_f32`, `sf_adam_flat_groups_f32`', '',
             '| model | tensors | elements | (a) us | (b) us | (b) / (a) |', '|---|---|---|---|---|---|']
    for name, r in res.items():
        lines.append(f"| {name} | {r['tensors']} | {r['elements']} | {r['a_us']} ({r['a_min_us']}) | {r['b_us']} ({r['b_min_us']}) | "
                     f"{r['b_us'] / r['a_us']:.2f} |")
    lines += ['', 'The kernels alone (50 back-to-back launches between two events, so launch gaps are inside; buckets of this size stay in the',
              'cache hierarchy between launches, so the rates are not HBM rates), bytes per second against the 8 TB/s HBM is priced at:', '',
              '| model | norm us | norm TB/s (share) | update us | update TB/s (share) | plain `sf_adam_flat_f32` us |', '|---|---|---|---|---|---|']
    for name, r in res.items():
        lines.append(f"| {name} | {r['norm_us']} | {r['norm_bytes_per_s'] / 1e12:.2f} ({r['norm_bytes_per_s'] / HBM_BYTES_PER_S:.0%}) | "
                     f"{r['adam_groups_us']} | {r['adam_bytes_per_s'] / 1e12:.2f} ({r['adam_bytes_per_s'] / HBM_BYTES_PER_S:.0%}) | {r['adam_plain_us']} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps({'metric': 'flat_adam_clipped_step_us', 'models': res}))


if __name__ == '__main__':
    main()
