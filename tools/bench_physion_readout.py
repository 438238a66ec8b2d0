"""Physion readout measurements (profiles/physion_readout.md).   python tools/bench_physion_readout.py [--json PATH] [--md PATH] [--seconds 0.5]

On one GPU, at the reference shape (6 slots of 192, 192 features, max over pairs, 75 frames), the kernels of csrc/physion_readout.hip against a
torch-eager restatement of the same model in this project's own words (gathered pairs -> linear -> max over pairs -> linear -> max over time,
torch autograd, torch.optim.Adam) on the same device and the same seeded data:

  * a training step at B 64 (forward, score, backward, FlatAdam) on a device-resident set, batches picked by `video_index`;
  * an evaluation pass at B 128 (forward + the six thresholds);
  * the sweep of test_physion_vqa.py: 50 checkpoints x 6 thresholds over 1000 videos -- `physion_vqa.evaluate` (the slots read once per batch)
    against eager run the reference's way (one full pass per checkpoint AND threshold) and against eager with one pass per checkpoint;
  * the forward kernel alone at B 64 (50 launches back to back on the C entry point, so that the wrapper's host time is not counted) against its
    count: 2 * (B T N) * C * 2F FLOPs x 3 split-bf16 passes at the dense bf16 MFMA peak, and the
    slots' bytes at the HBM peak.

The two paths alternate call by call after a warm-up of each, timed with device events until each has run for `--seconds`; medians, with the
minimum and maximum.  No GPU: the tool fails, it measures nothing."""
import argparse
import json
import os
import statistics
import sys
from itertools import combinations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as tnf  # noqa: E402

N, C, F, T = 6, 192, 192, 75
THRESHS = (0.4, 0.45, 0.5, 0.55, 0.6, 0.65)
PEAK_BF16_TFLOPS, PEAK_HBM_TBS = 2500.0, 8.0   # MI355X data sheet: dense bf16 matrix rate, HBM3E bandwidth


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, seconds, min_calls=5, max_calls=2000):
    """{name: [ms, ...]} of the callables run in turn until every one has run for `seconds`."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    while (min(sum(v) for v in ts.values()) < seconds * 1e3 or len(next(iter(ts.values()))) < min_calls) and len(next(iter(ts.values()))) < max_calls:
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    return ts


def stats(v):
    return {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4), 'calls': len(v)}


class EagerReadout(torch.nn.Module):
    """The same model on torch operators: every slot pair gathered, as the reference runs it."""

    def __init__(self):
        super().__init__()
        self.linear1, self.linear2 = torch.nn.Linear(2 * C, F), torch.nn.Linear(F, 1)
        pi, pj = torch.tensor(list(combinations(range(N), 2))).T
        self.register_buffer('pi', pi)
        self.register_buffer('pj', pj)

    def forward(self, slots):
        pairs = torch.cat([slots[:, :, self.pi], slots[:, :, self.pj]], -1)
        return self.linear2(self.linear1(pairs).max(2).values).squeeze(-1).max(1).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None)
    ap.add_argument('--seconds', type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_physion_readout: no GPU; nothing is measured without one')
    from slotformer_amd import ops, physion_vqa
    from slotformer_amd.physion_vqa.models import PhysionReadout
    from slotformer_amd.train import FlatAdam
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(0)
    V = 1000
    slots = torch.randn(V, T, N, C, generator=gen).to(dev)
    labels = (torch.rand(V, generator=gen) > 0.5).float().to(dev)
    torch.manual_seed(0)
    eager = EagerReadout().to(dev)
    native = PhysionReadout().to(dev)
    native.load_state_dict({'comb_idx': native.comb_idx, **{k: v for k, v in eager.state_dict().items() if k.startswith('linear')}})
    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'shape': dict(N=N, C=C, F=F, T=T)}

    # ---- training step, B 64 ----
    B = 64
    idx = torch.randperm(V, generator=gen)[:B].to(dev)
    idx32 = idx.to(torch.int32)
    params = [native.linear1.weight, native.linear1.bias, native.linear2.weight, native.linear2.bias]
    opt = FlatAdam(params, lr=1e-3)
    grad = torch.zeros(sum(p.numel() for p in params), device=dev)
    off = 0
    for p in params:
        p.grad = grad[off:off + p.numel()].view_as(p)
        off += p.numel()
    lab_b = labels[idx]

    @torch.no_grad()
    def native_step():
        W1, b1, w2, b2 = params
        logits, t_star, _, pairs = ops.physion_readout_fwd(slots, W1, b1, w2, b2, 'max', video_index=idx32, want_pairs=True)
        _, g, _, _ = ops.physion_readout_score(logits, lab_b)
        ops.physion_readout_bwd(slots, W1, b1, w2, g, t_star, 'max', pair_star=pairs, video_index=idx32, out=grad)
        opt.step()

    eopt = torch.optim.Adam(eager.parameters(), lr=1e-3)

    def eager_step():
        loss = tnf.binary_cross_entropy_with_logits(eager(slots[idx]), lab_b)
        eopt.zero_grad(set_to_none=True)
        loss.backward()
        eopt.step()

    ts = alternate({'native': native_step, 'eager': eager_step}, a.seconds)
    res['train_step_B64'] = {k: stats(v) for k, v in ts.items()}

    # ---- the forward kernel alone against its count ----
    W1, b1, w2, b2 = [p.detach() for p in params]
    from slotformer_amd._lib import lib, check
    out_l, out_t = torch.empty(1, B, device=dev), torch.empty(1, B, dtype=torch.int32, device=dev)
    w2r, stream, reps = w2.reshape(-1), torch.cuda.current_stream().cuda_stream, 50

    def fwd():   # `reps` launches back to back straight on the C entry point: the wrapper's host time (allocations, checks) is not the kernel's
        for _ in range(reps):
            check(lib().sf_physion_readout_fwd_f32(slots.data_ptr(), slots.stride(0), slots.stride(1), V, idx32.data_ptr(), W1.data_ptr(), b1.data_ptr(),
                                                   w2r.data_ptr(), b2.data_ptr(), out_l.data_ptr(), out_t.data_ptr(), None, None, 1, B, T, N, C, F, 0,
                                                   stream))

    ts = alternate({'forward_kernel': fwd}, a.seconds)
    ts['forward_kernel'] = [t / reps for t in ts['forward_kernel']]
    flops, nbytes = 2.0 * B * T * N * C * 2 * F, 4.0 * B * T * N * C
    st = stats(ts['forward_kernel'])
    least_us = max(3 * flops / (PEAK_BF16_TFLOPS * 1e12), nbytes / (PEAK_HBM_TBS * 1e12)) * 1e6
    st.update(gflop=round(flops / 1e9, 2), slot_mbytes=round(nbytes / 1e6, 1), least_us_at_peak=round(least_us, 2),
              measured_over_least=round(st['median_ms'] * 1e3 / least_us, 1), tflops_x3=round(3 * flops / st['median_ms'] / 1e9, 1))
    res['forward_B64'] = st

    # ---- evaluation pass, B 128 ----
    B = 128
    eidx = torch.arange(B, dtype=torch.int32, device=dev)
    th = torch.tensor(THRESHS, device=dev)

    @torch.no_grad()
    def native_eval():
        logits = ops.physion_readout_fwd(slots, W1, b1, w2, b2, 'max', video_index=eidx)[0]
        ops.physion_readout_score(logits, labels[:B], threshs=THRESHS, want_grad=False)

    @torch.no_grad()
    def eager_eval():
        p = torch.sigmoid(eager(slots[:B]))
        ((p[None] > th[:, None]).float() == labels[:B]).sum(1)

    ts = alternate({'native': native_eval, 'eager': eager_eval}, a.seconds)
    res['eval_pass_B128'] = {k: stats(v) for k, v in ts.items()}

    # ---- 50 checkpoints x 6 thresholds over 1000 videos ----
    K = 50
    sds = []
    for k in range(K):
        torch.manual_seed(100 + k)
        sds.append({k_: v.to(dev) for k_, v in PhysionReadout().state_dict().items()})

    def native_sweep():
        physion_vqa.evaluate(sds, slots, labels, threshs=THRESHS, batch_size=128)

    @torch.no_grad()
    def eager_probs(sd):
        eager.load_state_dict(sd, strict=False)
        return torch.cat([torch.sigmoid(eager(slots[s:s + 128])) for s in range(0, V, 128)])

    @torch.no_grad()
    def eager_sweep_reference_way():   # test_physion_vqa.py: the whole set once per checkpoint AND threshold
        for t in THRESHS:
            for sd in sds:
                ((eager_probs(sd) > t).float() == labels).float().mean()

    @torch.no_grad()
    def eager_sweep_one_pass_per_checkpoint():
        for sd in sds:
            p = eager_probs(sd)
            ((p[None] > th[:, None]).float() == labels).float().mean(1)

    ts = alternate({'native_evaluate': native_sweep, 'eager_pass_per_checkpoint': eager_sweep_one_pass_per_checkpoint}, a.seconds, min_calls=3)
    ts['eager_pass_per_checkpoint_and_threshold'] = [timed(eager_sweep_reference_way) for _ in range(2)]
    res['sweep_50x6_V1000'] = {k: stats(v) for k, v in ts.items()}

    def ratio(d, a_, b_):
        return round(d[b_]['median_ms'] / d[a_]['median_ms'], 2)

    res['eager_over_native'] = {'train_step_B64': ratio(res['train_step_B64'], 'native', 'eager'), 'eval_pass_B128': ratio(res['eval_pass_B128'], 'native', 'eager'),
                                'sweep_vs_pass_per_checkpoint': ratio(res['sweep_50x6_V1000'], 'native_evaluate', 'eager_pass_per_checkpoint'),
                                'sweep_vs_reference_way': ratio(res['sweep_50x6_V1000'], 'native_evaluate', 'eager_pass_per_checkpoint_and_threshold')}
    text = json.dumps(res, indent=1)
    print(text)
    for path in (a.json, ):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'w') as f:
                f.write(text + '\n')
    if a.md:
        rows = ['| measurement | path | median ms | min - max ms | calls |', '|---|---|---|---|---|']
        for sec in ('train_step_B64', 'eval_pass_B128', 'sweep_50x6_V1000'):
            for k, s in res[sec].items():
                rows.append(f"| {sec} | {k} | {s['median_ms']} | {s['min_ms']} - {s['max_ms']} | {s['calls']} |")
        s = res['forward_B64']
        rows.append(f"| forward_B64 | kernel | {s['median_ms']} | {s['min_ms']} - {s['max_ms']} | {s['calls']} |")
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, 'w') as f:
            f.write(f"Measured by `tools/bench_physion_readout.py` on {res['device']} (torch {res['torch']}).\n\n" + '\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
