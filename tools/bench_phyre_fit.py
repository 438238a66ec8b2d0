"""Training step of the PHYRE readout: `phyre_planning.fit`'s step against the same step on the nodes the project had before it and against torch
eager (profiles/phyre_fit.md).   python tools/bench_phyre_fit.py [--json PATH] [--seconds 1.0] [--windows 3] [--batches 256,64]

Shape: the reference's run (readout_phyre_params-fold0.py) -- batches of 256 (and 64), 8 slots of 128 at 2 frames (L = 17 tokens), 4 pre-LN layers
of d 128, 8 heads, FFN 512, dropout 0.1, Adam.  1024 videos x 4 frames on the device, batches picked by index.

  fused    fit's step: ops.phyre_readout_train_fwd (one launch per layer), the score launch, ops.phyre_readout_train_bwd (one launch per layer for
           the activation gradients) writing into FlatAdam's bucket, FlatAdam.step(gathered=True).
  nodes    the same step on the existing autograd nodes: the batch gathered on the device, train.linear(in_proj) + position row + CLS (no entry
           point hands out ph_embed's rows alone), train.transformer_encoder_layer x 4, train.linear(cls_mlp[0], relu), the 128 -> 1 row of
           cls_mlp[2] through torch (the linear node takes widths that are multiples of 64), train.readout_loss, backward(), FlatAdam.step().
  eager    the module's own nn.TransformerEncoder / nn.Linear layers under torch autograd on the same GPU, torch.optim.Adam: the reference module
           restated (the reference's class is not part of this repository).

All three run in ONE process in alternating windows of at least `--seconds` each, after a warm-up of each; a window ends in a device synchronise
and is timed with the host clock.  Per-step time = window time / steps; the median over the windows, with minimum and maximum.  The kernel
launches per step of `fused` and `nodes` are counted in a torch.profiler run of their own (8 steps each, outside the timed windows).
No GPU: the tool fails, it measures nothing."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

V, T_ALL, N, C = 1024, 4, 8, 128
RD = dict(num_slots=N, slot_size=C, t_pe='sin', d_model=128, num_layers=4, num_heads=8, ffn_dim=512, norm_first=True, sel_slots=[0, 3])
LR = 1e-3


def build(dev):
    from slotformer_amd.phyre_planning.models import PHYREReadout
    torch.manual_seed(1)
    return PHYREReadout(dict(RD)).to(dev).train()


class Fused:
    def __init__(self, slots, labels, B):
        from slotformer_amd import ops, phyre_planning, train
        self.m = build(slots.device)
        self.opt = train.FlatAdam(train.phyre_readout_parameters(self.m), lr=LR)
        self.model, self.keep = train.phyre_readout_model(self.m)
        self.slots, self.labels, self.B, self.step, self.ws = slots, labels, B, 0, None
        self.idx = [torch.randperm(V, generator=torch.Generator().manual_seed(k))[:B].to(torch.int32).to(slots.device) for k in range(8)]
        self.lab = [labels[i.long()] for i in self.idx]
        self.ops, self.seed_of = ops, phyre_planning.step_seed

    def run(self, n):
        ops = self.ops
        for _ in range(n):
            k, s = self.step % 8, self.seed_of(0, self.step)
            logits, self.ws, _, _ = ops.phyre_readout_train_fwd(self.model, self.slots, RD['sel_slots'], video_index=self.idx[k], p=0.1, seed=s, ws=self.ws)
            _, g, _, _ = ops.physion_readout_score(logits, self.lab[k])
            ops.phyre_readout_train_bwd(self.model, self.slots, RD['sel_slots'], g, self.ws, video_index=self.idx[k], p=0.1, seed=s, out=self.opt.grad)
            self.opt.step(gathered=True)
            self.step += 1


class Nodes:
    def __init__(self, slots, labels, B):
        from slotformer_amd import train
        self.m = build(slots.device)
        self.opt = train.FlatAdam(train.phyre_readout_parameters(self.m), lr=LR)
        self.slots, self.labels, self.B, self.step, self.train = slots, labels, B, 0, train
        self.idx = [torch.randperm(V, generator=torch.Generator().manual_seed(k))[:B].to(slots.device) for k in range(8)]
        self.lab = [labels[i] for i in self.idx]

    def run(self, n):
        m, tr = self.m, self.train
        for _ in range(n):
            k = self.step % 8
            x = self.slots[self.idx[k]][:, RD['sel_slots']]                               # [B, T, N, C] gathered
            tok = tr.linear(x.reshape(-1, C), m.in_proj).view(self.B, 2, N, -1) + m.enc_t_pe[0][None, :, None, :]
            x = torch.cat([m.CLS.expand(self.B, 1, -1), tok.flatten(1, 2)], 1)
            for layer in m.transformer_encoder.layers:
                x = tr.transformer_encoder_layer(x, layer)
            h = tr.linear(x[:, 0].contiguous(), m.cls_mlp[0], relu=True)
            logits = F.linear(h, m.cls_mlp[2].weight, m.cls_mlp[2].bias)[:, 0]
            loss = tr.readout_loss(logits, self.lab[k])
            self.opt.zero_grad()
            loss.backward()
            self.opt.step()
            self.step += 1


class Eager:
    def __init__(self, slots, labels, B):
        self.m = build(slots.device)
        self.opt = torch.optim.Adam(self.m.parameters(), lr=LR)
        self.slots, self.labels, self.B, self.step = slots, labels, B, 0
        self.idx = [torch.randperm(V, generator=torch.Generator().manual_seed(k))[:B].to(slots.device) for k in range(8)]
        self.lab = [labels[i] for i in self.idx]

    def run(self, n):
        m = self.m
        for _ in range(n):
            k = self.step % 8
            x = self.slots[self.idx[k]][:, RD['sel_slots']]
            tok = m.in_proj(x) + m.enc_t_pe[0][None, :, None, :]
            x = torch.cat([m.CLS.expand(self.B, 1, -1), tok.flatten(1, 2)], 1)
            logits = m.cls_mlp(m.transformer_encoder(x)[:, 0])[:, 0]
            loss = F.binary_cross_entropy_with_logits(logits, self.lab[k])
            self.opt.zero_grad()
            loss.backward()
            self.opt.step()
            self.step += 1


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4), 'windows': len(v)}


def launches_per_step(form, steps=8):
    """kernel launches per step, from a torch.profiler run of `steps` steps; None when the profiler records no kernels here"""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        form.run(steps)
        torch.cuda.synchronize()
    names, us = {}, {}
    for e in prof.events():
        if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower():
            names[e.name] = names.get(e.name, 0) + 1
            us[e.name] = us.get(e.name, 0.) + float(getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.) or 0.)
    total = sum(names.values())
    if not total:
        return None, {}
    # per kernel name: launches per step and device microseconds per step (the profiler's kernel durations), the twelve that hold the most time
    top = dict(sorted(((k[:60], [round(v / steps, 2), round(us[k] / steps, 1)]) for k, v in names.items()), key=lambda kv: -kv[1][1])[:12])
    return round(total / steps, 2), top


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--batches', default='256,64')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_phyre_fit: no GPU; nothing is measured without one')
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(0)
    slots = torch.randn(V, T_ALL, N, C, generator=gen).to(dev)
    labels = (torch.rand(V, generator=gen) > 0.5).float().to(dev)
    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'shape': dict(RD, videos=V, frames=T_ALL, dropout=0.1, tokens=17)}
    for B in [int(b) for b in a.batches.split(',')]:
        forms = {'fused': Fused(slots, labels, B), 'nodes': Nodes(slots, labels, B), 'eager': Eager(slots, labels, B)}
        n, times = {}, {k: [] for k in forms}
        for k, f in forms.items():   # warm-up, then how many steps make a window of `seconds`
            f.run(8)
            n[k] = max(8, int(a.seconds / (window(lambda: f.run(16)) / 16)) + 1)
        while min(len(v) for v in times.values()) < a.windows:
            for k, f in forms.items():
                w = window(lambda: f.run(n[k]))
                if w < a.seconds:   # the probe was optimistic: a window shorter than asked for is not kept
                    n[k] = int(1.3 * n[k] * a.seconds / w) + 1
                    continue
                if len(times[k]) < a.windows:
                    times[k].append(w / n[k] * 1e3)
        out = {k + '_step': stats(v) for k, v in times.items()}
        out['steps_per_window'] = n
        for k in ('fused', 'nodes'):
            out[k + '_launches_per_step'], out[k + '_kernels'] = launches_per_step(forms[k])
        med = {k: statistics.median(v) for k, v in times.items()}
        out['nodes_over_fused'] = round(med['nodes'] / med['fused'], 3)
        out['eager_over_fused'] = round(med['eager'] / med['fused'], 3)
        # "faster" only when the windows do not overlap
        out['fused_faster_than_nodes'] = bool(max(times['fused']) < min(times['nodes']))
        res[f'B{B}'] = out
    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
