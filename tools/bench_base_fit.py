"""Training the base models on resident frames: a step of `base_slots.fit` against the same step written by hand with the module calls, as
INTEGRATION.md spelled it before `fit` (profiles/base_fit.md).   python tools/bench_base_fit.py [--json PATH] [--seconds 1.0] [--windows 3] [--models savi,steve,dvae]

Shapes, the reference's per-GPU training batches:
  savi    stosavi_clevrer_params.py: 16 clips x 6 frames at 64 x 64, 7 slots of 128, residual-MLP predictor, stochastic kernels, clip_grad 0.05
  steve   steve_physion_params.py: 12 clips x 6 frames at 128 x 128, 6 slots of 192, vocabulary 4096, two rates, clip_grad 0.05; targets tokenised per step
  dvae    dvae_physion_params.py: 64 single frames at 128 x 128, vocabulary 4096

  fit     base_slots.fit on a uint8 table on the device: the batch gathered by index, every seed from (seed, step).  Timed as whole calls of one
          epoch, so the once-per-call host work (validation, schedule, upload, building FlatAdam) is in.
  loop    `model(batch)`, `calc_train_loss`, `backward()`, `FlatAdam.step()` with the rates computed on the host per step; the batch is ONE float
          tensor already on the device (no loader, no upload, no gather): the floor of what a hand-written loop costs.  StoSAVi's noise is the
          module's fresh torch.randn per frame, seeds come from torch's CPU generator, STEVE's step runs the no-grad encode for its masks.

Both run in ONE process in alternating windows of at least `--seconds` each, after a warm-up of each; a window ends in a device synchronise and is
timed with the host clock.  Per-step time = window time / steps; the median over the windows, with minimum and maximum; `loop_spread` is (max - min)
/ median of the loop's own windows, what `fit_over_loop` is to be read against; `fit_setup_per_call_ms` is a call of fit with epochs=0 on the
window's clips, the share of a fit window that is not steps.  Kernel launches per step come from a torch.profiler run of their
own.  No GPU: the tool fails, it measures nothing."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402

import golden_util as gu  # noqa: E402

SEED = 0
SHAPES = {'savi': dict(B=16, T=6, res=64, V=32, frames=16, lr=1e-4, clip=0.05, warmup=0.025),
          'steve': dict(B=12, T=6, res=128, V=24, frames=12, lr=1e-4, dec_lr=3e-4, clip=0.05, warmup=0.05),
          'dvae': dict(B=64, T=1, res=128, V=64, frames=8, lr=1e-3, clip=None, warmup=0.05)}


def build(kind, dev):
    from slotformer_amd.base_slots import build_model
    torch.manual_seed(1)
    if kind == 'savi':
        cfg = gu.TRAIN_SAVI
    elif kind == 'steve':
        from bench_train_steve import physion_cfg
        cfg = physion_cfg()
    else:
        cfg = dict(model='dVAE', vocab_size=4096)
    return build_model(gu.ParamsView(cfg)).to(dev).train()


class Loop:
    """The step as INTEGRATION.md wrote it before `fit`, on one batch that already lies on the device."""

    def __init__(self, kind, model, frames, sh, total):
        from slotformer_amd import train
        self.kind, self.model, self.sh, self.total, self.train, self.step = kind, model, sh, total, train, 0
        dev = frames.device
        cv = torch.arange(sh['B'], dtype=torch.int32, device=dev) % sh['V']
        img = train.clip_frames(frames, cv, torch.zeros_like(cv), 1, 0, sh['T'], 0.5, 0.5)
        self.batch = {'img': img}
        if kind == 'steve':
            self.opt = train.FlatAdam(train.steve_param_groups(model, sh['lr'], sh['dec_lr']), clip_grad=sh['clip'])
        else:
            self.opt = train.FlatAdam([p for p in model.parameters() if p.requires_grad], lr=sh['lr'], clip_grad=sh['clip'])

    def run(self, n):
        m, opt, sh, tr = self.model, self.opt, self.sh, self.train
        for _ in range(n):
            k = self.step % self.total
            if self.kind == 'steve':
                for g, peak in zip(opt.param_groups, (sh['lr'], sh['dec_lr'])):
                    g['lr'] = tr.warmup_cosine_lr(k, self.total, sh['warmup'] * self.total, peak)
            else:
                opt.lr = tr.warmup_cosine_lr(k, self.total, sh['warmup'] * self.total, sh['lr'], sh['lr'] * 0.01)
            opt.zero_grad()
            terms = m.calc_train_loss(self.batch, m(self.batch))
            if self.kind == 'savi':
                loss = terms['post_recon_loss'] + 1e-4 * terms['kld_loss']
            else:
                loss = terms['token_recon_loss' if self.kind == 'steve' else 'recon_loss']
            loss.backward()
            opt.step()
            self.step += 1


class Fit:
    def __init__(self, kind, model, frames, sh, clips):
        self.kind, self.model, self.frames, self.sh, self.clips = kind, model, frames, sh, clips

    def run(self, n, epochs=1):
        """n steps: one call of fit over the first n batches' worth of clips (epochs=0: the once-per-call host work alone)"""
        from slotformer_amd import base_slots as bs
        sh = self.sh
        bs.fit(self.model, self.frames, self.clips[:n * sh['B']], epochs, sh['B'], sh['lr'], SEED, sh['T'], warmup_pct=sh['warmup'],
               clip_grad=sh['clip'], dec_lr=sh.get('dec_lr'))


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4), 'windows': len(v)}


def launches_per_step(form, steps=2):
    """kernel launches per step and the ten kernel names with the most launches, from a torch.profiler run of `steps` steps"""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        form.run(steps)
        torch.cuda.synchronize()
    names = {}
    for e in prof.events():
        if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower():
            names[e.name] = names.get(e.name, 0) + 1
    total = sum(names.values())
    if not total:
        return None, {}
    return round(total / steps, 1), dict(sorted(((k[:70], round(v / steps, 1)) for k, v in names.items()), key=lambda kv: -kv[1])[:10])


def measure(kind, dev, seconds, windows):
    from slotformer_amd import base_slots as bs
    sh = SHAPES[kind]
    gen = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (sh['V'], sh['frames'], sh['res'], sh['res'], 3), dtype=torch.uint8, generator=gen).to(dev)
    clips = bs.clip_index(sh['V'], sh['frames'], sh['T'], 1, 'train')
    clips = clips.repeat(-(-16384 // clips.shape[0]), 1)   # enough clips for a window of a second: the table is revisited
    forms = {'fit': Fit(kind, build(kind, dev), frames, sh, clips), 'loop': Loop(kind, build(kind, dev), frames, sh, 1000)}
    n, times = {}, {k: [] for k in forms}
    for k, f in forms.items():   # warm-up, then how many steps make a window of `seconds`
        f.run(2)
        n[k] = min(max(2, int(seconds / (window(lambda: f.run(3)) / 3)) + 1), clips.shape[0] // sh['B'])
    while min(len(v) for v in times.values()) < windows:
        for k, f in forms.items():
            w = window(lambda: f.run(n[k]))
            if w < seconds and n[k] < clips.shape[0] // sh['B']:   # the probe was optimistic: a window shorter than asked for is not kept
                n[k] = min(int(1.3 * n[k] * seconds / w) + 1, clips.shape[0] // sh['B'])
                continue
            if len(times[k]) < windows:
                times[k].append(w / n[k] * 1e3)
    out = {'shape': {k: sh[k] for k in ('B', 'T', 'res')}, 'fit_step': stats(times['fit']), 'loop_step': stats(times['loop']), 'steps_per_window': n}
    for k, f in forms.items():
        out[k + '_launches_per_step'], out[k + '_kernels'] = launches_per_step(f)
    med = {k: statistics.median(v) for k, v in times.items()}
    out['fit_over_loop'] = round(med['fit'] / med['loop'], 4)
    out['loop_spread'] = round((max(times['loop']) - min(times['loop'])) / med['loop'], 4)
    setup = statistics.median(window(lambda: forms['fit'].run(n['fit'], epochs=0)) for _ in range(3)) * 1e3
    out['fit_setup_per_call_ms'] = round(setup, 3)
    out['fit_setup_per_step_ms'] = round(setup / n['fit'], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--models', default='savi,steve,dvae')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_base_fit: no GPU; nothing is measured without one')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__}
    for kind in a.models.split(','):
        res[kind] = measure(kind, dev, a.seconds, a.windows)
    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
