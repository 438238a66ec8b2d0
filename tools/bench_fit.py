"""SlotFormer training on resident slots: a step of `video_prediction.fit` against the same step written with what the project had before it
(profiles/slotformer_fit.md).   python tools/bench_fit.py [--json PATH] [--seconds 1.0] [--windows 3] [--img 0|1|both]

Shape: the reference's CLEVRER run -- B 64, 6 burn-in + 10 predicted frames 2 apart, 7 slots of 128, d_model 256, 4 layers, 8 heads, FFN 1024,
dropout 0.1 -- without and with the image loss (the frozen 8x8 -> 64x64 decoder on the 640 predicted frames).  128 videos x 128 frames on the device.

  fit      video_prediction.fit: clips by index, the fused loss, the backward writing into the optimiser's bucket, FlatAdam.step(gathered=True).
           Timed as whole calls of one epoch (196 steps), so the once-per-call host work (validation, schedule, uploads, building FlatAdam) is in.
  module   the batch gathered on the device (advanced indexing; frames through FrameIngest), model(data), calc_train_loss, backward,
           FlatAdam.step(), zero_grad -- with the same schedule arithmetic (warmup_cosine_lr, the loss decay factor) on the host.

Both run in ONE process in alternating windows of at least `--seconds` each, after a warm-up of each; a window ends in a device synchronise and is
timed with the host clock.  Per-step time = window time / steps; the median over the windows, with minimum and maximum.

--count PATH K: run K steps of one path ('fit' or 'module', with --img 0|1) and exit -- for a kernel trace in a run of its own (the launches per
step are the difference of two such runs' kernel counts over the difference of their K).  No GPU: the tool fails, it measures nothing."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

V, T, N, C, HIST, S, F, B = 128, 128, 7, 128, 6, 10, 2, 64
ROLL = dict(num_slots=N, slot_size=C, history_len=HIST, t_pe='sin', slots_pe='', d_model=256, num_layers=4, num_heads=8, ffn_dim=1024, norm_first=True)
DEC = dict(dec_channels=(128, 64, 64, 64, 64), dec_resolution=(8, 8), dec_ks=5, dec_norm='')
LR, SEED = 2e-4, 0


def build_model(img, dev):
    """SlotFormer at the CLEVRER shape around a seeded decoder checkpoint (the decoder is frozen: its values do not matter to the time)."""
    from slotformer_amd.host import containers
    from slotformer_amd.base_slots.models.utils import SoftPositionEmbed
    from slotformer_amd.video_prediction.models import SlotFormer
    torch.manual_seed(1)
    dec, _ = containers.deconv_stack(DEC['dec_channels'], 5, '', 8, 64)
    pos = SoftPositionEmbed(C, (8, 8))
    sd = {'decoder.' + k: v for k, v in dec.state_dict().items()}
    sd.update({'decoder_pos_embedding.' + k: v for k, v in pos.state_dict().items()})
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'dec.pth')
        torch.save({'state_dict': sd}, path)
        model = SlotFormer((64, 64), HIST + S, slot_dict=dict(num_slots=N, slot_size=C), dec_dict=dict(DEC, dec_ckp_path=path), rollout_dict=dict(ROLL),
                           loss_dict=dict(rollout_len=S, use_img_recon_loss=bool(img)))
    return model.to(dev).train()


class ModulePath:
    """The training step as it was written before `fit`: gather on the device, the module's forward and loss, autograd, FlatAdam.step()."""

    def __init__(self, model, table, frames, clips, epochs):
        from slotformer_amd import train, video_prediction as vp
        from slotformer_amd.ingest import FrameIngest
        self.model, self.table, self.frames = model, table, frames
        dev = table.device
        self.sched = vp.clip_schedule(clips.shape[0], epochs, B, SEED)
        self.per_epoch = len(self.sched[0])
        self.total = self.per_epoch * epochs
        order = torch.stack([b for e in self.sched for b in e]).long()
        self.video = clips[:, 0][order].long().to(dev)
        self.start = clips[:, 1][order].long().to(dev)
        self.steps = torch.arange(HIST + S, device=dev) * F
        self.opt = train.FlatAdam(train.rollouter_parameters(model.rollouter), lr=LR)
        self.ingest = FrameIngest((64, 64)) if frames is not None else None
        self.step = 0
        self.train, self.vp = train, vp

    def run(self, n):
        m, opt = self.model, self.opt
        for _ in range(n):
            k = self.step % self.total
            v, t = self.video[k][:, None], self.start[k][:, None] + self.steps[None]
            data = {'slots': self.table[v, t]}
            if self.frames is not None:
                data['img'] = self.ingest.ingest(self.frames[v, t].contiguous())
            m.loss_decay_factor = self.vp.loss_decay_factor(k, self.total, 0.2)
            out = m(data)
            terms = m.calc_train_loss(data, out)
            loss = terms['slot_recon_loss'] + (terms['img_recon_loss'] if self.frames is not None else 0.)
            opt.zero_grad()
            loss.backward()
            opt.lr = self.train.warmup_cosine_lr(k, self.total, 0.05 * self.total, LR, LR * 0.01)
            opt.step()
            self.step += 1


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4), 'windows': len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--img', default='both')
    ap.add_argument('--count', nargs=2, default=None, metavar=('PATH', 'K'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fit: no GPU; nothing is measured without one')
    from slotformer_amd import video_prediction as vp
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(V, T, N, C, generator=gen).to(dev)
    frames_u8 = torch.randint(0, 256, (V, T, 64, 64, 3), dtype=torch.uint8, generator=gen).to(dev)
    clips = vp.clip_index(V, T, HIST + S, F, 'train')
    per_epoch = clips.shape[0] // B

    def fit_epochs(model, frames, clip_subset):
        return vp.fit(model, table, clip_subset, 1, B, LR, SEED, F, loss_decay_pct=0.2, frames=frames)

    if a.count:
        path, k = a.count[0], int(a.count[1])
        img = a.img == '1'
        model = build_model(img, dev)
        frames = frames_u8 if img else None
        if path == 'fit':
            fit_epochs(model, frames, clips[:B * k])
        else:
            ModulePath(model, table, frames, clips, 1).run(k)
        torch.cuda.synchronize()
        print(json.dumps({'path': path, 'img': img, 'steps': k}))
        return

    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__,
           'shape': dict(B=B, burn_in=HIST, pred=S, frame_offset=F, slots=N, slot_size=C, **{k: ROLL[k] for k in ('d_model', 'num_layers', 'num_heads', 'ffn_dim')}),
           'table': [V, T, N, C], 'clips': int(clips.shape[0]), 'steps_per_fit_call': per_epoch}
    for img in ([False, True] if a.img == 'both' else [a.img == '1']):
        frames = frames_u8 if img else None
        m_fit, m_mod = build_model(img, dev), build_model(img, dev)
        mod = ModulePath(m_mod, table, frames, clips, 1)
        # warm-up of each, at the shapes the windows use
        fit_epochs(m_fit, frames, clips[:B * 4])
        mod.run(4)
        # how many module steps make a window of `seconds`
        probe = window(lambda: mod.run(8)) / 8
        n_mod = max(8, int(a.seconds / probe) + 1)
        setup = [window(lambda: vp.fit(m_fit, table, clips, 0, B, LR, SEED, F, frames=frames)) * 1e3 for _ in range(3)]
        t_fit, t_mod = [], []
        while len(t_mod) < a.windows:
            w_fit = window(lambda: fit_epochs(m_fit, frames, clips))
            w_mod = window(lambda: mod.run(n_mod))
            if w_mod < a.seconds:   # the probe was optimistic: a window shorter than asked for is not kept
                n_mod = int(1.3 * n_mod * a.seconds / w_mod) + 1
                continue
            t_fit.append(w_fit / per_epoch * 1e3)
            t_mod.append(w_mod / n_mod * 1e3)
        key = 'with_image_loss' if img else 'slot_loss_only'
        res[key] = {'fit_step': stats(t_fit), 'module_step': stats(t_mod), 'fit_window_s': round(statistics.median(t_fit) * per_epoch / 1e3, 3),
                    'module_window_s': round(statistics.median(t_mod) * n_mod / 1e3, 3), 'module_steps_per_window': n_mod,
                    'fit_setup_per_call_ms': round(statistics.median(setup), 3),
                    'module_over_fit': round(statistics.median(t_mod) / statistics.median(t_fit), 3)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
