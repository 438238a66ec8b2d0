"""Training step of the Aloe reasoner: `clevrer_vqa.fit`'s step against torch eager on the same GPU (profiles/clevrer_vqa_fit.md).
    python tools/bench_clevrer_vqa_fit.py [--json PATH] [--seconds 1.0] [--windows 3] [--questions 128] [--layers 12]

Shape: the reference's run (aloe_clevrer_params.py) -- 25 frames of 7 slots of 128, 32 text positions (L = 208 tokens), 12 pre-LN layers of d 144 =
8 x 18, FFN 512, dropout 0.1, Adam -- at 128 QUESTIONS a step: 64 descriptive ones and 64 multiple-choice ones of three choices each, 256 sequences.
256 videos x 25 frames on the device, batches picked by index.

  native   fit's step: ops.aloe_train_fwd, the score-gradient launch, ops.aloe_train_bwd writing into FlatAdam's bucket, FlatAdam.step(gathered=True),
           the addition of the two losses into the epoch's means.
  eager    the module's own nn.TransformerEncoderLayer / nn.Linear / nn.Embedding layers under torch autograd with a key-padding mask,
           F.cross_entropy + F.binary_cross_entropy_with_logits, torch.optim.Adam: the reference module restated (the reference's class is not
           part of this repository).

Both run in ONE process in alternating windows of at least `--seconds` each, after a warm-up of each; a window ends in a device synchronise and is
timed with the host clock.  Per-step time = window time / steps; the median over the windows, with minimum and maximum.  Kernel launches per step
come from a torch.profiler run of their own, peak memory from torch's allocator statistics over a window.  No GPU: the tool fails, it measures nothing."""
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

V, T, N, C, TEXT, QLEN, VOCAB, ANSWERS, CHOICES = 256, 25, 7, 128, 32, 20, 82, 22, 3
LR = 1e-3


def build(dev, layers):
    from slotformer_amd.clevrer_vqa.models import CLEVRERTransformerModel
    torch.manual_seed(1)
    tm = CLEVRERTransformerModel(dict(input_len=T * N + TEXT, input_dim=16, pos_enc='learnable', num_layers=layers, num_heads=8, ffn_dim=512,
                                      norm_first=True, cls_mlp_size=128), dict(question_len=QLEN, question_vocab_size=VOCAB, answer_vocab_size=ANSWERS),
                                 dict(vision_dim=C), dict(use_mask_obj_loss=False))
    return tm.to(dev).train()


def batches(dev, questions, count=8):
    """`count` batches of questions // 2 descriptive sequences and questions // 2 x CHOICES choices; padding as the dataset pads"""
    out = []
    b1 = questions // 2
    bn = (questions - b1) * CHOICES
    for k in range(count):
        g = torch.Generator().manual_seed(100 + k)
        tokens = torch.randint(1, VOCAB, (b1 + bn, TEXT), generator=g)
        pad = torch.ones(b1 + bn, TEXT, dtype=torch.bool)
        for b in range(b1 + bn):
            pad[b, :int(torch.randint(6, QLEN + 1, (1, ), generator=g))] = False
            if b >= b1:
                pad[b, QLEN:QLEN + int(torch.randint(3, TEXT - QLEN + 1, (1, ), generator=g))] = False
        tokens[pad] = 0
        out.append(dict(tokens=tokens.to(dev).int(), pad_mask=pad.to(dev), B1=b1, video_index=torch.randint(0, V, (b1 + bn, ), generator=g).to(dev).int(),
                        start=torch.zeros(b1 + bn, dtype=torch.int32, device=dev), frame_offset=1,
                        cls_label=torch.randint(0, ANSWERS, (b1, ), generator=g).to(dev).int(), mc_label=(torch.rand(bn, generator=g) > 0.5).float().to(dev),
                        loss_share=torch.tensor([1. / count, 1. / count]).to(dev)))
        out[-1]['cls_label64'] = out[-1]['cls_label'].long()   # (what F.cross_entropy takes: converted ahead, not inside eager's step)
    return out


class Native:
    def __init__(self, slots, bs, layers):
        from slotformer_amd import clevrer_vqa, ops, train
        self.tm = build(slots.device, layers)
        self.opt = train.FlatAdam(train.aloe_parameters(self.tm), lr=LR)
        self.model, self.keep = train.aloe_model(self.tm, N, T, TEXT)
        self.slots, self.bs, self.step, self.ws, self.ops, self.seed_of = slots, bs, 0, None, ops, clevrer_vqa.step_seed
        self.epoch_loss = torch.zeros(2, dtype=torch.float32, device=slots.device)

    def run(self, n):
        ops = self.ops
        for _ in range(n):
            b, s = self.bs[self.step % len(self.bs)], self.seed_of(0, self.step)
            cls_logits, mc_logits, self.ws, _, _ = ops.aloe_train_fwd(self.model, self.slots, b, p=0.1, seed=s, ws=self.ws)
            loss, g_cls, g_mc = ops.aloe_score_grad(cls_logits, b['cls_label'], mc_logits, b['mc_label'])
            ops.aloe_train_bwd(self.model, self.slots, b, g_cls, g_mc, self.ws, p=0.1, seed=s, out=self.opt.grad)
            self.opt.step(gathered=True)
            self.step += 1
            self.epoch_loss += loss * b['loss_share']   # (fit's bookkeeping of the epoch means: part of its step)


class Eager:
    def __init__(self, slots, bs, layers):
        self.tm = build(slots.device, layers)
        self.opt = torch.optim.Adam([p for p in self.tm.parameters() if p.requires_grad], lr=LR)
        self.slots, self.bs, self.step = slots, bs, 0

    def run(self, n):
        tm = self.tm
        for _ in range(n):
            b = self.bs[self.step % len(self.bs)]
            B, b1 = b['tokens'].shape[0], b['B1']
            frames = self.slots[b['video_index'].long()][:, :T].flatten(1, 2)                                  # [B, T N, C] gathered
            v_rows = tm.vision_in_proj(torch.cat([frames, tm.vision_token.expand(B, T * N, 2)], -1))
            typ = tm.cls_token.expand(B, TEXT, 2).clone()
            typ[b1:, :QLEN] = tm.mc_question_token
            q_rows = tm.q_in_proj(torch.cat([tm.q_embedding(b['tokens'].long()), typ, tm.text_token.expand(B, TEXT, 2)], -1))
            x = torch.cat([tm.CLS.expand(B, 1, -1), v_rows, q_rows], 1) + tm.transformer_encoder.pos_enc
            mask = torch.cat([torch.zeros(B, 1 + T * N, dtype=torch.bool, device=x.device), b['pad_mask']], 1)
            for layer in tm.transformer_encoder.layers:
                x = layer(x, src_key_padding_mask=mask)
            loss = F.cross_entropy(tm.cls_answer_mlp(x[:b1, 0]), b['cls_label64']) + \
                F.binary_cross_entropy_with_logits(tm.mc_answer_mlp(x[b1:, 0])[:, 0], b['mc_label'])
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


def launches_per_step(form, steps=2):
    """kernel launches per step and the twelve kernel names that hold the most device time, from a torch.profiler run of `steps` steps"""
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
    top = dict(sorted(((k[:60], [round(v / steps, 2), round(us[k] / steps, 1)]) for k, v in names.items()), key=lambda kv: -kv[1][1])[:12])
    return round(total / steps, 2), top


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--questions', type=int, default=128)
    ap.add_argument('--layers', type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_clevrer_vqa_fit: no GPU; nothing is measured without one')
    dev = torch.device('cuda:0')
    slots = torch.randn(V, T, N, C, generator=torch.Generator().manual_seed(0)).to(dev)
    bs = batches(dev, a.questions)
    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__,
           'shape': dict(videos=V, frames=T, num_slots=N, slot_size=C, text_len=TEXT, tokens=1 + T * N + TEXT, d_model=144, num_heads=8, ffn_dim=512,
                         num_layers=a.layers, dropout=0.1, questions=a.questions, sequences=bs[0]['tokens'].shape[0], descriptive=bs[0]['B1'])}
    forms = {'native': Native(slots, bs, a.layers), 'eager': Eager(slots, bs, a.layers)}
    n, times, peak = {}, {k: [] for k in forms}, {}
    for k, f in forms.items():   # warm-up, then how many steps make a window of `seconds`
        f.run(2)
        n[k] = max(2, int(a.seconds / (window(lambda: f.run(3)) / 3)) + 1)
    while min(len(v) for v in times.values()) < a.windows:
        for k, f in forms.items():
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            w = window(lambda: f.run(n[k]))
            peak[k] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)   # MiB a window adds over what both forms keep resident
            if w < a.seconds:   # the probe was optimistic: a window shorter than asked for is not kept
                n[k] = int(1.3 * n[k] * a.seconds / w) + 1
                continue
            if len(times[k]) < a.windows:
                times[k].append(w / n[k] * 1e3)
    out = {k + '_step': stats(v) for k, v in times.items()}
    out['steps_per_window'] = n
    out['peak_window_MiB'] = peak
    out['native_workspace_MiB'] = round(forms['native'].ws.numel() / 2 ** 20, 1)
    for k, f in forms.items():
        out[k + '_launches_per_step'], out[k + '_kernels'] = launches_per_step(f)
    med = {k: statistics.median(v) for k, v in times.items()}
    out['eager_over_native'] = round(med['eager'] / med['native'], 3)
    out['native_faster_than_eager'] = bool(max(times['native']) < min(times['eager']))   # "faster" only when the windows do not overlap
    res['result'] = out
    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
