"""The fused vocabulary head + cross-entropy against the chain it replaces (profiles/head_ce.md).
    python tools/bench_head_ce.py [--json PATH] [--seconds 1.0] [--windows 3] [--frames 16,64,192] [--fit-batches 2,4] [--no-fit]
    python tools/bench_head_ce.py --wgrad [--json PATH] [--seconds 1.0] [--windows 3] [--frames 16,64,72,192]     (profiles/head_ce_wgrad.md)

  fused   train.head_cross_entropy forward + backward: sf_head_ce_fwd_f32 / sf_head_ce_bwd_f32, no [R, V] tensor.
  chain   train.linear(x, head) + train.token_cross_entropy forward + backward: the logits, a saved copy's worth and their gradient.

Shapes: the Physion head, V 4096 x K 192, on R = frames x 1024 token rows.  Both forms run in ONE process in alternating windows of at least
`--seconds` each after a warm-up of each; a window ends in a device synchronise and is timed with the host clock; ms per call = window / calls, the
median over the windows with minimum and maximum.  The peak of torch's allocator over one call of each form (above what is allocated before it)
is the memory figure.  The fraction of the split-bf16 MFMA roof counts 3 x 2 R V K useful FLOP per call (one product forward, two backward)
against 2.5 PFLOP/s / 3, as bench.py prices the split-bf16 products.

Then one training step of `video_prediction.fit(tokens=)` at the Physion configuration (slotformer_physion_params.py: 15 burn-in + 10 predicted
frames, 6 slots of 192, rollouter d 256 x 8 layers, the frozen 4-block decoder of width 192 on 1024 tokens, vocabulary 4096) against the same step
through the module path (model(data), calc_train_loss, backward, FlatAdam.step()), at the batches of --fit-batches, with the peak memory of each;
the largest batch either path holds is EXTRAPOLATED from those peaks (linear in the batch) to the device's memory, not probed.
No GPU: the tool fails, it measures nothing."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

V, K, TOKENS = 4096, 192, 1024
ROOF = 2.5e15 / 3
HIST, S, F = 15, 10, 1
NV, NT = 4, 32


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4), 'windows': len(v)}


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def alternate(fa, fb, seconds, windows):
    """ms per call of the two forms, in alternating windows of at least `seconds`"""
    n = []
    for fn in (fa, fb):
        fn()
        probe = window(lambda: [fn() for _ in range(3)]) / 3
        n.append(max(3, int(seconds / probe) + 1))
    ta, tb = [], []
    while len(tb) < windows:
        wa = window(lambda: [fa() for _ in range(n[0])])
        wb = window(lambda: [fb() for _ in range(n[1])])
        if wa < seconds or wb < seconds:   # a probe was optimistic: a window shorter than asked for is not kept
            n = [int(1.3 * k * seconds / w) + 1 if w < seconds else k for k, w in zip(n, (wa, wb))]
            continue
        ta.append(wa / n[0] * 1e3)
        tb.append(wb / n[1] * 1e3)
    return ta, tb, n


def bench_head(frames, seconds, windows, dev):
    from slotformer_amd import train
    gen = torch.Generator().manual_seed(0)
    head = torch.nn.Linear(K, V, bias=False).to(dev)
    with torch.no_grad():
        head.weight.copy_(torch.randn(V, K, generator=gen) / K**0.5)
    frozen = torch.nn.Linear(K, V, bias=False).to(dev)
    frozen.load_state_dict(head.state_dict())
    frozen.weight.requires_grad_(False)
    out = {}
    for nf in frames:
        R = nf * TOKENS
        x0 = (torch.randn(R, K, generator=gen) * 2).to(dev)
        t = torch.randint(0, V, (R, ), generator=gen).to(dev)

        def fused():
            x = x0.detach().requires_grad_(True)
            train.head_cross_entropy(x, frozen, t)[0].backward()

        def chain():
            x = x0.detach().requires_grad_(True)
            train.token_cross_entropy(train.linear(x, head), t).backward()
            head.weight.grad = None

        tf, tc, n = alternate(fused, chain, seconds, windows)
        mf, mc = statistics.median(tf), statistics.median(tc)
        out[f'{nf}_frames'] = {'rows': R, 'fused': stats(tf), 'chain': stats(tc), 'calls_per_window': n, 'chain_over_fused': round(mc / mf, 3),
                               'fused_fraction_of_split_bf16_roof': round(3 * 2 * R * V * K / (mf * 1e-3) / ROOF, 4),
                               'fused_peak_MiB': round(peak(fused), 1), 'chain_peak_MiB': round(peak(chain), 1), 'one_RxV_tensor_MiB': R * V * 4 / 2**20}
        del x0, t
    return out


def bench_wgrad(frames, seconds, windows, dev):
    """forward + backward with a TRAINED head: head_cross_entropy(..., weight_grad=True) (loss, dx and dW without the logits: five products of
    2 R V K FLOP -- one forward, two in each of the two backward launches) against the chain, which forms the logits once (three products)"""
    from slotformer_amd import train
    gen = torch.Generator().manual_seed(0)
    head = torch.nn.Linear(K, V, bias=False).to(dev)
    with torch.no_grad():
        head.weight.copy_(torch.randn(V, K, generator=gen) / K**0.5)
    out = {}
    for nf in frames:
        R = nf * TOKENS
        x0 = (torch.randn(R, K, generator=gen) * 2).to(dev)
        t = torch.randint(0, V, (R, ), generator=gen).to(dev)

        def fused():
            x = x0.detach().requires_grad_(True)
            train.head_cross_entropy(x, head, t, weight_grad=True)[0].backward()
            head.weight.grad = None

        def chain():
            x = x0.detach().requires_grad_(True)
            train.token_cross_entropy(train.linear(x, head), t).backward()
            head.weight.grad = None

        tf, tc, n = alternate(fused, chain, seconds, windows)
        mf, mc = statistics.median(tf), statistics.median(tc)
        out[f'{nf}_frames'] = {'rows': R, 'fused': stats(tf), 'chain': stats(tc), 'calls_per_window': n, 'chain_over_fused': round(mc / mf, 3),
                               'fused_fraction_of_split_bf16_roof': round(5 * 2 * R * V * K / (mf * 1e-3) / ROOF, 4),
                               'chain_fraction_of_split_bf16_roof': round(3 * 2 * R * V * K / (mc * 1e-3) / ROOF, 4),
                               'fused_peak_MiB': round(peak(fused), 1), 'chain_peak_MiB': round(peak(chain), 1), 'one_RxV_tensor_MiB': R * V * 4 / 2**20}
        del x0, t
    return out


def physion_model(dev):
    """STEVESlotFormer at slotformer_physion_params.py on a STEVE of seeded weights (both frozen parts: their values do not matter to the time)."""
    import golden_util as gu
    from slotformer_amd.base_slots import build_model as bb
    from slotformer_amd.video_prediction import build_model as bv
    sc = gu.savi_cfg(128, 6, slot_size=192, mlp=384, iters=2, pred='transformer', rnn=True, kld='none', enc_out=192, pred_ffn=768)
    sc['model'] = 'STEVE'
    sc['dvae_dict'] = dict(down_factor=4, vocab_size=V, dvae_ckp_path='')
    sc['dec_dict'] = dict(dec_type='slate', dec_num_layers=4, dec_num_heads=4, dec_d_model=K)
    sc['loss_dict'] = dict(use_img_recon_loss=False)
    torch.manual_seed(1)
    steve = bb(gu.ParamsView(sc))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'steve.pth')
        torch.save({'state_dict': steve.state_dict()}, path)
        cfg = dict(model='STEVESlotFormer', resolution=sc['resolution'], input_frames=HIST, slot_dict=dict(num_slots=6, slot_size=192),
                   dvae_dict=dict(sc['dvae_dict']), dec_dict=dict(dec_num_layers=4, dec_num_heads=4, dec_d_model=K, dec_ckp_path=path),
                   rollout_dict=dict(num_slots=6, slot_size=192, history_len=HIST, t_pe='sin', slots_pe='', d_model=256, num_layers=8, num_heads=8,
                                     ffn_dim=1024, norm_first=True),
                   loss_dict=dict(rollout_len=S, use_img_recon_loss=True))
        model = bv(gu.ParamsView(cfg))
    return model.to(dev).train()


def bench_fit(batches, seconds, windows, dev):
    from slotformer_amd import train, video_prediction as vp
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(NV, NT, 6, 192, generator=gen).to(dev)
    tokens = torch.randint(0, V, (NV, NT, TOKENS), generator=gen).to(torch.int16).to(dev)
    clips = vp.clip_index(NV, NT, HIST + S, F, 'train')   # 8 starts x 4 videos
    steps = torch.arange(HIST + S, device=dev) * F
    out = {'clips': int(clips.shape[0])}
    total = torch.cuda.get_device_properties(0).total_memory / 2**20
    m_fit, m_mod = physion_model(dev), physion_model(dev)
    for B in batches:
        k = clips.shape[0] // B
        opt = train.FlatAdam(train.rollouter_parameters(m_mod.rollouter), lr=1e-4)
        vid, start = clips[:B * k, 0].long().to(dev).view(k, B), clips[:B * k, 1].long().to(dev).view(k, B)

        def fit_call():
            vp.fit(m_fit, table, clips[:B * k], 1, B, 1e-4, 0, F, tokens=tokens)

        def module_call():
            for i in range(k):
                v, t = vid[i][:, None], start[i][:, None] + steps[None]
                data = {'slots': table[v, t], 'token_id': tokens[v, t[:, HIST:]].long()}
                terms = m_mod.calc_train_loss(data, m_mod(data))
                opt.zero_grad()
                (terms['slot_recon_loss'] + terms['img_recon_loss']).backward()
                opt.step()

        tf, tm, n = alternate(fit_call, module_call, seconds, windows)
        out[f'batch_{B}'] = {'steps_per_call': k, 'rows': B * S * TOKENS, 'fit_step': stats([t / k for t in tf]), 'module_step': stats([t / k for t in tm]),
                             'module_over_fit': round(statistics.median(tm) / statistics.median(tf), 3),
                             'fit_peak_MiB': round(peak(fit_call), 1), 'module_peak_MiB': round(peak(module_call), 1)}
    if len(batches) >= 2:
        b0, b1 = batches[0], batches[-1]
        free = total - torch.cuda.memory_allocated() / 2**20
        for key in ('fit', 'module'):
            p0, p1 = out[f'batch_{b0}'][f'{key}_peak_MiB'], out[f'batch_{b1}'][f'{key}_peak_MiB']
            per = (p1 - p0) / (b1 - b0)
            out[f'{key}_MiB_per_clip'] = round(per, 1)
            out[f'{key}_largest_batch_extrapolated'] = int((free - (p0 - per * b0)) / per) if per > 0 else None
        out['device_memory_MiB'] = round(total, 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--frames', default='16,64,192')
    ap.add_argument('--fit-batches', default='2,4')
    ap.add_argument('--no-fit', action='store_true')
    ap.add_argument('--wgrad', action='store_true', help='a TRAINED head instead: weight_grad=True against the chain, at --frames (16,64,72,192)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_head_ce: no GPU; nothing is measured without one')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'head': dict(V=V, K=K, tokens_per_frame=TOKENS)}
    if a.wgrad:
        frames = '16,64,72,192' if a.frames == ap.get_default('frames') else a.frames
        res['head_ce_wgrad'] = bench_wgrad([int(f) for f in frames.split(',')], a.seconds, a.windows, dev)
    else:
        res['head_ce'] = bench_head([int(f) for f in a.frames.split(',')], a.seconds, a.windows, dev)
    if not a.no_fit and not a.wgrad:
        res['fit_step'] = bench_fit([int(b) for b in a.fit_batches.split(',')], a.seconds, a.windows, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
