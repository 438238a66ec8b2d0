"""CLEVRER VQA measurements (profiles/clevrer_vqa.md).   python tools/bench_clevrer_vqa.py [--json PATH] [--md PATH] [--seconds 0.5]

On one GPU, at the reference shape (aloe_clevrer_params-rollout.py: 25 frames of 7 slots of 128, 32 text positions, 208 tokens, 12 layers of
d 144 / 8 heads / ffn 512), on seeded weights, slots and questions, descriptive and multiple choice, at B 256 (the config's val_batch_size) and
B 32:

  * native: `CLEVRERTransformerModel.answer` (embed, per layer LN1 + q|k|v GEMM, attention, out_proj GEMM, LN2 + linear1 GEMM, linear2 GEMM,
    head);
  * eager: a torch-eager restatement of the same model in this project's own words (embedding lookup, cat of the id pairs, linear, cat, per
    layer layer_norm, linear, masked softmax attention, linear, layer_norm, linear, relu, linear, then linear, relu, linear);
  * torch_module: torch's own nn.TransformerEncoder on the same parameters with src_key_padding_mask, same device.

The paths alternate call by call after a warm-up of each, timed with device events until each has run for `--seconds`; medians, with the minimum
and maximum, and the largest distance of the three from each other.  No GPU: the tool fails, it measures nothing."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as tnf  # noqa: E402


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
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    while (min(sum(v) for v in ts.values()) < seconds * 1e3 or len(next(iter(ts.values()))) < min_calls) and len(next(iter(ts.values()))) < max_calls:
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    return ts


def stats(v):
    return {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4), 'calls': len(v)}


def eager_tokens(tm, slots, tokens, mc):
    """[B, L, d]: CLS, the projected slots (t-major, slot-minor), the projected text, + the position table"""
    B, text_len = tokens.shape
    v = torch.cat([slots.flatten(1, 2), tm.vision_token.expand(B, slots.shape[1] * slots.shape[2], 2)], -1)
    emb = tm.q_embedding(tokens)
    if mc:
        ql = tm.question_len
        typ = torch.cat([tm.mc_question_token.expand(B, ql, 2), tm.mc_choice_token.expand(B, text_len - ql, 2)], 1)
    else:
        typ = tm.cls_token.expand(B, text_len, 2)
    q = torch.cat([emb, typ, tm.text_token.expand(B, text_len, 2)], -1)
    x = torch.cat([tm.CLS.expand(B, 1, -1), tm.vision_in_proj(v), tm.q_in_proj(q)], 1)
    return x + tm.transformer_encoder.pos_enc


def full_mask(pad, L):
    return torch.cat([torch.zeros(pad.shape[0], L - pad.shape[1], dtype=torch.bool, device=pad.device), pad], 1)


@torch.no_grad()
def eager_forward(tm, slots, tokens, pad, mc):
    x = eager_tokens(tm, slots, tokens, mc)
    B, L, D = x.shape
    bias = torch.zeros(B, 1, 1, L, device=x.device).masked_fill_(full_mask(pad, L)[:, None, None, :], float('-inf'))
    for layer in tm.transformer_encoder.layers:
        h = tnf.layer_norm(x, (D, ), layer.norm1.weight, layer.norm1.bias, 1e-5)
        q, k, v = tnf.linear(h, layer.self_attn.in_proj_weight, layer.self_attn.in_proj_bias).split(D, -1)
        nh = layer.self_attn.num_heads
        sp = lambda t: t.reshape(B, L, nh, D // nh).transpose(1, 2)  # noqa: E731
        a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / (D // nh) ** 0.5 + bias, -1) @ sp(v)
        x = x + tnf.linear(a.transpose(1, 2).reshape(B, L, D), layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias)
        h = tnf.layer_norm(x, (D, ), layer.norm2.weight, layer.norm2.bias, 1e-5)
        x = x + tnf.linear(torch.relu(tnf.linear(h, layer.linear1.weight, layer.linear1.bias)), layer.linear2.weight, layer.linear2.bias)
    return (tm.mc_answer_mlp if mc else tm.cls_answer_mlp)(x[:, 0])


@torch.no_grad()
def module_forward(tm, encoder, slots, tokens, pad, mc):
    x = eager_tokens(tm, slots, tokens, mc)
    return (tm.mc_answer_mlp if mc else tm.cls_answer_mlp)(encoder(x, src_key_padding_mask=full_mask(pad, x.shape[1]))[:, 0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None)
    ap.add_argument('--seconds', type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_clevrer_vqa: no GPU; nothing is measured without one')
    import clevrer_vqa_cases as cases
    from slotformer_amd.clevrer_vqa.models import CLEVRERTransformerModel
    dev = torch.device('cuda:0')
    cfg = cases.config()
    tm = CLEVRERTransformerModel(*cfg)
    tm.load_state_dict(cases.seeded_weights(cfg, 1))
    tm = tm.eval().to(dev)
    # torch's module on the SAME parameter tensors
    td = cfg[0]
    layer = nn.TransformerEncoderLayer(d_model=tm.d_model, nhead=td['num_heads'], dim_feedforward=td['ffn_dim'], norm_first=True, batch_first=True)
    encoder = nn.TransformerEncoder(layer, td['num_layers'], enable_nested_tensor=False).eval().to(dev)
    encoder.layers = tm.transformer_encoder.layers
    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'transformer_dict': td}
    T, N, C, text_len = 25, 7, 128, 32
    for B in (256, 32):
        slots = torch.from_numpy(cases.seeded_slots(B, B, T, N, C)).to(dev)
        for mc in (False, True):
            tok, pad = cases.seeded_text(B + int(mc), B, text_len, 82, question_len=20 if mc else None)
            tok, pad = torch.from_numpy(tok).to(dev), torch.from_numpy(pad).to(dev)
            fns = {'native': lambda: tm.answer(slots, tok, pad, mc), 'eager': lambda: eager_forward(tm, slots, tok, pad, mc),
                   'torch_module': lambda: module_forward(tm, encoder, slots, tok, pad, mc)}
            sec = {k: stats(v) for k, v in alternate(fns, a.seconds).items()}
            nat, eag, mod = tm.answer(slots, tok, pad, mc)[0], eager_forward(tm, slots, tok, pad, mc), module_forward(tm, encoder, slots, tok, pad, mc)
            sec['max_abs_difference'] = {'native_vs_eager': float((nat - eag).abs().max()), 'module_vs_eager': float((mod - eag).abs().max()),
                                         'largest_abs_logit': float(eag.abs().max())}
            sec['over_native'] = {'eager': round(sec['eager']['median_ms'] / sec['native']['median_ms'], 2),
                                  'torch_module': round(sec['torch_module']['median_ms'] / sec['native']['median_ms'], 2)}
            res[f"{'mc' if mc else 'descriptive'}_B{B}"] = sec
    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')
    if a.md:
        rows = ['| measurement | path | median ms | min - max ms | calls |', '|---|---|---|---|---|']
        for name, sec in res.items():
            if isinstance(sec, dict):
                for k, s in sec.items():
                    if isinstance(s, dict) and 'median_ms' in s:
                        rows.append(f"| {name} | {k} | {s['median_ms']} | {s['min_ms']} - {s['max_ms']} | {s['calls']} |")
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, 'w') as f:
            f.write(f"Measured by `tools/bench_clevrer_vqa.py` on {res['device']} (torch {res['torch']}).\n\n" + '\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
