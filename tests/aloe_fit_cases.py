"""What the tests of the Aloe reasoner's training path share (no test in here): the seeded cases, a float64 restatement of the reference
`forward` + its training loss (w_cls cross-entropy + w_mc BCE-with-logits) under torch autograd -- the forward of `clevrer_vqa_cases.forward64`,
padded rows DROPPED, not masked -- whose dropout masks come from `train.dropout_keep_mask` in the full-L numbering with the live rows / keys
selected and whose ReLUs are written `h * gate` with the gates passed in, the band rule for gates, the planted set `fit` is tested on, and a
float64 restatement of a whole `fit` run (same schedule, same masks, torch.optim.Adam, the same learning-rate rule)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import clevrer_vqa_cases as cases
from phyre_fit_cases import keep_masks, leaves64, LAYER_KEYS

DEVICE_BAR = cases.DEVICE_BAR
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clevrer_aloe_grads.npz')   # tools/gen_golden_clevrer_vqa_grads.py


def grad_keys(cfg):
    """state-dict keys in the order of `ops.aloe_grad_layout` / `train.aloe_parameters`"""
    keys = ['CLS', 'transformer_encoder.pos_enc', 'vision_in_proj.weight', 'vision_in_proj.bias', 'q_in_proj.weight', 'q_in_proj.bias']
    for i in range(cases.dims(cfg)['nl']):
        keys += [f'transformer_encoder.layers.{i}.{k}' for k in LAYER_KEYS]
    return keys + ['cls_answer_mlp.0.weight', 'cls_answer_mlp.0.bias', 'mc_answer_mlp.0.weight', 'mc_answer_mlp.0.bias', 'q_embedding.weight',
                   'cls_answer_mlp.2.weight', 'cls_answer_mlp.2.bias', 'mc_answer_mlp.2.weight', 'mc_answer_mlp.2.bias']


def _case(name, T, N, C, text_len, cls_lengths=(), mc_lengths=(), choice_lengths=(), heads=8, input_dim=16, nl=1, ffn=64, p=0.0, seed=0, ql=None, **kw):
    return dict(name=name, T=T, N=N, C=C, text_len=text_len, cls_lengths=list(cls_lengths), mc_lengths=list(mc_lengths),
                choice_lengths=list(choice_lengths), heads=heads, input_dim=input_dim, nl=nl, ffn=ffn, p=p, seed=seed, ql=ql, **kw)


# Every sequence is one workgroup per head in both attention launches: a wave owns 16-query tiles (pass A) / 16-key tiles (pass B) and steps over
# 32 keys / queries at a time, so live lengths 15 / 16 / 17 and 31 / 32 / 33 stand on both sides of a tile and of an MFMA step.  The GEMMs and the
# weight-gradient contraction tile the B L rows by 32 / 64; the contraction splits its rows in two from 65 rows on (train_blocks.h:
# tn_splits_edge -- min(ceil(512 / tiles), ceil(rows / 64))): `rows64` and `rows65` stand on both sides.
CASES = [
    _case('tiny-L6', 1, 1, 32, 4, cls_lengths=[1, 4, 3], mc_lengths=[2, 1], choice_lengths=[1, 2], ql=2, seed=1),
    _case('live-15-16-17-b1-only', 2, 3, 32, 12, cls_lengths=[8, 9, 10], p=0.1, seed=2),
    _case('live-31-32-33-bn-only', 4, 5, 64, 14, mc_lengths=[6, 7, 8], choice_lengths=[4, 4, 4], ql=8, p=0.1, seed=3),
    _case('L256-full', 15, 16, 32, 15, cls_lengths=[15], mc_lengths=[9], choice_lengths=[5], ql=10, p=0.1, seed=4),
    _case('reference-geometry', 25, 7, 128, 32, cls_lengths=[14], mc_lengths=[12, 20], choice_lengths=[5, 12], ql=20, nl=2, ffn=512, p=0.1, seed=5),
    _case('hd6', 2, 3, 32, 5, cls_lengths=[5], mc_lengths=[2], choice_lengths=[2], ql=3, heads=2, input_dim=4, p=0.1, seed=6),
    _case('hd32', 3, 5, 96, 7, cls_lengths=[7, 4], mc_lengths=[3], choice_lengths=[1], ql=4, heads=4, input_dim=30, seed=7),
    _case('mc-padding-inside-one-choice', 2, 4, 64, 10, cls_lengths=[3], mc_lengths=[2, 2, 6], choice_lengths=[4, 1, 2], ql=6, mc_flag=[0, 0, 1], nl=2,
          p=0.1, seed=8),
    _case('strided-nan-start-offset', 4, 7, 128, 8, cls_lengths=[8, 5], mc_lengths=[2], choice_lengths=[3], ql=4, T_all=12, start=[3, 0, 5],
          frame_offset=2, strided=True, p=0.1, seed=9),
    _case('video-index-shuffled', 3, 7, 128, 8, cls_lengths=[3, 8, 1], mc_lengths=[6, 4], choice_lengths=[2, 1], ql=6, V=4, video_index=[3, 0, 0, 2, 1],
          seed=10),
    _case('n16-c256', 2, 16, 256, 6, cls_lengths=[6], mc_lengths=[2], choice_lengths=[2], ql=3, p=0.1, seed=11),
    _case('rows64', 3, 4, 32, 3, cls_lengths=[3, 1], mc_lengths=[1, 2], choice_lengths=[1, 1], ql=2, p=0.1, seed=12),
    _case('rows65', 2, 4, 32, 4, cls_lengths=[4, 1, 2], mc_lengths=[1, 2], choice_lengths=[1, 2], ql=2, p=0.1, seed=13),
]
CASE_IDS = [c['name'] for c in CASES]


def train_case(case, w_cls=1.0, w_mc=1.0):
    """-> dict(cfg, sd, slots [V, T_all, N, C], tokens / pad [B, text_len], B1, video_index, start, frame_offset, T, cls_label, mc_label, seed, p,
    w_cls, w_mc): ONE batch of B1 descriptive sequences, then Bn choices."""
    B1, Bn = len(case['cls_lengths']), len(case['mc_lengths'])
    B = B1 + Bn
    ql = case['ql'] if case['ql'] is not None else case['text_len']
    cfg = cases.config(case['T'], case['N'], case['C'], case['text_len'], case['heads'], case['input_dim'], case['nl'], case['ffn'], question_len=ql,
                       q_vocab=37, a_vocab=9, mlp=48)
    sd = cases.seeded_weights(cfg, 17000 + case['seed'])
    slots = cases.seeded_slots(18000 + case['seed'], case.get('V', B), case.get('T_all', case['T']), case['N'], case['C'])
    rng = np.random.default_rng(19000 + case['seed'])
    tok_c, pad_c = cases.seeded_text(19100 + case['seed'], B1, case['text_len'], 37, lengths=case['cls_lengths']) if B1 else (
        np.zeros((0, case['text_len']), np.int64), np.zeros((0, case['text_len']), bool))
    tok_m, pad_m = cases.seeded_text(19200 + case['seed'], Bn, case['text_len'], 37, lengths=case['mc_lengths'], question_len=ql,
                                     choice_lengths=case['choice_lengths']) if Bn else (np.zeros((0, case['text_len']), np.int64),
                                                                                        np.zeros((0, case['text_len']), bool))
    return dict(cfg=cfg, sd=sd, slots=slots, tokens=np.concatenate([tok_c, tok_m]), pad=np.concatenate([pad_c, pad_m]), B1=B1,
                video_index=case.get('video_index'), start=case.get('start'), frame_offset=case.get('frame_offset', 1), T=case['T'],
                cls_label=rng.integers(0, 9, size=B1), mc_label=(rng.uniform(size=Bn) > 0.5).astype(np.float32), seed=7654321 + case['seed'],
                p=case['p'], w_cls=w_cls, w_mc=w_mc, strided=bool(case.get('strided')))


def _layer(w, i, x, heads, m, gate):
    """one pre-LN nn.TransformerEncoderLayer on x [1, n, d] in float64 with the four keep masks m (already cut to the live rows) and the ReLU
    pattern `gate` [n, ffn] (None: this run's own signs) -> (output, hidden pre-activations [n, ffn] detached)"""
    g = lambda k: w[f'transformer_encoder.layers.{i}.{k}']  # noqa: E731
    n, d = x.shape[1], x.shape[2]
    hd = d // heads
    h = F.layer_norm(x, (d, ), g('norm1.weight'), g('norm1.bias'), 1e-5)
    q, k, v = F.linear(h, g('self_attn.in_proj_weight'), g('self_attn.in_proj_bias')).split(d, dim=-1)
    sp = lambda t: t.reshape(1, n, heads, hd).transpose(1, 2)  # noqa: E731
    a = (torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / hd ** 0.5, dim=-1) * m[0]) @ sp(v)
    x2 = x + F.linear(a.transpose(1, 2).reshape(1, n, d), g('self_attn.out_proj.weight'), g('self_attn.out_proj.bias')) * m[1]
    h2 = F.layer_norm(x2, (d, ), g('norm2.weight'), g('norm2.bias'), 1e-5)
    hid = F.linear(h2, g('linear1.weight'), g('linear1.bias'))
    gt = (hid.detach() > 0).double() if gate is None else gate.double()[None]
    return x2 + F.linear(hid * gt * m[2], g('linear2.weight'), g('linear2.bias')) * m[3], hid.detach()[0]


def forward64(w, tc, masks=None, gates=None, head_gates=None):
    """The training forward in float64 on tensors `w` {state-dict key: float64 tensor}.  masks: `keep_masks` over the FULL [B, heads, L, L] /
    [B, L, d] / [B, L, ffn] numbering (None: no dropout); gates [layer] -> [B * L, ffn] and head_gates [B, mlp] (0 / 1): the ReLU pattern to
    apply on the live rows (None: the sign of this run's own pre-activations).
    -> (cls_logits [B1, A], mc_logits [Bn], pre: [per layer [B, L, ffn] with zeros on the padded rows, ..., head [B, mlp]], live [B, L] bool)"""
    m = cases.dims(tc['cfg'])
    heads, nl, d, ffn = m['heads'], m['nl'], m['d'], m['ffn']
    s = torch.as_tensor(np.asarray(tc['slots'])).double()
    tokens, pad = np.asarray(tc['tokens']), np.asarray(tc['pad']).astype(bool)
    B, text_len = tokens.shape
    T, N = tc['T'], s.shape[2]
    L = 1 + T * N + text_len
    pos = w['transformer_encoder.pos_enc'][0]
    tok_pair = {k: torch.tensor(v, dtype=torch.float64) for k, v in cases._TOKENS.items()}
    pre = [torch.zeros(B, L, ffn, dtype=torch.float64) for _ in range(nl)] + [None]
    live = np.zeros((B, L), bool)
    out, head_pre = [], []
    for b in range(B):
        mc = b >= tc['B1']
        vid = b if tc['video_index'] is None else int(tc['video_index'][b])
        f0 = 0 if tc['start'] is None else int(tc['start'][b])
        frames = s[vid, [f0 + t * tc['frame_offset'] for t in range(T)]]
        v_in = torch.cat([frames.flatten(0, 1), tok_pair['vision_token'].expand(T * N, 2)], -1)
        v_rows = F.linear(v_in, w['vision_in_proj.weight'], w['vision_in_proj.bias'])
        emb = w['q_embedding.weight'][torch.as_tensor(tokens[b])]
        if mc:
            ql = m['question_len']
            typ = torch.cat([tok_pair['mc_question_token'].expand(ql, 2), tok_pair['mc_choice_token'].expand(text_len - ql, 2)], 0)
        else:
            typ = tok_pair['cls_token'].expand(text_len, 2)
        q_rows = F.linear(torch.cat([emb, typ, tok_pair['text_token'].expand(text_len, 2)], -1), w['q_in_proj.weight'], w['q_in_proj.bias'])
        x = torch.cat([w['CLS'][0], v_rows, q_rows], 0) + pos
        keep = np.concatenate([np.ones(1 + T * N, bool), ~pad[b]])
        live[b] = keep
        kt = torch.as_tensor(np.nonzero(keep)[0])
        x = x[kt][None]                                                                  # the padded rows are gone
        for i in range(nl):
            if masks is None:
                mk = (1.0, 1.0, 1.0, 1.0)
            else:
                mk = (masks[i][0][b][:, kt][:, :, kt][None], masks[i][1][b][kt][None], masks[i][2][b][kt][None], masks[i][3][b][kt][None])
            gate = None if gates is None else torch.as_tensor(np.asarray(gates[i])).reshape(B, L, ffn)[b][kt]
            x, hid = _layer(w, i, x, heads, mk, gate)
            pre[i][b, kt] = hid
        mlp = 'mc_answer_mlp' if mc else 'cls_answer_mlp'
        hh = F.linear(x[0, 0], w[mlp + '.0.weight'], w[mlp + '.0.bias'])
        head_pre.append(hh.detach())
        gt = (hh.detach() > 0).double() if head_gates is None else torch.as_tensor(np.asarray(head_gates))[b].double()
        out.append(F.linear(hh * gt, w[mlp + '.2.weight'], w[mlp + '.2.bias']))
    pre[-1] = torch.stack(head_pre)
    A = m['a_vocab']
    cls_logits = torch.stack(out[:tc['B1']]) if tc['B1'] else torch.zeros(0, A, dtype=torch.float64)
    mc_logits = torch.cat(out[tc['B1']:]) if B > tc['B1'] else torch.zeros(0, dtype=torch.float64)
    return cls_logits, mc_logits, pre, live


def loss64(cls_logits, mc_logits, tc):
    """-> (w_cls CE + w_mc BCE, [CE, BCE]); a kind without rows counts 0"""
    ce = F.cross_entropy(cls_logits, torch.as_tensor(np.asarray(tc['cls_label'])).long()) if cls_logits.shape[0] else cls_logits.sum() * 0
    bce = F.binary_cross_entropy_with_logits(mc_logits, torch.as_tensor(np.asarray(tc['mc_label'])).double()) if mc_logits.shape[0] else \
        mc_logits.sum() * 0
    return tc['w_cls'] * ce + tc['w_mc'] * bce, (float(ce.detach()), float(bce.detach()))


def masks_of(tc):
    m = cases.dims(tc['cfg'])
    B, text_len = np.asarray(tc['tokens']).shape
    L = 1 + tc['T'] * np.asarray(tc['slots']).shape[2] + text_len
    return keep_masks(tc['seed'], tc['p'], B, L, m['nl'], d=m['d'], heads=m['heads'], ffn=m['ffn'])


def loss_and_grads64(tc, gates=None, head_gates=None, masks='auto'):
    """-> dict(loss, losses (CE, BCE), cls_logits, mc_logits numpy, grads {key: float64 numpy} for every key of `grad_keys`, pre, live)"""
    w = leaves64(tc['sd'])
    if isinstance(masks, str):
        masks = masks_of(tc)
    cls_logits, mc_logits, pre, live = forward64(w, tc, masks, gates, head_gates)
    loss, parts = loss64(cls_logits, mc_logits, tc)
    loss.backward()
    grads = {k: (w[k].grad if w[k].grad is not None else torch.zeros_like(w[k])).numpy() for k in grad_keys(tc['cfg'])}
    return dict(loss=loss.item(), losses=parts, cls_logits=cls_logits.detach().numpy(), mc_logits=mc_logits.detach().numpy(), grads=grads, pre=pre,
                live=live)


def clear_of_band(pre, live):
    """[bool arrays]: the gates a device must reproduce -- live rows with |h| >= DEVICE_BAR max|h| of their layer (the head: every unit)"""
    out = []
    for i, h in enumerate(pre):
        h = h.numpy()
        ok = np.abs(h) >= DEVICE_BAR * np.abs(h).max()
        out.append(ok & live[:, :, None] if i < len(pre) - 1 else ok)
    return out


def split_flat(flat, cfg, sd):
    """a flat gradient buffer (numpy) in `grad_keys` order -> {key: array shaped as the parameter}"""
    out, off = {}, 0
    for k in grad_keys(cfg):
        n = sd[k].numel()
        out[k] = np.asarray(flat[off:off + n]).reshape(tuple(sd[k].shape))
        off += n
    assert off == len(flat), (off, len(flat))
    return out


def rel_err(got, ref):
    """max |got - ref| / max |ref|; a reference that is zero everywhere wants zeros exactly (-> 0.0, else inf)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float('inf')
    big = np.abs(ref).max()
    if big == 0:
        return 0.0 if not np.any(got) else float('inf')
    return float(np.abs(got - ref).max() / big)


# ---- the REFERENCE's gradients ------------------------------------------------------------------------------------------------------------
FIXTURE = _case('fixture', 3, 4, 32, 12, cls_lengths=[5, 12, 8], mc_lengths=[4, 4, 8], choice_lengths=[3, 4, 2], ql=8, mc_flag=[0, 0, 1], heads=4, nl=2,
                seed=77)


def fixture_train_case():
    """The inputs of tests/golden/clevrer_aloe_grads.npz: 2 layers, d 72 = 4 x 18, ffn 64, C 32; 3 descriptive questions and 2 multiple-choice ones
    with 2 + 1 choices on videos 0 and 2 (the video of a choice is an index composition); eval(): no dropout."""
    tc = train_case(FIXTURE)
    tc['video_index'] = [0, 1, 2, 0, 0, 2]
    tc['mc_flag'], tc['mc_video'] = np.array(FIXTURE['mc_flag']), np.array([0, 2])
    return tc


def check_against_golden(grads, losses, bar):
    g = np.load(GOLDEN)
    keys = json.loads(str(g['keys']))
    assert sorted(keys) == sorted(grads), set(keys) ^ set(grads)
    for mine, ref in zip(losses, (float(g['cls_loss']), float(g['mc_loss']))):
        assert abs(mine - ref) < bar * abs(ref), (mine, ref)
    worst = 0.0
    for k in keys:
        err = rel_err(grads[k], g['grad.' + k])
        worst = max(worst, err)
        assert err < bar, (k, err)
    return worst


# ---- the planted set of the fit test -----------------------------------------------------------------------------------------------------------
FIT = dict(V=32, T=2, N=3, C=32, text_len=6, ql=4, heads=2, input_dim=6, nl=1, ffn=64, mlp=16, q_vocab=12, a_vocab=4, batch_size=8, lr=4e-3, seed=5,
           epochs=32)


def fit_case():
    """32 videos of 2 frames, 3 slots of 32.  One descriptive question per video whose answer is the sign of a fixed projection of slot (frame 1,
    slot 0); 16 multiple-choice questions on the even videos with two choices each, both labelled by the sign of a second projection of the same
    slot.  -> (cfg, sd, slots, questions: the collated arrays with labels)"""
    f = FIT
    cfg = cases.config(f['T'], f['N'], f['C'], f['text_len'], f['heads'], f['input_dim'], f['nl'], f['ffn'], question_len=f['ql'], q_vocab=f['q_vocab'],
                       a_vocab=f['a_vocab'], mlp=f['mlp'])
    sd = cases.seeded_weights(cfg, 41337)
    rng = np.random.default_rng(41338)
    slots = rng.standard_normal((f['V'], f['T'], f['N'], f['C'])).astype(np.float32)
    proj = rng.standard_normal((2, f['C']))
    score = slots[:, 1, 0].astype(np.float64) @ proj.T                                # [V, 2]
    cls_tok, cls_pad = cases.seeded_text(41339, f['V'], f['text_len'], f['q_vocab'], lengths=rng.integers(1, f['text_len'] + 1, size=f['V']))
    mc_video = np.arange(0, f['V'], 2)
    flag = np.repeat(np.arange(len(mc_video)), 2)
    mc_tok, mc_pad = cases.seeded_text(41340, len(flag), f['text_len'], f['q_vocab'], lengths=np.repeat(rng.integers(1, f['ql'] + 1, size=len(mc_video)), 2),
                                       question_len=f['ql'])
    q = dict(cls_q_tokens=cls_tok, cls_q_pad_mask=cls_pad, cls_video_index=np.arange(f['V']), cls_start=np.zeros(f['V'], np.int64),
             cls_label=(score[:, 0] > 0).astype(np.int64), mc_q_tokens=mc_tok, mc_q_pad_mask=mc_pad, mc_flag=flag, mc_video_index=mc_video,
             mc_start=np.zeros(len(mc_video), np.int64), mc_label=(score[mc_video[flag], 1] > 0).astype(np.float32),
             mc_subtype=np.tile([1, 2, 3, 1], len(mc_video) // 4), frame_offset=1, num_frames=f['T'])
    return cfg, sd, slots, q


def batch_case(cfg, sd, slots, q, b, seed, p):
    """one batch of `clevrer_vqa.question_schedule` as a `train_case`-shaped dict"""
    flag = np.asarray(q['mc_flag'])
    rows = b['mc_rows']
    return dict(cfg=cfg, sd=sd, slots=slots, tokens=np.concatenate([q['cls_q_tokens'][b['cls']], q['mc_q_tokens'][rows]]),
                pad=np.concatenate([q['cls_q_pad_mask'][b['cls']], q['mc_q_pad_mask'][rows]]), B1=len(b['cls']),
                video_index=np.concatenate([q['cls_video_index'][b['cls']], q['mc_video_index'][flag[rows]]]),
                start=np.concatenate([q['cls_start'][b['cls']], q['mc_start'][flag[rows]]]), frame_offset=q['frame_offset'], T=q['num_frames'],
                cls_label=q['cls_label'][b['cls']], mc_label=q['mc_label'][rows], seed=seed, p=p, w_cls=1.0, w_mc=1.0)


def fit64(cfg, sd, slots, q, epochs, batch_size, lr, seed, warmup_steps_pct=0.1, min_lr_ratio=0.01, p=0.1):
    """`clevrer_vqa.fit` restated in float64 torch: the same schedule, the same masks, torch.optim.Adam, the same learning-rate rule.
    -> (trained {key: float64 tensor}, per-epoch mean losses [epochs, 2])"""
    from slotformer_amd import clevrer_vqa, train
    w = leaves64(sd)
    opt = torch.optim.Adam([w[k] for k in grad_keys(cfg)], lr=lr)
    sched = clevrer_vqa.question_schedule(q, epochs, batch_size, seed)
    total = sum(len(e) for e in sched)
    warm = int(round(warmup_steps_pct * total))
    n_cls, n_mc = max(len(q['cls_q_tokens']), 1), max(len(q['mc_flag']), 1)
    step, losses = 0, []
    for batches in sched:
        acc = np.zeros(2)
        for b in batches:
            tc = batch_case(cfg, w, slots, q, b, clevrer_vqa.step_seed(seed, step), p)
            cls_logits, mc_logits, _, _ = forward64(w, tc, masks_of(tc))
            loss, parts = loss64(cls_logits, mc_logits, tc)
            opt.zero_grad()
            loss.backward()
            for g in opt.param_groups:
                g['lr'] = train.warmup_cosine_lr(step, total, warm, lr, lr * min_lr_ratio)
            opt.step()
            step += 1
            acc += np.array(parts) * np.array([tc['B1'] / n_cls, len(b['mc_rows']) / n_mc])
        losses.append(acc)
    return {k: v.detach() for k, v in w.items()}, np.array(losses)
