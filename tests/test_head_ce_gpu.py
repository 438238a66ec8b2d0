"""GPU: the fused vocabulary head + cross-entropy (csrc/head_ce.hip, train.head_cross_entropy) and the token loss of `video_prediction.fit` /
`evaluate` that rests on it.  The kernel pair is held to torch.float64 `F.cross_entropy` with autograd on the CPU -- never to the chain it
replaces -- at the project's own bars: 1e-3 relative for the loss and lse (the README's fp32 bar), L2TOL['bf16x3'] = 2e-3 for gradients
(tests/test_train_gpu.py).  Measured errors: profiles/head_ce.md."""
import functools

import numpy as np
import pytest
import torch

import golden_util as gu
import oracle

pytestmark = pytest.mark.gpu

TOL = 1e-3      # loss, lse: relative to the largest entry
L2TOL = 2e-3    # gradients: relative L2 norm (tests/test_train_gpu.py, 'bf16x3')
# one row; a ragged and an over-full row tile; a vocabulary the four waves cannot split evenly; the Physion shape; the widest K
SHAPES = [(1, 32, 32), (63, 64, 64), (65, 96, 64), (130, 4096, 192), (64, 160, 256)]


def rel_err(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max()).item()


def l2_err(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return ((a - b).norm() / b.norm()).item()


def _targets(R, V, gen):
    """word 0 and word V - 1 occur, and where there is a whole tile of 64 rows, it shares one target"""
    t = torch.randint(0, V, (R, ), generator=gen)
    if R >= 64:
        t[:64] = 7
    if R == 64:
        t[:] = V - 1
        return t
    t[-1] = 0
    if 2 <= R < 64:
        t[0] = V - 1
    if R > 65:
        t[-2] = V - 1
    return t


@functools.lru_cache(maxsize=None)
def case(R, V, K, peak=None):
    """x, w, targets and the float64 reference (per-row lse and loss, d(sum of the losses)/dx), computed once and shared.  The logits have a
    standard deviation of about 2; with `peak`, x is scaled so that the largest logit is +-peak."""
    gen = torch.Generator().manual_seed(1000 * R + V + K)
    x = torch.randn(R, K, generator=gen) * 2
    w = torch.randn(V, K, generator=gen) / K**0.5
    if peak is not None:
        x = (x * (peak / (x.double() @ w.double().t()).abs().max())).float()
    t = _targets(R, V, gen)
    xr = x.double().requires_grad_(True)
    logits = xr @ w.double().t()
    loss = torch.nn.functional.cross_entropy(logits, t, reduction='none')
    loss.sum().backward()
    out = dict(x=x, w=w, t=t, lse=torch.logsumexp(logits.detach(), 1), loss=loss.detach(), dx=xr.grad, peak=float(logits.detach().abs().max()))
    assert all(bool(torch.isfinite(out[k]).all()) for k in ('lse', 'loss', 'dx'))   # the reference itself is finite
    return out


def run_pair(dev, c, dtype=torch.int64, ld=None, g=1., group_w=None, group=1, rows=None):
    """The two launches on case `c` (or on its rows `rows`) -> lse, loss_rows, stats, dx, all on the host."""
    from slotformer_amd import ops
    x, t = (c['x'], c['t']) if rows is None else (c['x'][rows], c['t'][rows])
    R, K = x.shape
    V = c['w'].shape[0]
    if ld is None:
        xd = x.to(dev).contiguous()
    else:   # rows of a wider buffer whose other columns hold NaN: nothing beyond column K may be read
        buf = torch.full((R, ld), float('nan'), device=dev)
        buf[:, :K] = x.to(dev)
        xd = buf[:, :K]
    packed = ops.pack_head_ce_weight(c['w'].to(dev))
    td = t.to(dev).to(dtype)
    gw = None if group_w is None else group_w.to(dev)
    stats = torch.zeros(2, dtype=torch.float64, device=dev)
    lse, loss = ops.head_ce_forward(xd, packed, td, V, gw, group, stats)
    dx = ops.head_ce_backward(xd, packed, td, V, lse, torch.tensor([g], device=dev), gw, group)
    return lse.cpu(), loss.cpu(), stats.cpu(), dx.cpu()


@pytest.mark.parametrize('dtype', [torch.int64, torch.int16], ids=['i64', 'i16'])
@pytest.mark.parametrize('R,V,K', SHAPES)
def test_kernel_pair_vs_float64(dev, R, V, K, dtype):
    c = case(R, V, K)
    lse, loss, stats, dx = run_pair(dev, c, dtype)
    e = (rel_err(lse, c['lse']), rel_err(loss, c['loss']), l2_err(dx, c['dx']))
    print(f'head_ce R {R} V {V} K {K}: lse {e[0]:.3g} loss {e[1]:.3g} dx(l2) {e[2]:.3g}')
    assert e[0] < TOL and e[1] < TOL and e[2] < L2TOL
    assert abs(float(stats[0]) - float(c['loss'].sum())) < TOL * float(c['loss'].sum()) and float(stats[1]) == R
    assert float(stats[0]) == pytest.approx(float(loss.double().sum()), rel=1e-12)   # the float64 sum of the rows it wrote


@pytest.mark.parametrize('R,V,K,group', [(65, 96, 64, 1), (64, 160, 256, 8), (130, 4096, 192, 1), (1, 32, 32, 1)])
def test_strided_rows_scaled_gradient_and_group_weights(dev, R, V, K, group):
    """ld > K, g != 1, and group weights with zeros: a dropped group contributes nothing and its rows get exact zeros."""
    c = case(R, V, K)
    gen = torch.Generator().manual_seed(R)
    gw = torch.rand(R // group, generator=gen) + 0.5
    gw[::3] = 0.
    if R == 1:
        gw[:] = 1.5
    g = -0.37
    lse, loss, stats, dx = run_pair(dev, c, ld=K + 12, g=g, group_w=gw, group=group)
    wr = gw.double().repeat_interleave(group)
    assert rel_err(lse, c['lse']) < TOL and rel_err(loss, c['loss']) < TOL
    want = (float((wr * c['loss']).sum()), float(wr.sum()))
    assert abs(float(stats[0]) - want[0]) < TOL * want[0] and abs(float(stats[1]) - want[1]) <= 1e-12 * want[1]
    assert l2_err(dx, g * wr[:, None] * c['dx']) < L2TOL
    dropped = wr == 0
    assert bool((dx[dropped] == 0).all()) and (R == 1 or bool(dropped.any()))
    # stats are ADDED to: a second call on the same buffer doubles them, bit for bit
    from slotformer_amd import ops
    packed = ops.pack_head_ce_weight(c['w'].to(dev))
    st = torch.zeros(2, dtype=torch.float64, device=dev)
    for _ in range(2):
        ops.head_ce_forward(c['x'].to(dev), packed, c['t'].to(dev), V, gw.to(dev), group, st)
    assert torch.equal(st.cpu(), 2 * stats)


def test_logits_of_80_do_not_overflow(dev):
    c = case(63, 64, 64, 80.)
    assert 79.9 < c['peak'] < 80.1
    lse, loss, _, dx = run_pair(dev, c)
    assert bool(torch.isfinite(lse).all() and torch.isfinite(loss).all() and torch.isfinite(dx).all())
    e = (rel_err(lse, c['lse']), rel_err(loss, c['loss']), l2_err(dx, c['dx']))
    print(f'head_ce logits +-80: lse {e[0]:.3g} loss {e[1]:.3g} dx(l2) {e[2]:.3g}')
    assert e[0] < TOL and e[1] < TOL and e[2] < L2TOL


def test_target_outside_the_vocabulary_matches_nothing(dev):
    """picked by comparison, never by address: loss = lse, and the gradient is the softmax's alone"""
    c = dict(case(65, 96, 64))
    t = c['t'].clone()
    t[3], t[64] = -1, 96
    c['t'] = t
    lse, loss, _, dx = run_pair(dev, c)
    assert torch.equal(loss[[3, 64]], lse[[3, 64]])
    p = torch.softmax(c['x'].double() @ c['w'].double().t(), 1)
    assert l2_err(dx[[3, 64]], (p @ c['w'].double())[[3, 64]]) < L2TOL
    keep = torch.ones(65, dtype=torch.bool)
    keep[[3, 64]] = False
    assert rel_err(loss[keep], c['loss'][keep]) < TOL and l2_err(dx[keep], c['dx'][keep]) < L2TOL


def test_two_calls_and_any_place_in_the_batch_give_the_same_bits(dev):
    c = case(130, 4096, 192)
    gw = torch.ones(130)
    a = run_pair(dev, c, g=0.5, group_w=gw)
    b = run_pair(dev, c, g=0.5, group_w=gw)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    for r in (0, 63, 64, 129):   # first and last row of a tile, and the ragged tile's last
        lse, loss, stats, dx = run_pair(dev, c, g=0.5, rows=[r])
        assert torch.equal(lse[0], a[0][r]) and torch.equal(loss[0], a[1][r]) and torch.equal(dx[0], a[3][r]), r
    rows = list(range(60, 70))    # ... and a run of rows that lands at other places of other tiles
    lse, loss, stats, dx = run_pair(dev, c, g=0.5, rows=rows)
    assert torch.equal(lse, a[0][rows]) and torch.equal(loss, a[1][rows]) and torch.equal(dx, a[3][rows])


def _peak(dev, fn):
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - base, out


def test_memory_does_not_grow_with_rows_times_vocabulary(dev):
    """R 4096 x V 4096: one [R, V] float32 tensor is 64 MiB.  The fused node stays below half of that (its live tensors -- dx, the packed head,
    the per-row vectors -- add up to about 15 MiB); the chain it replaces, run here too, exceeds 64 MiB, so the bound discriminates."""
    from slotformer_amd import train
    R, V, K = 4096, 4096, 192
    gen = torch.Generator().manual_seed(9)
    head = torch.nn.Linear(K, V, bias=False).to(dev)
    with torch.no_grad():
        head.weight.copy_(torch.randn(V, K, generator=gen) / K**0.5)
    x0 = (torch.randn(R, K, generator=gen) * 2).to(dev)
    t = torch.randint(0, V, (R, ), generator=gen).to(dev)

    def fused():
        x = x0.clone().requires_grad_(True)
        loss, _ = train.head_cross_entropy(x, head, t)
        loss.backward()
        return float(loss.detach()), x.grad.cpu()

    def chain():
        x = x0.clone().requires_grad_(True)
        loss = train.token_cross_entropy(train.linear(x, head), t)
        loss.backward()
        return float(loss.detach()), x.grad.cpu()

    head.weight.requires_grad_(False)
    fused_peak, (fl, fdx) = _peak(dev, fused)
    head.weight.requires_grad_(True)
    chain_peak, (cl, cdx) = _peak(dev, chain)
    print(f'head_ce memory R {R} V {V} K {K}: fused peak {fused_peak / 2**20:.1f} MiB, chain peak {chain_peak / 2**20:.1f} MiB')
    assert fused_peak < R * V * 4 // 2
    assert chain_peak > R * V * 4
    # the two forms are the same function (each is held to float64 elsewhere)
    assert abs(fl - cl) < TOL * cl and l2_err(fdx, cdx) < 2 * L2TOL


def test_head_that_requires_grad_is_refused(dev):
    from slotformer_amd import train
    head = torch.nn.Linear(64, 64, bias=False).to(dev)
    x = torch.randn(8, 64, device=dev, requires_grad=True)
    t = torch.zeros(8, dtype=torch.int64, device=dev)
    with pytest.raises(NotImplementedError, match='weight gradient'):
        train.head_cross_entropy(x, head, t)
    head.weight.requires_grad_(False)
    loss, stats = train.head_cross_entropy(x, head, t)
    loss.backward()
    assert x.grad is not None and float(stats[1]) == 8
    # the packed copy follows the weight
    with torch.no_grad():
        head.weight.mul_(2.)
    loss2, _ = train.head_cross_entropy(x, head, t)
    want = torch.nn.functional.cross_entropy(x.detach().cpu().double() @ head.weight.cpu().double().t(), t.cpu())
    assert abs(float(loss2.detach()) - float(want)) < TOL * float(want)
    # a bare [V, K] tensor in place of the module: the same bits
    loss3, _ = train.head_cross_entropy(x, head.weight.detach(), t)
    assert torch.equal(loss3.detach(), loss2.detach())


# ---- the reference's own numbers ---------------------------------------------------------------------------------------------------------------
def _steve_slotformer(dev, tmp_path, sd_seed=None, golden=None):
    """The STEVESlotFormer of test_train_gpu.py::test_steve_slotformer_training_vs_oracle: the reduced Physion configuration (V 64, d 64,
    16 x 16 tokens, burn-in 3 + 2) on a STEVE checkpoint of seeded weights."""
    from slotformer_amd.base_slots import build_model as bb
    from slotformer_amd.video_prediction import build_model as bv
    steve = bb(gu.ParamsView(gu.steve_tokens_cfg()))
    path = str(tmp_path / 'steve.pth')
    torch.save({'state_dict': steve.state_dict()}, path)
    cfg = gu.steve_slotformer_cfg()
    cfg['dec_dict']['dec_ckp_path'] = path
    m = bv(gu.ParamsView(cfg))
    sd = None
    if golden is not None:
        sd = gu.seeded_state_dict(gu.shapes_from_golden(golden), sd_seed, keep=dict(m.state_dict()))
        m.load_state_dict(sd, strict=True)
    return m.to(dev), cfg, sd


def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.


def test_fused_token_loss_vs_oracle(dev, tmp_path):
    """The fixture of test_steve_slotformer_training_vs_oracle (same seeds, the reference's target_token_id): the fused loss on
    slate_decoder_hidden against the reference's img_recon_loss, the rollouter gradients of (slot MSE + fused token loss) against the oracle's
    autograd."""
    from slotformer_amd import train
    g = gu.load_golden('steve_slotformer')
    m, cfg, sd = _steve_slotformer(dev, tmp_path, 701, g)
    m.train()
    _no_dropout(m)
    rd = cfg['rollout_dict']
    hist, S = rd['history_len'], cfg['loss_dict']['rollout_len']
    slots = gu.seeded_normal((1, hist + S, rd['num_slots'], rd['slot_size']), 702)
    tok = torch.from_numpy(g['target_token_id']).to(torch.int64)                  # [S, h*w], the reference's targets
    sl = slots.to(dev)
    pred = m.rollout(sl[:, :hist], S)
    hidden = train.slate_decoder_hidden(m.decoder, pred.flatten(0, 1), tok.to(dev)[:, :-1].contiguous())
    assert hidden.shape[:2] == tok.shape
    img, stats = train.head_cross_entropy(hidden, m.decoder.head, tok.to(dev))
    e = abs(float(img.detach()) - float(g['img_recon_loss'])) / float(g['img_recon_loss'])
    print(f'head_ce vs the reference: img_recon_loss {float(img.detach()):.6f} / {float(g["img_recon_loss"]):.6f} (rel {e:.3g})')
    assert e < 1e-3 and float(stats[1]) == tok.numel()
    (((pred - sl[:, hist:])**2).mean() + img).backward()
    names = [n for n, p_ in m.named_parameters() if p_.requires_grad]
    assert names and all(n.startswith('rollouter.') for n in names)
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    opred = oracle.rollouter_forward(slots[:, :hist], S, osd, rd)
    dd = cfg['dec_dict']
    logits = oracle.steve_decoder_forward(opred.flatten(0, 1), tok[:, :-1], osd, dd['dec_num_heads'], dd['dec_num_layers'], p='decoder.')
    (((opred - slots[:, hist:])**2).mean() + torch.nn.functional.cross_entropy(logits.flatten(0, 1), tok.flatten(0, 1))).backward()
    got = dict(m.named_parameters())
    worst = max(l2_err(got[n].grad, osd[n].grad) for n in names)
    print(f'head_ce vs the oracle: worst rollouter gradient (l2) {worst:.3g}')
    for n in names:
        assert l2_err(got[n].grad, osd[n].grad) < L2TOL, n
    assert all(p_.grad is None for n, p_ in m.named_parameters() if not n.startswith('rollouter.'))


# ---- fit / evaluate with tokens= ------------------------------------------------------------------------------------------------------------------
NV, NT, HIST, S = 3, 8, 3, 2


def _tables(cfg, hw):
    gen = torch.Generator().manual_seed(31)
    rd = cfg['rollout_dict']
    table = torch.randn(NV, NT, rd['num_slots'], rd['slot_size'], generator=gen)
    tokens = torch.randint(0, cfg['dvae_dict']['vocab_size'], (NV, NT, hw), generator=gen).to(torch.int16)
    return table, tokens


def _gather(t, clips, n, f, first=0):
    return torch.stack([torch.stack([t[int(v), int(s) + (first + j) * f] for j in range(n)]) for v, s in clips.tolist()])


@pytest.mark.parametrize('clip_len', [None, [5, 4, 5]], ids=['whole', 'truncated'])
def test_fit_step_with_tokens_equals_the_module_path(dev, tmp_path, clip_len):
    """One step of fit(tokens=): the gradient that reaches the optimiser's bucket against the module path (model(data), the token cross-entropy of
    its logits, backward) on the same clips -- with clip_len, on the frames that count: clip 1 keeps the first of its two predicted frames."""
    from slotformer_amd import train, video_prediction as vp
    torch.manual_seed(5)
    model, cfg, _ = _steve_slotformer(dev, tmp_path)
    model.train()
    _no_dropout(model)
    hw = model.h * model.w
    assert (hw, model.decoder.head.weight.shape[0], HIST, S) == (256, 64, model.history_len, model.rollout_len)
    table, tokens = _tables(cfg, hw)
    f = 1
    clips = torch.tensor([[2, 3], [0, 0], [2, 1]])
    B = clips.shape[0]
    opt = train.FlatAdam(train.rollouter_parameters(model.rollouter) + train.learnable_tables(model.rollouter), lr=1e-3)
    td, kd = table.to(dev), tokens.to(dev)
    cv, cs = clips[:, 0].to(torch.int32).to(dev), clips[:, 1].to(torch.int32).to(dev)
    cl = None if clip_len is None else torch.tensor(clip_len, dtype=torch.int32, device=dev)
    fw = None if cl is None else vp._frame_weights(cl, HIST, S)
    pred, slot_loss, tok_loss, _, ce = vp._token_step(model, td, kd, cv, cs, f, HIST, S, 0, opt.grad, None, cl, fw, (1., 1.))
    (slot_loss + tok_loss).backward()
    bucket = opt.grad.clone()
    for p in opt.params:
        p.grad = None
    # the module path
    ids = _gather(tokens, clips, S, f, HIST).long()                       # [B, S, hw]
    data = {'slots': _gather(table, clips, HIST + S, f).to(dev), 'token_id': ids.to(dev)}
    out = model(data)
    assert torch.equal(pred, out['pred_slots'])
    keep = torch.ones(B, S, dtype=torch.bool) if clip_len is None else (HIST + torch.arange(S))[None] < torch.tensor(clip_len)[:, None]
    assert int(keep.sum()) == (B * S if clip_len is None else B * S - 1)
    kf = keep.flatten().to(dev)
    if clip_len is None:
        terms = model.calc_train_loss(data, out)
        want_slot, want_tok = terms['slot_recon_loss'], terms['img_recon_loss']
    else:
        sq = ((out['pred_slots'] - out['gt_slots'])**2).flatten(0, 1)[kf]
        want_slot = sq.mean()
        want_tok = train.token_cross_entropy(out['pred_token_id'][kf].flatten(0, 1).contiguous(), out['target_token_id'][kf].flatten().contiguous())
    (want_slot + want_tok).backward()
    e = (abs(float(slot_loss.detach()) - float(want_slot.detach())) / float(want_slot.detach()),
         abs(float(ce) - float(want_tok.detach())) / float(want_tok.detach()),
         l2_err(bucket, torch.cat([p.grad.reshape(-1) for p in opt.params])))
    print(f'fit step with tokens ({"whole" if clip_len is None else "truncated"}): slot loss {e[0]:.3g} token loss {e[1]:.3g} bucket (l2) {e[2]:.3g}')
    assert e[0] < 1e-5 and e[1] < TOL and e[2] < L2TOL
    assert all(p.grad is None for p in model.decoder.parameters())


def test_fit_and_evaluate_with_tokens(dev, tmp_path):
    from slotformer_amd import train, video_prediction as vp
    f = 1

    def run(seed):
        torch.manual_seed(5)
        model, cfg, _ = _steve_slotformer(dev, tmp_path)
        table, tokens = _tables(cfg, model.h * model.w)
        clips = vp.clip_index(NV, NT, HIST + S, f, 'train')
        assert clips.shape[0] == 12
        before = torch.cat([p.detach().reshape(-1) for p in train.rollouter_parameters(model.rollouter)]).clone()
        lens = [5] * 11 + [4]
        out = vp.fit(model, table.to(dev), clips, 2, 4, 1e-3, seed, f, tokens=tokens.to(dev), clip_len=lens)
        after = torch.cat([p.detach().reshape(-1) for p in train.rollouter_parameters(model.rollouter)]).clone()
        return model, out, before, after, (table, tokens, clips)

    model, a, before, pa, (table, tokens, clips) = run(7)
    _, b, _, pb, _ = run(7)
    assert a['img_loss'].shape == (2, ) and bool(torch.isfinite(a['img_loss']).all()) and bool(torch.isfinite(a['loss']).all())
    assert a['state']['step'] == 6 and not torch.equal(before, pa)
    assert torch.equal(pa, pb) and torch.equal(a['img_loss'], b['img_loss']) and torch.equal(a['loss'], b['loss'])   # one seed, one result
    assert all(p.grad is None for p in model.decoder.parameters())
    # evaluate: the eval-mode module path on gathered clips
    model.eval()
    td, kd = table.to(dev), tokens.to(dev)
    got = vp.evaluate(model, td, clips, 5, f, tokens=kd.long())      # int64 ids, a ragged last batch
    data = {'slots': _gather(table, clips, HIST + S, f).to(dev), 'token_id': _gather(tokens, clips, S, f, HIST).long().to(dev)}
    with torch.no_grad():
        terms = model.calc_train_loss(data, model(data))
    want = float(terms['img_recon_loss'])
    print(f'evaluate with tokens: img_recon_loss {got["img_recon_loss"]:.6f} / {want:.6f}')
    assert abs(got['img_recon_loss'] - want) < TOL * want
    assert abs(got['slot_recon_loss'] - float(terms['slot_recon_loss'])) <= 1e-6 * float(terms['slot_recon_loss'])
    assert vp.evaluate(model, td, clips, 5, f, tokens=kd)['img_recon_loss'] == got['img_recon_loss']   # int16 ids: the same bits
    assert 'img_recon_loss' not in vp.evaluate(model, td, clips, 5, f)
    # the argument checks, before any loop
    with pytest.raises(ValueError, match='int16 or int64'):
        vp.fit(model, td, clips, 1, 4, 1e-3, 1, f, tokens=kd.float())
    with pytest.raises(ValueError, match='int16 or int64'):
        vp.fit(model, td, clips, 1, 4, 1e-3, 1, f, tokens=kd[:, :-1])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vp.fit(model, td, clips, 1, 4, 1e-3, 1, f, tokens=tokens)
    with pytest.raises(NotImplementedError, match='tokens='):
        vp.fit(model, td, clips, 1, 4, 1e-3, 1, f, frames=torch.zeros(NV, NT, 64, 64, 3, dtype=torch.uint8, device=dev))
    import slotformer_fit_cases as fc
    savi = fc.build_model(fc.decoder_checkpoint(str(tmp_path / 'dec.pth'))).to(dev)
    with pytest.raises(ValueError, match='no dVAE'):
        vp.fit(savi, fc.seeded_table().to(dev), vp.clip_index(fc.V, fc.T, fc.HIST + fc.S, 1, 'train'), 1, 8, 1e-3, 1, 1,
               tokens=torch.zeros(fc.V, fc.T, 4, dtype=torch.int16, device=dev))
