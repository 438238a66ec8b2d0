"""GPU: SlotFormer training from a device-resident slot table (video_prediction.fit / evaluate, csrc/clip_train.hip, the FlatAdam additions).
Only data movement is new in the clip forward and in the gradient's way into the optimiser's bucket, so those are held to torch.equal against the
module path; the fused loss is held to a float64 restatement of slotformer.py:289-318."""
import numpy as np
import pytest
import torch

import slotformer_fit_cases as fc

pytestmark = pytest.mark.gpu

HIST, S, N, C = fc.HIST, fc.S, fc.N, fc.C


def rel_err(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max()).item()


def l2_err(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return ((a - b).norm() / b.norm()).item()


def _rollouter(dev, seed=3, single_step=False, **over):
    from slotformer_amd.video_prediction.models import SlotRollouter, SingleStepSlotRollouter
    torch.manual_seed(seed)
    cfg = dict(fc.ROLL, **over)
    if single_step:
        cfg.update(history_len=1, cond_len=2)
        return SingleStepSlotRollouter(**cfg).to(dev)
    return SlotRollouter(**cfg).to(dev)


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


def _clips_for(f, B, n_frames, T):
    """B = 3: out of video order, the same clip twice, and that clip ends on the table's last frame; B = 1: the clip that ends on the last frame."""
    last = T - 1 - (n_frames - 1) * f
    assert last >= 0
    return torch.tensor([[3, last], [0, 1 if last >= 1 else 0], [3, last]][:B] if B == 3 else [[2, last]])


@pytest.fixture(scope='module')
def ckpt(tmp_path_factory):
    return fc.decoder_checkpoint(str(tmp_path_factory.mktemp('fit') / 'dec.pth'))


# ---- 1. the clip forward is the module forward on a gathered copy, bit for bit -------------------------------------------------------------
@pytest.mark.parametrize('p_drop', [0., 0.1])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('f', [1, 2, 3])
def test_clip_forward_equals_gathered(dev, f, B, p_drop):
    """(V 4 x T 12 holds 2 + 3 frames at offsets 1 and 2; at offset 3 they span 13 frames, so those cases take a table of T 13.)"""
    from slotformer_amd import train
    T = max(fc.T, (HIST + S - 1) * f + 1)
    table = fc.seeded_table(t=T)
    clips = _clips_for(f, B, HIST + S, T)
    r = _rollouter(dev)
    r.train(p_drop > 0)
    for layer in r.transformer_encoder.layers:
        assert layer.dropout.p == 0.1
    r.dropout_seed_override = 1234
    want = train.rollout_with_grad(r, fc.gather_clips(table, clips, HIST, f).to(dev), S)
    got = train.rollout_clips_with_grad(r, table.to(dev), _i32(clips[:, 0].tolist(), dev), _i32(clips[:, 1].tolist(), dev), f, S)
    assert got.shape == (B, S, N, C) and torch.equal(got, want)
    if p_drop > 0:   # (the masks were on: another seed gives another prediction)
        other = train.rollout_clips_with_grad(r, table.to(dev), _i32(clips[:, 0].tolist(), dev), _i32(clips[:, 1].tolist(), dev), f, S, seed=99)
        assert not torch.equal(other, want)


@pytest.mark.parametrize('f', [1, 2])
def test_clip_forward_single_step(dev, f):
    """The single-step rollouter (cond_len 2): the burn-in is ONE frame, the window grows to two."""
    from slotformer_amd import train
    table = fc.seeded_table()
    clips = _clips_for(f, 3, 1 + S, fc.T)
    r = _rollouter(dev, single_step=True).eval()
    assert train.burnin_len(r) == 1
    want = train.rollout_with_grad(r, fc.gather_clips(table, clips, 1, f).to(dev), S)
    got = train.rollout_clips_with_grad(r, table.to(dev), _i32(clips[:, 0].tolist(), dev), _i32(clips[:, 1].tolist(), dev), f, S)
    assert torch.equal(got, want)


# ---- 2. the fused loss against float64 ------------------------------------------------------------------------------------------------------
def _ulp32(x):
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32)).astype(np.float64))


MSE_CASES = [   # B, S, N, C, decay, clip_len
    (3, 3, 3, 64, None, None),                 # B * E / 4 = 144 float4s: not a multiple of the 256-thread tile
    (3, 3, 3, 64, 0.5, None),
    (2, 1, 3, 64, 0.5, None),                  # S = 1
    (5, 7, 7, 128, 0.5, None),                 # 1120 float4s per step: five workgroups per step
    (5, 7, 7, 128, None, [9, 2, 5, 4, 100]),   # hist 2: 7, 0, 3, 2, 7 steps count -- a clip with none
    (3, 3, 3, 64, 0.5, [3, 5, 2]),
]


@pytest.mark.parametrize('where', ['dense', 'table'])
@pytest.mark.parametrize('B,S_,N_,C_,decay,clip_len', MSE_CASES)
def test_clip_mse_against_float64(dev, B, S_, N_, C_, decay, clip_len, where):
    """d_pred per element within 4 * 2**-24 * max|pred - target| * scale * w_s / count plus one float32 ulp of the value (the kernel rounds three
    times: the difference, the coefficient scale * w_s * 2 / count, their product); loss and per-step sums within 1e-6 relative."""
    from slotformer_amd import train
    g = torch.Generator().manual_seed(B * 100 + S_)
    f, hist, scale = 2, 2, 0.7
    T = (hist + S_ - 1) * f + 3
    table = torch.randn(4, T, N_, C_, generator=g)
    clips = torch.stack([torch.randint(0, 4, (B, ), generator=g), torch.randint(0, 3, (B, ), generator=g)], 1)
    target = fc.gather_clips(table, clips, hist + S_, f)[:, hist:].contiguous()
    pred = target + torch.randn(B, S_, N_, C_, generator=g) * 0.3
    w = None
    if decay is not None:
        w = torch.tensor(decay, dtype=torch.float64)**torch.arange(S_, dtype=torch.float64)
        w = (w / w.sum() * S_).float()
    cl = None if clip_len is None else torch.tensor(clip_len, dtype=torch.int32)
    loss_ref, d_ref, sums_ref, counts_ref, count = fc.mse_reference(pred, target, hist, w, cl, scale)

    def run():
        p = pred.to(dev).requires_grad_(True)
        kw = dict(hist=hist, step_w=None if w is None else w.to(dev), clip_len=None if cl is None else cl.to(dev), scale=scale)
        if where == 'dense':
            loss, stats = train.clip_mse(p, target.to(dev), **kw)
        else:
            loss, stats = train.clip_mse(p, table.to(dev), _i32(clips[:, 0].tolist(), dev), _i32(clips[:, 1].tolist(), dev), f, **kw)
        loss.backward()
        return loss.detach(), stats, p.grad

    loss, stats, d = run()
    loss2, stats2, d2 = run()
    assert torch.equal(loss, loss2) and torch.equal(stats, stats2) and torch.equal(d, d2)   # the same bits from call to call
    stats, d = stats.cpu(), d.cpu().double()
    maxdiff = float((pred.double() - target.double()).abs().max())
    wv = torch.ones(S_, dtype=torch.float64) if w is None else w.double()
    bound = 4 * 2.**-24 * maxdiff * scale * wv.view(1, S_, 1, 1) / count + _ulp32(d_ref)
    err = (d - d_ref).abs()
    print(f'max |d_pred - f64| / bound = {float((err / bound).max()):.3g}; loss rel {abs(float(stats[0]) - loss_ref) / loss_ref:.3g}')
    assert bool((err <= bound).all())
    assert abs(float(stats[0]) - loss_ref) <= 1e-6 * loss_ref and abs(float(loss) - loss_ref) <= 1e-6 * loss_ref
    assert bool(((stats[1:1 + S_] - sums_ref).abs() <= 1e-6 * sums_ref).all())
    assert torch.equal(stats[1 + S_:], counts_ref)
    if cl is not None:   # masked steps carry no gradient
        keep = (torch.arange(S_)[None] + hist) < cl.long()[:, None]
        assert float(d[~keep].abs().max()) == 0.


# ---- 3. the weight gradients land in the optimiser's bucket, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize('t_pe', ['sin', 'learnable'])
def test_clip_backward_fills_the_bucket(dev, t_pe):
    from slotformer_amd import train
    f = 2
    table = fc.seeded_table()
    clips = _clips_for(f, 3, HIST + S, fc.T)
    r = _rollouter(dev, t_pe=t_pe).eval()
    if t_pe == 'learnable':
        with torch.no_grad():
            r.enc_t_pe.normal_()
    params = train.rollouter_parameters(r) + train.learnable_tables(r)
    assert len(train.learnable_tables(r)) == (1 if t_pe == 'learnable' else 0)
    opt = train.FlatAdam(params, lr=1e-3)
    td, cv, cs = table.to(dev), _i32(clips[:, 0].tolist(), dev), _i32(clips[:, 1].tolist(), dev)
    pred = train.rollout_clips_with_grad(r, td, cv, cs, f, S, grad_out=opt.grad)
    pred.retain_grad()
    loss, _ = train.clip_mse(pred, td, cv, cs, f, HIST)
    loss.backward()
    assert all(p.grad is None for p in params)   # the bucket holds them
    d_pred = pred.grad.clone()
    bucket = opt.grad.clone()
    # the module path on a gathered copy, fed the fused kernel's d_pred
    pred2 = train.rollout_with_grad(r, fc.gather_clips(table, clips, HIST, f).to(dev), S)
    assert torch.equal(pred2, pred)
    pred2.backward(d_pred)
    want = torch.cat([p.grad.reshape(-1) for p in params])
    assert torch.equal(bucket, want)
    off = 0
    for p in opt.params:   # ... and they are what the optimiser's views show
        assert torch.equal(opt.grad[off:off + p.numel()].view_as(p), p.grad)
        off += p.numel()
    assert float(bucket.abs().max()) > 0


# ---- 4. step(gathered=True) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clip_grad', [None, 0.05])
def test_step_gathered_equals_step(dev, clip_grad):
    from slotformer_amd import train
    a, b = _rollouter(dev), _rollouter(dev)
    oa = train.FlatAdam(train.rollouter_parameters(a), lr=2e-3, clip_grad=clip_grad)
    ob = train.FlatAdam(train.rollouter_parameters(b), lr=2e-3, clip_grad=clip_grad)
    assert torch.equal(oa.flat, ob.flat)
    for step in range(3):
        g = (torch.randn(oa.flat.numel(), generator=torch.Generator().manual_seed(50 + step)) * 0.1).to(dev)
        off = 0
        for p in oa.params:
            p.grad = g[off:off + p.numel()].view_as(p).clone()
            off += p.numel()
        ob.grad.copy_(g)
        oa.step()
        ob.step(gathered=True)
        assert torch.equal(oa.flat, ob.flat) and torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
    assert all(p._version == q._version for p, q in zip(oa.params, ob.params))


# ---- 5. state dicts ---------------------------------------------------------------------------------------------------------------------------
def test_state_dict_exchanges_with_torch_adam(dev):
    """A torch.optim.Adam state dict taken after two steps loads into FlatAdam and the third step agrees with torch's (1e-5, the bar
    test_flat_adam_gpu.py holds one step to); FlatAdam's own state dict loads into torch.optim.Adam the same way."""
    from slotformer_amd import train
    a, b = _rollouter(dev), _rollouter(dev)
    pa, pb = train.rollouter_parameters(a), train.rollouter_parameters(b)
    ref = torch.optim.Adam(pa, lr=2e-4)
    grads = [[(torch.randn(p.shape, generator=torch.Generator().manual_seed(70 + s * 100 + i)) * 0.1).to(dev) for i, p in enumerate(pa)]
             for s in range(4)]

    def torch_step(s):
        for p, g in zip(pa, grads[s]):
            p.grad = g.clone()
        ref.step()

    torch_step(0)
    torch_step(1)
    with torch.no_grad():
        for p, q in zip(pa, pb):
            q.copy_(p)
    opt = train.FlatAdam(pb, lr=1.)   # (the rate comes from the state dict)
    opt.load_state_dict(ref.state_dict())
    assert opt.steps == 2 and opt.lr == 2e-4
    torch_step(2)
    for p, g in zip(opt.params, grads[2]):
        p.grad = g.clone()
    opt.step()
    for p, q in zip(pa, pb):
        assert rel_err(q, p.detach().cpu()) < 1e-5
    # ... and back: torch's Adam resumes from FlatAdam's state dict
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups'} and sd['param_groups'][0]['params'] == list(range(len(pb)))
    assert sd['param_groups'][0]['weight_decay'] == 0 and sd['param_groups'][0]['amsgrad'] is False and sd['param_groups'][0]['betas'] == (0.9, 0.999)
    assert float(sd['state'][0]['step']) == 3. and sd['state'][0]['exp_avg'].shape == pb[0].shape
    c = _rollouter(dev)
    pc = train.rollouter_parameters(c)
    with torch.no_grad():
        for p, q in zip(pb, pc):
            q.copy_(p)
    back = torch.optim.Adam(pc, lr=1.)
    back.load_state_dict(sd)
    for p, g in zip(pc, grads[3]):
        p.grad = g.clone()
    back.step()
    torch_step(3)
    for p, q in zip(pa, pc):
        assert rel_err(q, p.detach().cpu()) < 1e-5
    bad = ref.state_dict()
    bad['param_groups'][0]['weight_decay'] = 0.1
    with pytest.raises(ValueError):
        opt.load_state_dict(bad)


# ---- 6. target frames ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', [(8, 8), (16, 8)])
def test_clip_frames_equal_ingest(dev, H, W):
    from slotformer_amd import train
    from slotformer_amd.ingest import FrameIngest
    f = 2
    frames = torch.randint(0, 256, (fc.V, fc.T, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H))
    clips = _clips_for(f, 3, HIST + S, fc.T)   # (the repeated clip ends on the table's last frame)
    mean, std = (0.4, 0.5, 0.6), (0.5, 0.25, 0.3)
    got = train.clip_frames(frames.to(dev), _i32(clips[:, 0].tolist(), dev), _i32(clips[:, 1].tolist(), dev), f, HIST, S, mean, std)
    gathered = fc.gather_clips(frames, clips, HIST + S, f)[:, HIST:].contiguous()
    want = FrameIngest((H, W), mean=mean, std=std).ingest(gathered.to(dev))
    assert got.shape == (3, S, 3, H, W) and torch.equal(got, want)
    one = train.clip_frames(frames.to(dev), _i32(clips[:, 0].tolist(), dev), _i32(clips[:, 1].tolist(), dev), f, HIST, S)
    assert torch.equal(one, FrameIngest((H, W)).ingest(gathered.to(dev)))


# ---- 7. fit -----------------------------------------------------------------------------------------------------------------------------------
def _rotating_table():
    """Every slot turns by one fixed orthogonal map per frame: x[t + 1] = Q x[t]."""
    g = torch.Generator().manual_seed(21)
    q, _ = torch.linalg.qr(torch.randn(C, C, generator=g, dtype=torch.float64))
    x = torch.randn(fc.V, N, C, generator=g, dtype=torch.float64)
    frames = [x]
    for _ in range(fc.T - 1):
        frames.append(frames[-1] @ q.T)
    return torch.stack(frames, 1).float().contiguous()


def _fit(ckpt, dev, table, clips, seed, **kw):
    from slotformer_amd import train, video_prediction as vp
    model = fc.build_model(ckpt).to(dev)
    out = vp.fit(model, table, clips, kw.pop('epochs', 30), 8, 2e-3, seed, 1, **kw)
    return model, out, torch.cat([p.detach().reshape(-1) for p in train.rollouter_parameters(model.rollouter)]).clone()


def test_fit_learns_planted_dynamics(dev, ckpt):
    from slotformer_amd import video_prediction as vp
    table = _rotating_table().to(dev)
    clips = vp.clip_index(fc.V, fc.T, HIST + S, 1, 'train')
    assert clips.shape[0] == 32
    _, a, pa = _fit(ckpt, dev, table, clips, 7, loss_decay_pct=0.2, clip_grad=1.0)
    loss = a['loss'].cpu()
    print(f'fit: first epoch loss {float(loss[0]):.6g}, last {float(loss[-1]):.6g}')
    assert loss.shape == (30, ) and bool(torch.isfinite(loss).all()) and float(loss[-1]) < float(loss[0])
    assert a['img_loss'] is None and a['state']['step'] == 120
    _, b, pb = _fit(ckpt, dev, table, clips, 7, loss_decay_pct=0.2, clip_grad=1.0)
    assert torch.equal(pa, pb) and torch.equal(a['loss'], b['loss'])           # one seed, one result
    _, c, pc = _fit(ckpt, dev, table, clips, 8, loss_decay_pct=0.2, clip_grad=1.0)
    assert not torch.equal(pa, pc) and not torch.equal(a['loss'], c['loss'])


def test_fit_resume_reproduces_the_straight_run(dev, ckpt):
    """Two epochs straight through, against one epoch, the state saved, a fresh model and optimiser, the state loaded, the second epoch."""
    from slotformer_amd import train, video_prediction as vp
    table = _rotating_table().to(dev)
    clips = vp.clip_index(fc.V, fc.T, HIST + S, 1, 'train')
    _, straight, p2 = _fit(ckpt, dev, table, clips, 7, epochs=2)
    first_model, first, _ = _fit(ckpt, dev, table, clips, 7, epochs=2, stop_after=1)
    assert first['state']['step'] == 4 and first['loss'].shape == (1, )
    fresh = fc.build_model(ckpt).to(dev)
    fresh.rollouter.load_state_dict(first_model.rollouter.state_dict())
    second = vp.fit(fresh, table, clips, 2, 8, 2e-3, 7, 1, resume=first['state'])
    got = torch.cat([p.detach().reshape(-1) for p in train.rollouter_parameters(fresh.rollouter)])
    assert torch.equal(got, p2)
    assert torch.equal(torch.cat([first['loss'], second['loss']]), straight['loss'])
    assert second['state']['step'] == 8
    with pytest.raises(ValueError):
        vp.fit(fresh, table, clips, 2, 8, 2e-3, 8, 1, resume=first['state'])
    with pytest.raises(ValueError):   # a clip that leaves the table is caught on the host, before the loop
        vp.fit(fresh, table, torch.tensor([[0, fc.T - 4]] * 8), 1, 8, 2e-3, 7, 1)


def test_fit_image_loss_step(dev, ckpt):
    """With the decoder (a 2x2 grid to 8x8) and frames=: the gradient that reaches pred_slots in one step of `fit` against the module path's
    (forward, calc_train_loss, backward on gathered clips), within the 1e-2 (L2) that test_train_gpu.py holds the decode node to; then a run."""
    from slotformer_amd import train, video_prediction as vp
    from slotformer_amd.ingest import FrameIngest
    f = 1
    table = _rotating_table()
    frames = torch.randint(0, 256, (fc.V, fc.T, fc.RES, fc.RES, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    clips = _clips_for(f, 3, HIST + S, fc.T)
    model = fc.build_model(ckpt, img=True).to(dev).train()
    fc.no_dropout(model)
    r = model.rollouter
    opt = train.FlatAdam(train.rollouter_parameters(r), lr=1e-3)
    td, fd, cv, cs = table.to(dev), frames.to(dev), _i32(clips[:, 0].tolist(), dev), _i32(clips[:, 1].tolist(), dev)
    pred, slot_loss, img_loss, _, _ = vp._image_step(model, td, fd, cv, cs, f, HIST, S, 0, opt.grad, None, None, 0.5, 0.5, (1., 1.))
    pred.retain_grad()
    (slot_loss + img_loss).backward()
    bucket = opt.grad.clone()
    data = {'slots': fc.gather_clips(table, clips, HIST + S, f).to(dev),
            'img': FrameIngest((fc.RES, fc.RES)).ingest(fc.gather_clips(frames, clips, HIST + S, f).to(dev))}
    out = model(data)
    out['pred_slots'].retain_grad()
    terms = model.calc_train_loss(data, out)
    (terms['slot_recon_loss'] + terms['img_recon_loss']).backward()
    assert torch.equal(pred, out['pred_slots'])
    want_slot, want_img = float(terms['slot_recon_loss'].detach()), float(terms['img_recon_loss'].detach())
    assert abs(float(slot_loss.detach()) - want_slot) <= 1e-6 * want_slot
    assert abs(float(img_loss.detach()) - want_img) <= 1e-5 * want_img
    assert l2_err(pred.grad, out['pred_slots'].grad.cpu()) < 1e-2
    assert l2_err(bucket, torch.cat([p.grad.reshape(-1) for p in opt.params]).cpu()) < 1e-2
    # ... and the loop itself, with frames
    model2 = fc.build_model(ckpt, img=True).to(dev)
    res = vp.fit(model2, td, vp.clip_index(fc.V, fc.T, HIST + S, 1, 'train'), 2, 8, 1e-3, 3, 1, frames=fd)
    assert res['img_loss'].shape == (2, ) and bool(torch.isfinite(res['img_loss']).all()) and bool(torch.isfinite(res['loss']).all())
    assert all(p.grad is None for p in model2.decoder.parameters())


# ---- 8. evaluate ------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_equals_module_path(dev, ckpt):
    from slotformer_amd import video_prediction as vp
    f = 2
    table = fc.seeded_table()
    clips = vp.clip_index(fc.V, fc.T, HIST + S, f, 'train')   # 4 starts x 4 videos; batches of 5: the last one is ragged
    assert clips.shape[0] == 16
    model = fc.build_model(ckpt).to(dev).eval()
    got = vp.evaluate(model, table.to(dev), clips, 5, f)
    data = {'slots': fc.gather_clips(table, clips, HIST + S, f).to(dev)}
    terms = model.calc_train_loss(data, model(data))
    assert set(got) == {'slot_recon_loss', 'slot_recon_loss_1', 'slot_recon_loss_2', 'slot_recon_loss_3'}
    for k, v in got.items():
        assert abs(v - float(terms[k].detach())) <= 1e-6 * float(terms[k].detach()), k
    # the vid_len truncation: clips of 4 frames count two of their three steps
    short = vp.evaluate(model, table.to(dev), clips, 16, f, clip_len=[4] * 16)
    want = (got['slot_recon_loss_1'] + got['slot_recon_loss_2']) / 2
    assert abs(short['slot_recon_loss'] - want) <= 1e-6 * want


def test_fit_and_evaluate_single_step(dev, ckpt):
    """SingleStepSlotFormer (burn-in of ONE frame, the window grows to cond_len 2): `fit` runs and repeats itself, `evaluate` equals the module path."""
    from slotformer_amd import train, video_prediction as vp
    f = 2
    table = fc.seeded_table()
    clips = vp.clip_index(fc.V, fc.T, 1 + S, f, 'train')   # 4 frames 2 apart: starts 0..5 of 4 videos
    assert clips.shape[0] == 24

    def run():
        model = fc.build_model(ckpt, single_step=True).to(dev)
        out = vp.fit(model, table.to(dev), clips, 2, 8, 1e-3, 5, f)
        return model, out, torch.cat([p.detach().reshape(-1) for p in train.rollouter_parameters(model.rollouter)]).clone()

    model, a, pa = run()
    _, b, pb = run()
    assert a['loss'].shape == (2, ) and bool(torch.isfinite(a['loss']).all()) and a['state']['step'] == 6
    assert torch.equal(pa, pb) and torch.equal(a['loss'], b['loss'])
    model.eval()
    got = vp.evaluate(model, table.to(dev), clips, 7, f)
    data = {'slots': fc.gather_clips(table, clips, 1 + S, f).to(dev)}
    terms = model.calc_train_loss(data, model(data))
    for k, v in got.items():
        assert abs(v - float(terms[k].detach())) <= 1e-6 * float(terms[k].detach()), k
