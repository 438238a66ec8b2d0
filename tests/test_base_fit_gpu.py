"""GPU: `base_slots.fit` / `evaluate` and what they add underneath -- the in-kernel normal noise against its host twin, the sampling + KL node
against float64, and the loop against the same steps written by hand with the module calls.  Shapes are the smallest the kernels and models take
(tests/base_fit_cases.py): 64 x 64 frames, 4 videos of 6 frames, batches of 2 clips x 2 frames.  Figures measured on an MI355X are quoted in the
docstrings and in profiles/base_fit.md; every test prints its own before it asserts."""
import math

import numpy as np
import pytest
import torch

import base_fit_cases as bc

pytestmark = pytest.mark.gpu

U = 2.**-24   # half an ulp of float32, relative: one rounding


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.fixture(scope='module')
def frames(dev):
    return bc.smooth_frames().to(dev)


def gather(frames, clips, idx, n_frames=bc.N_FRAMES):
    """(cv, cs, img) of the clips `idx`: the batch as fit gathers it"""
    from slotformer_amd import train
    dev = frames.device
    idx = torch.as_tensor(idx).long()
    cv, cs = clips[idx, 0].contiguous().to(dev), clips[idx, 1].contiguous().to(dev)
    return cv, cs, train.clip_frames(frames, cv, cs, 1, 0, n_frames, 0.5, 0.5)


def params_of(m):
    return {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}


# ---- 1. the generator ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 255, 257, 2688])
def test_normal_noise_against_the_twin(dev, n):
    """sf_normal_noise_f32 against train.normal_noise (float64 Box-Muller on the same uniforms): max |difference| <= 1e-5.  The bound: at most two
    roundings of the cosine's argument (2^-24 * 2 pi = 3.7e-7 each) times the amplitude 5.77 = 4.3e-6, plus four results (logf, sqrtf, cosf, the
    product) within 2 ulp at 5.77, about 2e-6.  Measured on the MI355X: 7.2e-7 at most over these sizes (profiles/base_fit.md)."""
    from slotformer_amd import ops, train
    worst = 0.
    for seed, tag in ((1, 0), (0x0badc0de12345678, 1), (2**62 - 5, 5)):
        got = ops.normal_noise(seed, tag, n, dev)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, )
        worst = max(worst, float((got.cpu().double() - train.normal_noise(seed, tag, n).double()).abs().max()))
        assert torch.equal(got, ops.normal_noise(seed, tag, n, dev))
        assert torch.equal(got.reshape(-1)[:1], ops.normal_noise(seed, tag, (1, 1), dev).reshape(-1))   # element i does not depend on the shape
    print(f'normal_noise n={n}: max |gpu - twin| = {worst:.3e}')
    assert worst <= 1e-5


# ---- 2. the node --------------------------------------------------------------------------------------------------------------------------------
PRIOR = math.log(0.01)
SAMPLE_SEED, SAMPLE_TAG = 0x1234567890abcdef, 3


def _sample_case(R, D, mode, dev):
    from slotformer_amd import ops
    g = torch.Generator().manual_seed(R * 1000 + D)
    dist = torch.randn(R, 2 * D, generator=g)
    dist[:, D:] = 0.7 * dist[:, D:] - 1.
    gk = torch.randn(R, D, generator=g).to(dev)
    gkld = torch.tensor(0.37, device=dev)
    if mode == 'seed':
        eps, kw = ops.normal_noise(SAMPLE_SEED, SAMPLE_TAG, (R, D), dev), dict(seed=SAMPLE_SEED, tag=SAMPLE_TAG)
    else:
        eps = torch.randn(R, D, generator=g).to(dev)
        kw = dict(noise=eps)
    return dist, gk, gkld, eps, kw


def _sample_run(dist, D, gk, gkld, kw, dev):
    from slotformer_amd import train
    d = dist.to(dev).requires_grad_(True)
    k, kld = train.kernel_sample(d, D, PRIOR, **kw)
    ((k * gk).sum() + gkld * kld).backward()
    return k.detach(), kld.detach(), d.grad


@pytest.mark.parametrize('mode', ['noise', 'seed'])
@pytest.mark.parametrize('R,D', [(1, 64), (7, 128), (21, 128), (300, 192)])
def test_kernel_sample_against_float64(dev, R, D, mode):
    """train.kernel_sample, forward and backward, against float64 on the float32 inputs (seed mode: on the noise sf_normal_noise_f32 gives for that
    seed).  Elementwise bounds, U = 2^-24 per float32 rounding, expf / expm1f within 1 ulp = 2 U, sigma = exp(log_var / 2), x = log_var - prior:
      kernels    U * (3 |eps sigma| + |kernels|)        expf 2, the product 1 (on |eps sigma|), the sum 1
      d_mu       exact (a copy of d_kernels)
      d_log_var  = a + b, a = d_kernels eps sigma / 2, b = g expm1(x), g = d_kld / (2 R):
                 U * (4 |a| + 5 |b| + |g| e^x |x| + |a + b|)   a: d_kernels eps 1, expf 2, the product 1; b: 1 / R and g 1 each, expm1f 2, the
                 product 1, and x's own rounding U |x| carried through e^x; the sum 1
      kld        1e-6 relative (float32 terms, float64 sums, one float32 rounding of the mean).
    Measured on the MI355X: kernels 0.94, d_log_var 0.63 of the bound at most, kld 3.4e-8.  (300, 192) spans 57 workgroups: the last arriver's tree."""
    from slotformer_amd import ops
    dist, gk, gkld, eps, kw = _sample_case(R, D, mode, dev)
    k, kld, dd = _sample_run(dist, D, gk, gkld, kw, dev)
    assert tuple(k.shape) == (R, D) and kld.dim() == 0 and kld.dtype == torch.float32 and tuple(dd.shape) == (R, 2 * D)
    prior = float(np.float32(PRIOR))
    mu, lv, e, g64 = dist[:, :D].double(), dist[:, D:].double(), eps.cpu().double(), gk.cpu().double()
    sigma, x = torch.exp(0.5 * lv), lv - prior
    k_ref = mu + e * sigma
    kld_ref = float((0.5 * (prior - lv) + torch.exp(lv) / (2. * math.exp(prior)) - 0.5).sum() / R)
    a, gc = g64 * e * 0.5 * sigma, float(gkld) / R * 0.5
    b = gc * torch.expm1(x)
    r_k = float(((k.cpu().double() - k_ref).abs() / (U * (3 * (e * sigma).abs() + k_ref.abs()))).max())
    r_d = float(((dd[:, D:].cpu().double() - (a + b)).abs() / (U * (4 * a.abs() + 5 * b.abs() + abs(gc) * torch.exp(x) * x.abs() + (a + b).abs()))).max())
    r_kld = abs(float(kld) - kld_ref) / abs(kld_ref)
    print(f'kernel_sample R={R} D={D} {mode}: kernels {r_k:.2f} of the bound, d_log_var {r_d:.2f} of the bound, kld rel {r_kld:.1e}')
    assert r_k <= 1. and r_d <= 1.
    assert torch.equal(dd[:, :D], gk)
    assert r_kld <= 1e-6
    # the same call twice: the same bits
    k2, kld2, dd2 = _sample_run(dist, D, gk, gkld, kw, dev)
    assert torch.equal(k, k2) and torch.equal(kld, kld2) and torch.equal(dd, dd2)
    if mode == 'seed':   # the seed stands for exactly the tensor sf_normal_noise_f32 writes
        k3, kld3, dd3 = _sample_run(dist, D, gk, gkld, dict(noise=eps), dev)
        assert torch.equal(k, k3) and torch.equal(kld, kld3) and torch.equal(dd, dd3)
    # the KL sum is added to, not overwritten; a missing d_kernels is zero
    d = dist.to(dev)
    s0, s5 = torch.zeros(1, dtype=torch.float64, device=dev), torch.full((1, ), 5., dtype=torch.float64, device=dev)
    ops.kernel_sample_fwd(d, D, PRIOR, s0, **kw)
    ops.kernel_sample_fwd(d, D, PRIOR, s5, **kw)
    assert torch.equal(s5, s0 + 5.) and float(s0) != 0.
    only_kld = ops.kernel_sample_bwd(d, D, PRIOR, None, gkld.reshape(1), 1. / R, **kw)
    assert not only_kld[:, :D].any() and rel_l2(only_kld[:, D:].cpu(), b) < 1e-6


# ---- 3. StoSAVi: the step of fit against the module's ------------------------------------------------------------------------------------------
def test_savi_step_gradients_fit_path_against_module_path(dev, frames):
    """One StoSAVi training step from `noise_seed` (train.kernel_sample per frame, what fit runs) against the module path on the same noise as a
    tensor (`data['noise']`, torch's sampling glue and host.losses.kernel_kld): both loss terms and every parameter's gradient, by relative L2.
    The two differ only in where the KL term and the gradient of the sample round: kernel_sample.hip rounds the sample itself as torch's unfused
    glue does (it is built with -ffp-contract=off), so both paths see the same slots.  With a fused multiply-add in the sample the slots differed by
    3e-6 and the decoder's gradients, through its ReLU kinks, by 1.1e-3.  Measured on the MI355X: the terms agree to 1.5e-7, the worst gradient to
    5.5e-6 (SAVI_GRAD_WORST); the bound is ten times that, and no more than the 1e-4 the golden step test holds this step to."""
    from slotformer_amd import base_slots as bs, video_prediction as vp
    clips = bs.clip_index(bc.V, bc.T, bc.N_FRAMES, 1, 'train')
    _, _, img = gather(frames, clips, [3, 12])
    sd = vp._step_seed(bc.SEED, 0)
    w = bs.LOSS_W['savi']
    ma, mb = bc.savi().to(dev).train(), bc.savi().to(dev).train()
    ta = [t for t, _ in bs._train_terms('savi', ma, img, None, sd, None)]
    (w[0] * ta[0] + w[1] * ta[1]).backward()
    data = {'img': img, 'noise': mb.seeded_noise(sd, img.shape[0], img.shape[1], dev)}
    out = mb(data)
    assert 'kld' not in out
    tb = mb.calc_train_loss(data, out)
    (w[0] * tb['post_recon_loss'] + w[1] * tb['kld_loss']).backward()
    fa, fb = [float(t.detach()) for t in ta], [float(tb[k].detach()) for k in ('post_recon_loss', 'kld_loss')]
    e_terms = max(abs(a - b) / b for a, b in zip(fa, fb))
    ga, gb = dict(ma.named_parameters()), dict(mb.named_parameters())
    worst, name = 0., None
    for n, p in gb.items():
        assert (p.grad is None) == (ga[n].grad is None), n
        if p.grad is None:
            continue
        if n == 'slot_attention.project_q.0.bias':   # (zero in exact arithmetic: a bias in front of a softmax over the slots it is shared by)
            assert float(ga[n].grad.abs().max()) < 1e-5 and float(p.grad.abs().max()) < 1e-5
            continue
        e = rel_l2(ga[n].grad, p.grad)
        if e > worst:
            worst, name = e, n
    print(f'savi step: loss terms rel {e_terms:.2e}, worst gradient rel-L2 {worst:.2e} ({name})')
    assert e_terms <= 1e-6
    assert worst <= SAVI_GRAD_BOUND


SAVI_GRAD_WORST = 5.5e-6   # measured (see the docstring above and profiles/base_fit.md)
SAVI_GRAD_BOUND = min(10 * SAVI_GRAD_WORST, 1e-4)


# ---- 4. dVAE: fit is the hand-written loop ----------------------------------------------------------------------------------------------------------
def test_dvae_fit_equals_the_hand_written_loop(dev, frames):
    """Three steps of fit on a dVAE against the loop INTEGRATION.md used to spell out -- the module's forward and loss, FlatAdam, the same rates,
    temperatures and Gumbel seeds: every parameter bit for bit (the fused image loss gives the gradient torch's mean of squares gives)."""
    from slotformer_amd import base_slots as bs, train, video_prediction as vp
    clips = bs.clip_index(bc.V, bc.T, bc.N_FRAMES, 1, 'train')[:6]
    lr, total = 1e-3, 3
    ma, mb = bc.dvae().to(dev).eval(), bc.dvae().to(dev).train()
    res = bs.fit(ma, frames, clips, 1, bc.BATCH, lr, bc.SEED, bc.N_FRAMES)
    assert res['state']['step'] == total and tuple(res['recon_loss'].shape) == (1, )
    opt = train.FlatAdam([p for p in mb.parameters() if p.requires_grad], lr=lr)
    losses = []
    for s, idx in enumerate(bs.clip_schedule(clips.shape[0], 1, bc.BATCH, bc.SEED)[0]):
        _, _, img = gather(frames, clips, idx)
        data = {'img': img, 'gumbel_tau': bs.cosine_anneal(s, 1., 0.1, 0.15 * total), 'gumbel_seed': vp._step_seed(bc.SEED, s)}
        opt.lr = train.warmup_cosine_lr(s, total, 0.05 * total, lr, lr * 0.01)
        opt.zero_grad()
        loss = mb.calc_train_loss(data, mb(data))['recon_loss']
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    pa, pb = params_of(ma), params_of(mb)
    bad = [n for n in pb if not torch.equal(pa[n], pb[n])]
    print(f'dvae: fit recon_loss {float(res["recon_loss"][0]):.6f}, loop {sum(losses) / total:.6f}; parameters that differ: {bad}')
    assert not bad
    assert float(res['recon_loss'][0]) == pytest.approx(sum(losses) / total, rel=1e-6)
    assert not ma.training   # fit leaves the mode it found


# ---- 5. STEVE ------------------------------------------------------------------------------------------------------------------------------------
def _steve_tokens(model, frames):
    from slotformer_amd import train
    dev = frames.device
    every = torch.arange(bc.V, dtype=torch.int32, device=dev)
    x = train.clip_frames(frames, every, torch.zeros_like(every), 1, 0, bc.T, 0.5, 0.5)
    return model.dvae.tokenize_ids(x, dtype=torch.int16).flatten(2, 3).contiguous()


def _steve_hand_loop(model, frames, clips, tokens, steps, lr, dec_lr):
    from slotformer_amd import base_slots as bs, train, video_prediction as vp
    opt = train.FlatAdam(train.steve_param_groups(model, lr, dec_lr))
    sched = bs.clip_schedule(clips.shape[0], 1, bc.BATCH, bc.SEED)[0]
    assert len(sched) == steps
    for s, idx in enumerate(sched):
        cv, cs, img = gather(frames, clips, idx)
        t = cs.long()[:, None] + torch.arange(bc.N_FRAMES, device=cs.device)
        data = {'img': img, 'token_id': tokens[cv.long()[:, None], t]}
        for g, peak in zip(opt.param_groups, (lr, dec_lr)):
            g['lr'] = train.warmup_cosine_lr(s, steps, 0.05 * steps, peak)
        opt.zero_grad()
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(vp._step_seed(bc.SEED, s))
            model.calc_train_loss(data, model(data))['token_recon_loss'].backward()
        opt.step()
    return params_of(model)


@pytest.mark.parametrize('case', ['table', 'on_the_fly', 'table_fused'])
def test_steve_fit_against_the_hand_written_loop(dev, frames, case, monkeypatch):
    """Two steps of fit on STEVE against the hand-written loop (module forward, calc_train_loss, FlatAdam with the two groups, the dropout seeds of
    the step), with the targets from a token table, tokenised on the fly, and with `fused_token_loss`.  The decoder attention's backward adds dq
    with float atomics, so the comparison is by relative L2 against ten times the spread between two runs of the hand-written loop itself.
    Measured on the MI355X over six pairs of runs: the loop against itself 0 to 4.7e-10 (STEVE_SPREAD: the largest), fit against the loop 5.8e-11 to
    9.3e-10.  The run's own spread is printed beside them.  fit runs no inference encode: engine.savi_encode is not called, the module step calls it."""
    from slotformer_amd import base_slots as bs, engine
    fused = case == 'table_fused'
    clips = bs.clip_index(bc.V, bc.T, bc.N_FRAMES, 1, 'train')[:4]
    lr, dec_lr, steps = 1e-4, 3e-4, 2
    models = [bc.steve(fused=fused).to(dev).train() for _ in range(3)]
    tokens = _steve_tokens(models[0], frames)
    cv, cs, img = gather(frames, clips, [0, 3])
    t = cs.long()[:, None] + torch.arange(bc.N_FRAMES, device=dev)
    assert torch.equal(models[0].dvae.tokenize_ids(img, dtype=torch.int16).flatten(2, 3), tokens[cv.long()[:, None], t])
    calls = []
    real = engine.savi_encode
    monkeypatch.setattr(engine, 'savi_encode', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    h1 = _steve_hand_loop(models[1], frames, clips, tokens, steps, lr, dec_lr)
    n_module = len(calls)
    h2 = _steve_hand_loop(models[2], frames, clips, tokens, steps, lr, dec_lr)
    del calls[:]
    res = bs.fit(models[0], frames, clips, 1, bc.BATCH, lr, bc.SEED, bc.N_FRAMES, dec_lr=dec_lr, tokens=None if case == 'on_the_fly' else tokens)
    n_fit = len(calls)
    pf = params_of(models[0])
    spread = max(rel_l2(h2[n], h1[n]) for n in h1)
    err = max(rel_l2(pf[n], h1[n]) for n in h1)
    print(f'steve {case}: hand-written loop run to run {spread:.2e}, fit against it {err:.2e}; savi_encode calls: module {n_module}, fit {n_fit}')
    assert n_fit == 0 and n_module >= 1
    assert res['img_recon_loss'] is None and tuple(res['token_recon_loss'].shape) == (1, ) and math.isfinite(float(res['token_recon_loss'][0])) and float(res['token_recon_loss'][0]) > 0.
    assert err <= 10 * STEVE_SPREAD


STEVE_SPREAD = 4.7e-10   # measured (see the docstring above and profiles/base_fit.md)


# ---- 6. one seed, one result ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['savi', 'dvae'])
def test_fit_is_deterministic_and_resumes(dev, frames, kind):
    from slotformer_amd import base_slots as bs
    build = bc.savi if kind == 'savi' else bc.dvae
    term = 'post_recon_loss' if kind == 'savi' else 'recon_loss'
    clips = bs.clip_index(bc.V, bc.T, bc.N_FRAMES, 1, 'train')[::5]   # 4 clips: 2 steps an epoch
    args = (frames, clips, 2, bc.BATCH, 1e-3, bc.SEED, bc.N_FRAMES)
    ma, mb, mc = (build().to(dev) for _ in range(3))
    torch.manual_seed(77)
    before = torch.random.get_rng_state()
    ra = bs.fit(ma, *args, clip_grad=0.05)
    assert torch.equal(torch.random.get_rng_state(), before)
    rb = bs.fit(mb, *args, clip_grad=0.05)
    pa, pb = params_of(ma), params_of(mb)
    assert all(torch.equal(pa[n], pb[n]) for n in pa)
    assert torch.equal(ra[term], rb[term]) and tuple(ra[term].shape) == (2, ) and ra['state']['step'] == 4
    if kind == 'savi':
        assert torch.equal(ra['kld_loss'], rb['kld_loss']) and float(ra['kld_loss'][0]) > 0.
    half = bs.fit(mc, *args, clip_grad=0.05, stop_after=1)
    assert half['state']['step'] == 2 and torch.equal(half[term], ra[term][:1])
    rest = bs.fit(mc, *args, clip_grad=0.05, resume=half['state'])
    pc = params_of(mc)
    assert all(torch.equal(pa[n], pc[n]) for n in pa)
    assert torch.equal(rest[term], ra[term][1:]) and rest['state']['step'] == 4
    assert torch.equal(torch.random.get_rng_state(), before)
    other = bs.fit(build().to(dev), frames, clips, 2, bc.BATCH, 1e-3, bc.SEED + 1, bc.N_FRAMES, clip_grad=0.05)
    assert not torch.equal(other[term], ra[term])


def test_plain_savi_has_no_kld_term(dev, frames):
    """kld_method 'none' skips the node: no 'kld' in the step, None for the term, and the noise seed changes nothing."""
    from slotformer_amd import base_slots as bs
    clips = bs.clip_index(bc.V, bc.T, bc.N_FRAMES, 1, 'train')[:2]
    m = bc.savi(kld='none').to(dev)
    res = bs.fit(m, frames, clips, 1, bc.BATCH, 1e-4, bc.SEED, bc.N_FRAMES)
    assert res['kld_loss'] is None and float(res['post_recon_loss'][0]) > 0.


# ---- 7. it learns -------------------------------------------------------------------------------------------------------------------------------------
def test_dvae_learns_smooth_frames(dev, frames):
    """The dVAE on the 24 single frames of 4 smooth videos, 3 epochs of 12 steps at lr 1e-3: the last epoch's recon_loss is below 0.9 of the first's."""
    from slotformer_amd import base_slots as bs
    clips = bs.clip_index(bc.V, bc.T, 1, 1, 'train')
    assert clips.shape[0] == bc.V * bc.T
    res = bs.fit(bc.dvae().to(dev), frames, clips, 3, bc.BATCH, 1e-3, bc.SEED, 1)
    loss = [float(v) for v in res['recon_loss']]
    print(f'dvae recon_loss per epoch: {loss}')
    assert loss[-1] < 0.9 * loss[0]


# ---- 8. evaluate ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['savi', 'dvae', 'steve'])
def test_evaluate_equals_the_module_terms(dev, frames, kind):
    """evaluate over 5 clips in batches of 2 (the last one ragged) against the batch-size-weighted mean of the module's eval-mode loss terms on the
    same noise, to 1e-6 relative.  STEVE's token loss comes from the fused head there and from the logits here."""
    from slotformer_amd import base_slots as bs, video_prediction as vp
    model = {'savi': bc.savi, 'dvae': bc.dvae, 'steve': bc.steve}[kind]().to(dev).train()
    clips = bs.clip_index(bc.V, bc.T, bc.N_FRAMES, 1, 'val')[:5]
    tokens = _steve_tokens(model, frames) if kind == 'steve' else None
    got = bs.evaluate(model, frames, clips, bc.BATCH, bc.N_FRAMES, seed=bc.SEED, tokens=tokens)
    assert model.training
    model.eval()
    want = {}
    with torch.no_grad():
        for i, s in enumerate(range(0, 5, bc.BATCH)):
            cv, cs, img = gather(frames, clips, list(range(s, min(s + bc.BATCH, 5))))
            b, sd = img.shape[0], vp._step_seed(bc.SEED, i)
            data = {'img': img}
            if kind == 'savi':
                data['noise'] = model.seeded_noise(sd, b, bc.N_FRAMES, dev)
            elif kind == 'dvae':
                data['gumbel_seed'] = sd
            else:
                t = cs.long()[:, None] + torch.arange(bc.N_FRAMES, device=dev)
                data['token_id'] = tokens[cv.long()[:, None], t]
            for k, v in model.calc_train_loss(data, model(data)).items():
                want[k] = want.get(k, 0.) + float(v.double()) * b / 5
    print(f'evaluate {kind}: {got} against {want}')
    assert sorted(got) == sorted(want) and all(isinstance(v, float) for v in got.values())
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-6), k


# ---- the seeds of the two Gumbel draws ---------------------------------------------------------------------------------------------------------------
def test_gumbel_seed_fixes_the_draw(dev, frames):
    """`gumbel_seed` in dVAE.forward and on STEVE's use_img_recon_loss branch: the same seed gives the same bits, another seed another sample, and
    for the dVAE it is the noise train.gumbel_noise restates."""
    from slotformer_amd import base_slots as bs, train
    clips = bs.clip_index(bc.V, bc.T, bc.N_FRAMES, 1, 'train')
    _, _, img = gather(frames, clips, [1, 8])
    dv = bc.dvae().to(dev).eval()
    st = bc.steve(img_loss=True).to(dev).eval()
    with torch.no_grad():
        a = dv({'img': img, 'gumbel_seed': 5})['recon']
        assert torch.equal(a, dv({'img': img, 'gumbel_seed': 5})['recon'])
        assert not torch.equal(a, dv({'img': img, 'gumbel_seed': 6})['recon'])
        g = train.gumbel_noise(5, img.shape[0] * img.shape[1] * 16 * 16 * 64).reshape(img.shape[0], img.shape[1], 16, 16, 64).permute(0, 1, 4, 2, 3)
        assert rel_l2(dv({'img': img, 'gumbel': g.to(dev)})['recon'], a) < 1e-5
        b = st({'img': img, 'gumbel_seed': 5})['recon_img']
        assert torch.equal(b, st({'img': img, 'gumbel_seed': 5})['recon_img'])
        assert not torch.equal(b, st({'img': img, 'gumbel_seed': 6})['recon_img'])
