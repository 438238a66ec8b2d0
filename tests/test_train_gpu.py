"""GPU parity of the rollout TRAINING path: loss and gradients through the reference-shaped
nn.Module API (`forward` -> `calc_train_loss` -> `loss.backward()`) against a golden fixture produced by the reference's
own SlotFormer under torch autograd, and against autograd of the oracle at full width (d_model 256, 4 layers)."""
import numpy as np
import pytest
import torch

import golden_util as gu
import oracle
from test_engine_gpu import build, rel_err

pytestmark = pytest.mark.gpu

GTOL = 2e-4   # gradients: fp32 with split-bf16 contractions; relative to the largest entry of each tensor
# At full width a handful of the ~10^7 FFN pre-activations sit within rounding distance of the ReLU kink and take the
# other branch than on the CPU (more of them under split-bf16 than under exact f32): a few rows of linear1's gradient move
# by one sample's contribution.  So there each tensor is compared in relative L2 norm, not entry by entry.
L2TOL = {'bf16x3': 2e-3, 'f32': 4e-4}


def l2_err(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm()).item()


def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.


def _oracle_grads(slots, sd, cfg, S, decay, names, drop=None):
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    x = slots.clone().requires_grad_(True)
    hist = cfg['rollout_dict']['history_len']
    if drop is None:
        pred = oracle.rollouter_forward(x[:, :hist], S, osd, cfg['rollout_dict'])
    else:
        pred = oracle.rollouter_forward_train(x[:, :hist], S, osd, cfg['rollout_dict'], drop)
    loss = oracle.slot_mse_losses(pred, x[:, hist:], training=True, loss_decay_factor=decay)['slot_recon_loss']
    loss.backward()
    return float(loss.detach()), pred.detach(), {n: osd[n].grad for n in names}, x.grad


def _engine_grads(m, slots, decay, dev):
    m.loss_decay_factor = decay
    x = slots.to(dev).requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    out = m({'slots': x})
    loss = m.calc_train_loss({'slots': x}, out)['slot_recon_loss']
    loss.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if n.startswith('rollouter.') and p.requires_grad}
    return float(loss.detach()), out['pred_slots'].detach(), grads, x.grad


def test_rollout_grads_golden(dev, precision):
    g = gu.load_golden('roll_train')
    cfg = gu.TRAIN_ROLL
    m, sd = build(cfg, g, 801, dev, vp=True)
    m.train()
    _no_dropout(m)
    rd = cfg['rollout_dict']
    slots = gu.seeded_normal((2, rd['history_len'] + 3, rd['num_slots'], rd['slot_size']), 802)
    loss, pred, grads, d_slots = _engine_grads(m, slots, 0.9, dev)
    assert abs(loss - float(g['loss'])) < 1e-5 * abs(float(g['loss']))
    assert rel_err(pred, g['pred_slots']) < 1e-4
    names = [str(n) for n in g['grad_names']]
    assert sorted(names) == sorted(grads)
    for n in names:
        assert grads[n] is not None, n
        assert rel_err(grads[n], g['grad.' + n]) < GTOL, n
    assert rel_err(d_slots, g['d_slots']) < GTOL
    # the frozen decoder and the position table get no gradient
    assert all(p.grad is None for n, p in m.named_parameters() if not n.startswith('rollouter.') or not p.requires_grad)


def test_rollout_grads_with_learnable_position_tables(dev, precision):
    """t_pe = slots_pe = 'learnable' (build_pos_enc, slotformer.py:19-29): the tables are parameters, the kernels read them folded into
    one token table and the backward pass returns that table's gradient, summed here over slots / frames.  Fixture: the reference's own
    training step with a non-zero temporal table."""
    g = gu.load_golden('roll_train_pe')
    cfg = gu.TRAIN_ROLL_PE
    m, sd = build(cfg, g, 821, dev, vp=True)
    with torch.no_grad():
        m.rollouter.enc_t_pe.copy_(torch.from_numpy(g['closed::rollouter.enc_t_pe']).to(dev))
    assert m.rollouter.enc_t_pe.requires_grad and m.rollouter.enc_slots_pe.requires_grad
    m.train()
    _no_dropout(m)
    rd = cfg['rollout_dict']
    slots = gu.seeded_normal((2, rd['history_len'] + 3, rd['num_slots'], rd['slot_size']), 822)
    loss, pred, grads, d_slots = _engine_grads(m, slots, 0.9, dev)
    assert abs(loss - float(g['loss'])) < 1e-5 * abs(float(g['loss']))
    assert rel_err(pred, g['pred_slots']) < 1e-4
    names = [str(n) for n in g['grad_names']]
    assert sorted(names) == sorted(grads) and 'rollouter.enc_t_pe' in names and 'rollouter.enc_slots_pe' in names
    for n in names:
        assert grads[n] is not None, n
        assert rel_err(grads[n], g['grad.' + n]) < GTOL, n
    assert rel_err(d_slots, g['d_slots']) < GTOL
    # an optimizer step moves the tables, and the next forward sees the moved tables (the plan is re-folded)
    opt = torch.optim.SGD(m.rollouter.parameters(), lr=0.5)
    before = m.rollouter.enc_t_pe.detach().clone()
    opt.step()
    assert not torch.equal(before, m.rollouter.enc_t_pe.detach())
    loss2 = _engine_grads(m, slots, 0.9, dev)[0]
    assert loss2 != loss
    # inference kernels read the same (re-folded) tables
    m.eval()
    with torch.no_grad():
        out = m({'slots': slots.to(dev)})['pred_slots']
    sd2 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = oracle.slotformer_forward(slots, sd2, cfg, 3)['pred_slots']
    assert rel_err(out, ref) < 1e-4


@pytest.mark.parametrize('B,S', [(3, 4), (1, 2)])
def test_rollout_grads_c2_vs_oracle(dev, precision, B, S):
    """CLEVRER width (slotformer_clevrer_params.py: d_model 256, 4 layers, 8 heads, ffn 1024, 6 x 7 tokens)."""
    cfg = {**gu.C2_ROLL, 'loss_dict': dict(rollout_len=S, use_img_recon_loss=False)}
    m, sd = build(cfg, gu.load_golden('roll_c2'), 202, dev, vp=True)
    m.train()
    _no_dropout(m)
    slots = gu.seeded_normal((B, 6 + S, 7, 128), 900 + B)
    loss, pred, grads, d_slots = _engine_grads(m, slots, 1.0, dev)
    oloss, opred, ograds, od = _oracle_grads(slots, sd, cfg, S, 1.0, set(grads))
    assert abs(loss - oloss) < 1e-5 * abs(oloss)
    assert rel_err(pred, opred) < 1e-4
    for n in grads:
        assert l2_err(grads[n], ograds[n]) < L2TOL[precision], n
    assert l2_err(d_slots, od) < L2TOL[precision]


def _double(t):
    return t.double() if t.dtype.is_floating_point else t


@pytest.mark.parametrize('name,cfg_name,seed,B,S', [
    # the reference's Physion window (slotformer_physion_params.py: 15 burn-in frames x 6 slots = 90 tokens, 8 layers): MFMA
    # attention on 96-token tiles, past 64 KB of LDS
    ('roll_c4_ref', 'C4_ROLL_REF', 214, 2, 2),
    # OBJ3D (d_model 128, 8 heads of 16): the scalar attention kernels
    ('roll_c1', 'C1_ROLL', 201, 3, 3),
    # CLEVRER at tools/bench_train.py's training batch, oracle in float64
    ('roll_c2', 'C2_ROLL', 202, 32, 10),
])
def test_rollout_grads_reference_shapes_vs_oracle(dev, precision, name, cfg_name, seed, B, S):
    cfg = {**getattr(gu, cfg_name), 'loss_dict': dict(rollout_len=S, use_img_recon_loss=False)}
    m, sd = build(cfg, gu.load_golden(name), seed, dev, vp=True)
    m.train()
    _no_dropout(m)
    rd = cfg['rollout_dict']
    slots = gu.seeded_normal((B, rd['history_len'] + S, rd['num_slots'], rd['slot_size']), 910 + B)
    loss, pred, grads, d_slots = _engine_grads(m, slots, 1.0, dev)
    oloss, opred, ograds, od = _oracle_grads(slots.double(), {k: _double(v) for k, v in sd.items()}, cfg, S, 1.0, set(grads))
    worst = max((l2_err(grads[n], ograds[n]), n) for n in grads)
    print(name, precision, f'loss {abs(loss - oloss) / abs(oloss):.2e} pred {rel_err(pred, opred):.2e} worst grad {worst[0]:.2e} ({worst[1]})',
          f'd_slots {l2_err(d_slots, od):.2e} (bound {L2TOL[precision]:.0e})')
    assert abs(loss - oloss) < 1e-5 * abs(oloss)
    assert rel_err(pred, opred) < 1e-4
    for n in grads:
        assert l2_err(grads[n], ograds[n]) < L2TOL[precision], n
    assert l2_err(d_slots, od) < L2TOL[precision]


def test_rollout_dropout_masks_vs_oracle(dev):
    """Train mode with the layer's default dropout (p = 0.1): the library's masks are a pure function of
    (seed, step, layer, site, element), rebuilt here on the host and fed to the oracle."""
    from slotformer_amd.train import dropout_keep_mask
    S, B, p, seed = 3, 2, 0.1, 0x1234567_89abcdef
    cfg = {**gu.C2_ROLL, 'loss_dict': dict(rollout_len=S, use_img_recon_loss=False)}
    m, sd = build(cfg, gu.load_golden('roll_c2'), 202, dev, vp=True)
    m.train()
    m.rollouter.dropout_seed_override = seed
    slots = gu.seeded_normal((B, 6 + S, 7, 128), 950)
    loss, pred, grads, d_slots = _engine_grads(m, slots, 1.0, dev)

    def drop(step, layer, site, t):
        keep = dropout_keep_mask(seed, step, layer, site, t.numel(), p)
        return t * torch.from_numpy(keep.astype(np.float32)).view(t.shape) / (1.0 - float(np.float32(p)))

    oloss, opred, ograds, od = _oracle_grads(slots, sd, cfg, S, 1.0, set(grads), drop)
    # without the masks the result is far away: the comparison is meaningful
    assert rel_err(pred, oracle.rollouter_forward(slots[:, :6], S, sd, cfg['rollout_dict'])) > 1e-2
    assert rel_err(pred, opred) < 1e-4
    assert abs(loss - oloss) < 1e-5 * abs(oloss)
    for n in grads:
        assert l2_err(grads[n], ograds[n]) < L2TOL['bf16x3'], n
    assert l2_err(d_slots, od) < L2TOL['bf16x3']
    # keep rate of one site
    keep = dropout_keep_mask(seed, 0, 0, 2, 1 << 20, p)
    assert abs(keep.mean() - 0.9) < 2e-3
    # a different seed gives a different result; eval mode ignores dropout altogether
    m.rollouter.dropout_seed_override = seed + 1
    assert rel_err(_engine_grads(m, slots, 1.0, dev)[1], opred) > 1e-3
    m.eval()
    ev = _engine_grads(m, slots, 1.0, dev)[1]
    assert rel_err(ev, oracle.rollouter_forward(slots[:, :6], S, sd, cfg['rollout_dict'])) < 1e-4


def test_training_step_reduces_loss(dev):
    """A few Adam steps on one batch (the reference's optimiser, slotformer_clevrer_params.py:16-19) drive the loss down,
    and the inference engine sees the updated weights (its packed copies are rebuilt per weight version)."""
    S = 4
    cfg = {**gu.C2_ROLL, 'loss_dict': dict(rollout_len=S, use_img_recon_loss=False)}
    m, sd = build(cfg, gu.load_golden('roll_c2'), 202, dev, vp=True)
    m.train()
    slots = (0.5 * gu.seeded_normal((4, 6 + S, 7, 128), 960)).to(dev)
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=2e-4)
    hist = []
    for _ in range(8):
        opt.zero_grad(set_to_none=True)
        out = m({'slots': slots})
        loss = m.calc_train_loss({'slots': slots}, out)['slot_recon_loss']
        loss.backward()
        opt.step()
        hist.append(float(loss))
    assert hist[-1] < 0.8 * hist[0], hist
    m.eval()
    with torch.no_grad():
        pred = m({'slots': slots})['pred_slots']
    new_sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = oracle.rollouter_forward(slots[:, :6].cpu(), S, new_sd, cfg['rollout_dict'])
    assert rel_err(pred, ref) < 1e-3


@pytest.mark.parametrize('B,HW,N,D', [(3, 4096, 7, 128), (2, 4096, 6, 128), (2, 1024, 4, 64), (1, 4096, 8, 128), (2, 4096, 6, 192), (1, 1024, 5, 256)])
def test_slot_attention_iteration_backward(dev, B, HW, N, D):
    """sf_slot_attn_iter_bwd_f32 against autograd of the oracle's attention half (savi.py:82-94)."""
    from slotformer_amd import ops
    k = gu.seeded_normal((B, HW, D), 11)
    v = gu.seeded_normal((B, HW, D), 12)
    q = 2.0 * gu.seeded_normal((B, N, D), 13)
    du = gu.seeded_normal((B, N, D), 14)
    kk, vv, qq = (t.clone().requires_grad_(True) for t in (k, v, q))
    upd = oracle.slot_attention_updates(kk, vv, qq)
    upd.backward(du)
    pn, pd, _ = ops.slot_attn_iter(k.to(dev), v.to(dev), q.to(dev))
    assert rel_err(pn.sum(1) / pd.sum(1).unsqueeze(-1), upd) < 1e-4
    dq, dk, dv = ops.slot_attn_iter_bwd(k.to(dev), v.to(dev), q.to(dev), pn, pd, du.to(dev))
    assert rel_err(dq, qq.grad) < 1e-4
    assert rel_err(dk, kk.grad) < 1e-4
    assert rel_err(dv, vv.grad) < 1e-4
    # second iteration of the same frame: gradients accumulate into dk / dv
    dq2, dk2, dv2 = ops.slot_attn_iter_bwd(k.to(dev), v.to(dev), q.to(dev), pn, pd, du.to(dev), dk=dk.clone(), dv=dv.clone())
    assert rel_err(dk2, 2 * kk.grad) < 1e-4 and rel_err(dv2, 2 * vv.grad) < 1e-4 and rel_err(dq2, qq.grad) < 1e-4


@pytest.mark.parametrize('B,HW,N,D,Cin,H,iters', [(3, 4096, 7, 128, 128, 256, 2), (2, 1024, 4, 64, 64, 128, 3), (2, 4096, 6, 192, 192, 384, 2)])
def test_slot_attention_module_backward(dev, precision, B, HW, N, D, Cin, H, iters):
    """SlotAttention.forward under autograd (savi.py:56-102: LN + k/v projection, `iters` x [q projection, attention,
    GRUCell, residual MLP]) against autograd of the oracle: output, gradients of all 17 parameter leaves, of the input
    features and of the initial slots."""
    from slotformer_amd.base_slots.models.savi import SlotAttention
    torch.manual_seed(5)
    sa = SlotAttention(Cin, iters, N, D, H).to(dev)
    with torch.no_grad():
        for p in sa.parameters():   # well away from the default LayerNorm (1, 0) so that every gradient path is exercised
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    x = gu.seeded_normal((B, HW, Cin), 21)
    s0 = gu.seeded_normal((B, N, D), 22)
    dout = gu.seeded_normal((B, N, D), 23)
    sd = {'slot_attention.' + k: v.detach().cpu().clone().requires_grad_(True) for k, v in sa.state_dict().items()}
    xo, so = x.clone().requires_grad_(True), s0.clone().requires_grad_(True)
    ref = oracle.slot_attention(xo, so, sd, iters)
    ref.backward(dout)
    xg, sg = x.to(dev).requires_grad_(True), s0.to(dev).requires_grad_(True)
    out = sa(xg, sg)
    out.backward(dout.to(dev))
    assert rel_err(out, ref) < 1e-4
    tol = L2TOL[precision]
    for name, p in sa.named_parameters():
        assert p.grad is not None, name
        ref_g = sd['slot_attention.' + name].grad
        if name == 'project_q.0.bias':
            # a bias on LN_q shifts every slot's logits of a pixel by the same amount: the softmax over slots, hence the
            # loss, does not depend on it -- both gradients are rounding noise around zero
            assert ref_g.abs().max() < 1e-5 and p.grad.abs().max() < 1e-5
            continue
        assert l2_err(p.grad, ref_g) < tol, name
    assert l2_err(sg.grad, so.grad) < tol
    assert l2_err(xg.grad, xo.grad) < tol
    # inference path unchanged and equal to the training forward
    with torch.no_grad():
        assert rel_err(sa(xg.detach(), sg.detach()), ref) < 1e-4


def test_rollout_grads_with_image_loss_golden(dev, precision):
    """The reference's default CLEVRER / OBJ3D training objective (use_img_recon_loss=True, slotformer.py:272-281,313-326):
    slot loss + MSE of the frames decoded from the predicted slots by the frozen SAVi decoder.  Loss and gradients
    against the fixture produced by the reference's own SlotFormer + torch autograd."""
    g = gu.load_golden('roll_train_img')
    cfg = gu.TRAIN_ROLL_IMG
    m, sd = build(cfg, g, 811, dev, vp=True)
    m.train()
    _no_dropout(m)
    rd = cfg['rollout_dict']
    T = rd['history_len'] + 2
    slots = gu.seeded_normal((1, T, rd['num_slots'], rd['slot_size']), 812)
    data = {'slots': slots.to(dev).requires_grad_(True), 'img': gu.seeded_img(1, T, 64, 813).to(dev)}
    m.loss_decay_factor = 0.9
    out = m(data)
    terms = m.calc_train_loss(data, out)
    loss = terms['slot_recon_loss'] + terms['img_recon_loss']
    loss.backward()
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-5 * abs(float(g['loss']))
    grads = {n: p.grad for n, p in m.named_parameters() if n.startswith('rollouter.') and p.requires_grad}
    for n in (str(x) for x in g['grad_names']):
        assert rel_err(grads[n], g['grad.' + n]) < GTOL, n
    assert rel_err(data['slots'].grad, g['d_slots']) < GTOL
    assert all(p.grad is None for n, p in m.named_parameters() if n.startswith('decoder'))


@pytest.mark.parametrize('Fr', [2, 5])
def test_decoder_data_gradient_vs_oracle(dev, precision, Fr):
    """d(recon_combined)/d(slots) of the SAVi decoder at the CLEVRER decoder shape (7 slots, D=128, 8x8 -> 64x64)."""
    cfg = gu.savi_cfg(64, 7, kernel_mlp=False, pred='mlp', rnn=False)
    m, sd = build(cfg, gu.load_golden('decode_c2'), 401, dev)
    for p in list(m.decoder.parameters()) + list(m.decoder_pos_embedding.parameters()):
        p.requires_grad_(False)
    slots = gu.seeded_normal((Fr, 7, 128), 31)
    target = gu.seeded_img(1, Fr, 64, 32)[0]
    so = slots.clone().requires_grad_(True)
    ref = oracle.savi_decode(so, sd, cfg)[0]
    ((ref - target)**2).mean().backward()
    sg = slots.to(dev).requires_grad_(True)
    recon, recons, masks, _ = m.decode(sg)
    assert rel_err(recon, ref) < 1e-4 and not recons.requires_grad and not masks.requires_grad
    ((recon - target.to(dev))**2).mean().backward()
    # ~10^7 ReLU units per frame: the kink-flip noise of L2TOL's comment, larger here
    assert l2_err(sg.grad, so.grad) < {'bf16x3': 1e-2, 'f32': 2e-3}[precision]


@pytest.mark.parametrize('learn_pe', [False, True])
def test_single_step_rollouter_grads_vs_oracle(dev, precision, learn_pe):
    """PHYRE's SingleStepSlotRollouter under autograd (single_step_slotformer.py:49-90): one burn-in frame, the window grows
    to cond_len = 6 frames (8 .. 48 tokens) and then slides; 8 layers.  Gradients against autograd of the oracle.  learn_pe: the
    temporal table is trained too (a growing window reads the table's LAST rows only, :84-85)."""
    S, B = 8, 2
    cfg = {**gu.C5_ROLL, 'loss_dict': dict(rollout_len=S, use_img_recon_loss=False)}
    m, sd = build(cfg, gu.load_golden('roll_c5'), 205, dev, vp=True)
    m.rollouter.enc_t_pe.requires_grad_(learn_pe)
    m.train()
    _no_dropout(m)
    slots = gu.seeded_normal((B, 1 + S, 8, 128), 970)
    m.loss_decay_factor = 1.0
    x = slots.to(dev).requires_grad_(True)
    out = m({'slots': x})
    loss = m.calc_train_loss({'slots': x}, out)['slot_recon_loss']
    loss.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if n.startswith('rollouter.') and p.requires_grad}
    osd = {k: (v.clone().requires_grad_(True) if k in grads else v) for k, v in sd.items()}
    xo = slots.clone().requires_grad_(True)
    pred = oracle.single_step_rollouter_forward(xo[:, :1], S, osd, cfg['rollout_dict'])
    oloss = ((pred - xo[:, 1:])**2).mean()
    oloss.backward()
    assert rel_err(out['pred_slots'], pred) < 1e-4
    assert abs(float(loss.detach()) - float(oloss.detach())) < 1e-5 * abs(float(oloss.detach()))
    # the last layer's FFN only sees gradient on the 8 newest tokens of each window (128 rows in all), so one ReLU-kink
    # flip weighs more there than in the 4-layer sliding-window case: 2.5 x L2TOL
    tol = 2.5 * L2TOL[precision]
    assert ('rollouter.enc_t_pe' in grads) == learn_pe
    for n in grads:
        assert l2_err(grads[n], osd[n].grad) < tol, n
    assert l2_err(x.grad, xo.grad) < tol


@pytest.mark.parametrize('cfg_name,Fr', [('C2', 3), ('C1', 2)])
def test_savi_encoder_features_backward(dev, precision, cfg_name, Fr):
    """The SAVi image encoder under autograd (conv stack 3 -> 64 -> 64 -> 64 -> 64, position embedding, per-pixel MLP;
    savi.py:220-250,367-377): output and every parameter gradient against autograd of the oracle.  C2: 128x128 input
    (first conv stride 2), C1: 64x64."""
    from slotformer_amd import train
    cfg = gu.C2_SAVI if cfg_name == 'C2' else gu.C1_SAVI
    m, sd = build(cfg, gu.load_golden('savi_c2' if cfg_name == 'C2' else 'savi_c1'), 103, dev)
    m.train()
    img = gu.seeded_img(1, Fr, cfg['resolution'][0], 77)[0]
    dout = gu.seeded_normal((Fr, 4096, cfg['slot_dict'].get('enc_out', 128) if False else m.enc_out_channels), 78)
    names = [n for n, _ in m.named_parameters() if n.startswith(('encoder.', 'encoder_pos_embedding.dense', 'encoder_out_layer.'))]
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    ref = oracle.savi_encoder_out(img, osd, cfg)
    ref.backward(dout)
    out = train.features_with_grad(m, img.to(dev))
    out.backward(dout.to(dev))
    assert rel_err(out, ref) < 1e-4
    tol = 2.5 * L2TOL[precision]   # millions of ReLU units: kink-flip noise, see L2TOL
    got = dict(m.named_parameters())
    assert len(names) == 2 * 4 + 2 + 6
    for n in names:
        assert got[n].grad is not None, n
        assert l2_err(got[n].grad, osd[n].grad) < tol, n


def test_decoder_parameter_gradients_vs_oracle(dev, precision):
    """SAVi's own training objective back-propagates into the decoder (savi.py:527-538): gradients of the four transposed
    convs, the 1x1 head, the position-embedding Linear and the slots at the CLEVRER decoder shape."""
    cfg = gu.savi_cfg(64, 7, kernel_mlp=False, pred='mlp', rnn=False)
    m, sd = build(cfg, gu.load_golden('decode_c2'), 401, dev)
    m.train()
    Fr = 3
    slots = gu.seeded_normal((Fr, 7, 128), 41)
    target = gu.seeded_img(1, Fr, 64, 42)[0]
    names = [n for n, _ in m.named_parameters() if n.startswith(('decoder.', 'decoder_pos_embedding.dense'))]
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    so = slots.clone().requires_grad_(True)
    ((oracle.savi_decode(so, osd, cfg)[0] - target)**2).mean().backward()
    sg = slots.to(dev).requires_grad_(True)
    recon = m.decode(sg)[0]
    ((recon - target.to(dev))**2).mean().backward()
    tol = {'bf16x3': 1e-2, 'f32': 2e-3}[precision]
    got = dict(m.named_parameters())
    assert len(names) == 2 * 4 + 2 + 2
    for n in names:
        assert got[n].grad is not None, n
        assert l2_err(got[n].grad, osd[n].grad) < tol, n
    assert l2_err(sg.grad, so.grad) < tol


@pytest.mark.parametrize('name,cfg_name,T,seed,noise_seed', [('savi_train', 'TRAIN_SAVI', 2, 901, 9), ('savi_train_c1', 'C1_SAVI', 3, 911, None)])
def test_savi_training_step_golden(dev, precision, name, cfg_name, T, seed, noise_seed):
    """StoSAVi trains end to end on the HIP path: `model(batch)` in train() mode -> `calc_train_loss` -> `backward()` gives
    the reference's loss terms and gradients for every parameter.  savi_train: stosavi_clevrer_params.py (residual-MLP
    predictor, stochastic kernels); savi_train_c1: savi_obj3d_params.py (kernel MLP, Transformer + LSTM predictor whose state
    carries the graph over 3 frames).  Fixtures hold norms + strided samples from the reference; the full element-wise
    comparison is against autograd of the oracle, which the CPU suite pins to the same fixtures."""
    g = gu.load_golden(name)
    cfg = getattr(gu, cfg_name)
    m, sd = build(cfg, g, seed, dev)
    m.train()
    _no_dropout(m)
    m.testing = False
    N, D = cfg['slot_dict']['num_slots'], cfg['slot_dict']['slot_size']
    img = gu.seeded_img(1, T, 64, seed + 1)
    noise = gu.seeded_normal((1, T, N, D), noise_seed) if noise_seed is not None else None
    data = {'img': img.to(dev)}
    if noise is not None:
        data['noise'] = noise.to(dev)
    out = m(data)
    terms = m.calc_train_loss(data, out)
    loss = terms['post_recon_loss'] + float(g['kld_w']) * terms['kld_loss']
    loss.backward()
    assert abs(float(terms['kld_loss'].detach()) - float(g['kld_loss'])) <= 1e-4 * float(g['kld_loss'])
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-4 * float(g['loss'])
    assert rel_err(out['post_slots'], g['post_slots']) < 1e-4
    names = [str(n) for n in g['grad_names']]
    got = dict(m.named_parameters())
    assert sorted(n for n, p in got.items() if p.grad is not None) == sorted(names)   # e.g. prior_slot_layer stays unused
    # oracle gradients (full tensors)
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    o = oracle.savi_encode(img, osd, cfg, noise=noise)
    rec = oracle.savi_decode(o['post_slots'].flatten(0, 1), osd, cfg)[0].unflatten(0, (1, T))
    (((rec - img)**2).mean() + float(g['kld_w']) * oracle.kernel_kld(o['kernel_dist'], cfg)).backward()
    # ReLU-kink noise of the conv / decoder stacks, see above; the 3-frame fixture's gradients are ~1e-7 in size and twice as noisy
    tol = {'bf16x3': 1e-2, 'f32': 4e-3}[precision] * (2 if T > 2 else 1)
    st = int(g['stride'])
    for n, norm in zip(names, g['grad_norms']):
        if n == 'slot_attention.project_q.0.bias':
            assert got[n].grad.abs().max() < 1e-5
            continue
        assert l2_err(got[n].grad, osd[n].grad) < tol, n
        assert abs(float(got[n].grad.norm()) - float(norm)) < tol * float(norm), n
        ref = torch.from_numpy(g['gs.' + n])
        samp = got[n].grad.detach().cpu().flatten()[::st]
        assert float((samp - ref).norm()) <= tol * max(float(ref.norm()), float(norm) * (ref.numel() / got[n].numel())**0.5) * 3, n


def test_dropout_and_attention_nodes(dev):
    """The slot-level autograd nodes with dropout on (nn.TransformerEncoderLayer in train() mode inside the SAVi predictor):
    masks rebuilt on the host from the seed drive a torch restatement."""
    from slotformer_amd import train
    p, seed = 0.1, 0x0badc0de_12345678
    x = gu.seeded_normal((6, 8, 128), 51)
    xg = x.to(dev).requires_grad_(True)
    y = train._Dropout.apply(xg, p, seed)
    keep = torch.from_numpy(train.dropout_keep_mask(seed, 0, 0, 1, x.numel(), p).astype(np.float32)).view(x.shape)
    scale = 1.0 / (1.0 - float(np.float32(p)))
    assert rel_err(y, x * keep * scale) < 1e-6
    y.backward(torch.ones_like(y))
    assert rel_err(xg.grad, keep * scale) < 1e-6
    assert abs(float(keep.mean()) - 0.9) < 0.02
    # attention core with dropped softmax weights, B = 3 sequences of L = 8 slots, 4 heads of 32
    B, L, d, H = 3, 8, 128, 4
    qkv = gu.seeded_normal((B * L, 3 * d), 52)
    dctx = gu.seeded_normal((B * L, d), 53)
    qg = qkv.to(dev).requires_grad_(True)
    ctx = train._MHA.apply(qg, B, L, d, H, p, seed)
    ctx.backward(dctx.to(dev))
    qo = qkv.clone().requires_grad_(True)
    q, k, v = (t.view(B, L, H, d // H).transpose(1, 2) for t in qo.chunk(3, -1))
    att = torch.softmax((q * (d // H)**-0.5) @ k.transpose(-1, -2), dim=-1)
    am = torch.from_numpy(train.dropout_keep_mask(seed, 0, 0, 0, att.numel(), p).astype(np.float32)).view(att.shape)
    ref = ((att * am * scale) @ v).transpose(1, 2).reshape(B * L, d)
    ref.backward(dctx)
    assert rel_err(ctx, ref) < 1e-5
    assert rel_err(qg.grad, qo.grad) < 1e-4


def test_amp_bf16_policy(dev):
    """Precision mode 2 (train.amp_bf16): single-pass bf16 contractions (8 mantissa bits per operand), fp32 everything else.
    Losses stay within 1 %, the gradients within ~10 % in L2 of the fp32 references on these fixtures (seeded weights much
    larger than trained ones, plus ReLU-kink flips), and the mode is restored on exit."""
    from slotformer_amd import train, _lib
    before = _lib.lib().sf_get_precision()
    # SlotFormer with the image loss
    g = gu.load_golden('roll_train_img')
    cfg = gu.TRAIN_ROLL_IMG
    m, sd = build(cfg, g, 811, dev, vp=True)
    m.train()
    _no_dropout(m)
    data = {'slots': gu.seeded_normal((1, 5, 3, 64), 812).to(dev).requires_grad_(True), 'img': gu.seeded_img(1, 5, 64, 813).to(dev)}
    m.loss_decay_factor = 0.9
    with train.amp_bf16():
        assert _lib.lib().sf_get_precision() == 2
        out = m(data)
        terms = m.calc_train_loss(data, out)
        loss = terms['slot_recon_loss'] + terms['img_recon_loss']
        loss.backward()
    assert _lib.lib().sf_get_precision() == before
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-2 * abs(float(g['loss']))
    worst = max(l2_err(p.grad, g['grad.' + n]) for n, p in m.named_parameters() if n.startswith('rollouter.') and p.requires_grad)
    assert worst < 0.15, worst
    # StoSAVi
    g = gu.load_golden('savi_train')
    m, sd = build(gu.TRAIN_SAVI, g, 901, dev)
    m.train()
    m.testing = False
    data = {'img': gu.seeded_img(1, 2, 64, 902).to(dev), 'noise': gu.seeded_normal((1, 2, 7, 128), 9).to(dev)}
    with train.amp_bf16():
        out = m(data)
        terms = m.calc_train_loss(data, out)
        loss = terms['post_recon_loss'] + float(g['kld_w']) * terms['kld_loss']
        loss.backward()
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-2 * float(g['loss'])
    got = dict(m.named_parameters())
    errs = {n: abs(float(got[n].grad.norm()) - float(norm)) / float(norm) for n, norm in zip((str(x) for x in g['grad_names']), g['grad_norms'])
            if n != 'slot_attention.project_q.0.bias'}
    assert max(errs.values()) < 0.15, sorted(errs.items(), key=lambda kv: -kv[1])[:3]


def test_flat_adam_matches_torch(dev):
    """train.FlatAdam (one sf_adam_flat_f32 launch over the flat parameter bucket) against torch.optim.Adam, the reference's
    optimiser, over several steps on the rollouter's parameters with synthetic gradients."""
    from slotformer_amd import train
    from slotformer_amd.video_prediction.models import SlotRollouter
    torch.manual_seed(3)
    a = SlotRollouter(**gu.C1_ROLL['rollout_dict']).to(dev)
    b = SlotRollouter(**gu.C1_ROLL['rollout_dict']).to(dev)
    b.load_state_dict(a.state_dict())
    ref = torch.optim.Adam([p for p in a.parameters() if p.requires_grad], lr=2e-4)
    opt = train.FlatAdam(b.parameters(), lr=2e-4)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))   # re-pointing kept the values
    for step in range(5):
        g = torch.Generator(device='cpu').manual_seed(100 + step)
        for pa, pb in zip([p for p in a.parameters() if p.requires_grad], opt.params):
            gr = torch.randn(pa.shape, generator=g).to(dev) * 0.1
            pa.grad, pb.grad = gr.clone(), gr.clone()
        ref.step()
        opt.step()
    for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert rel_err(pb, pa.detach().cpu()) < 1e-5, n   # fp32 rounding of the bias corrections
    # the parameters are views of one bucket, and the inference engine sees the updated values
    assert opt.params[0].data_ptr() == opt.flat.data_ptr()
    x = gu.seeded_normal((2, 6, 6, 128), 5).to(dev)
    with torch.no_grad():
        assert rel_err(b.eval()(x, 3), a.eval()(x, 3).cpu()) < 1e-5


def test_decoder_gradients_phyre_shape(dev):
    """The PHYRE decoder (savi_phyre_params: 8 slots, 16x16 broadcast grid -> 128x128, so the stride-1 layer runs on the GEMM
    core instead of the 64-wide halo kernel and the weight-gradient windows are 128 pixels wide): slot and parameter
    gradients against autograd of the oracle."""
    cfg = gu.C5_SAVI
    m, sd = build(cfg, gu.load_golden('savi_c5'), 105, dev)
    m.train()
    slots = gu.seeded_normal((1, 8, 128), 61)
    target = gu.seeded_img(1, 1, 128, 62)[0]
    names = [n for n, _ in m.named_parameters() if n.startswith(('decoder.', 'decoder_pos_embedding.dense'))]
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    so = slots.clone().requires_grad_(True)
    ref = oracle.savi_decode(so, osd, cfg)[0]
    ((ref - target)**2).mean().backward()
    sg = slots.to(dev).requires_grad_(True)
    recon = m.decode(sg)[0]
    assert rel_err(recon, ref) < 1e-4
    ((recon - target.to(dev))**2).mean().backward()
    got = dict(m.named_parameters())
    for n in names:
        assert l2_err(got[n].grad, osd[n].grad) < 1e-2, n
    assert l2_err(sg.grad, so.grad) < 1e-2


def test_savi_training_step_128_vs_oracle(dev):
    """StoSAVi at the north-star resolution (C2: 128x128 input, first conv stride 2, decoder 8x8 -> 128x128 in four stride-2
    layers): one training step against autograd of the oracle."""
    cfg = gu.C2_SAVI
    m, sd = build(cfg, gu.load_golden('savi_c2'), 103, dev)
    m.train()
    m.testing = False
    img = gu.seeded_img(1, 2, 128, 71)
    noise = gu.seeded_normal((1, 2, 7, 128), 72)
    data = {'img': img.to(dev), 'noise': noise.to(dev)}
    out = m(data)
    terms = m.calc_train_loss(data, out)
    loss = terms['post_recon_loss'] + 1e-4 * terms['kld_loss']
    loss.backward()
    got = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    osd = {k: (v.clone().requires_grad_(True) if k in got else v) for k, v in sd.items()}
    o = oracle.savi_encode(img, osd, cfg, noise=noise)
    rec = oracle.savi_decode(o['post_slots'].flatten(0, 1), osd, cfg)[0].unflatten(0, (1, 2))
    oloss = ((rec - img)**2).mean() + 1e-4 * oracle.kernel_kld(o['kernel_dist'], cfg)
    oloss.backward()
    assert abs(float(loss.detach()) - float(oloss.detach())) < 1e-4 * float(oloss.detach())
    assert rel_err(out['post_slots'], o['post_slots']) < 1e-4
    assert len(got) == 54
    for n, g_ in got.items():
        if n == 'slot_attention.project_q.0.bias':
            continue
        assert l2_err(g_, osd[n].grad) < 1.5e-2, n


def test_steve_decoder_training_vs_oracle(dev, precision):
    """STEVETransformerDecoder.forward under autograd (steve_transformer.py:275-303: token + position embedding, blocks of
    causal self-attention / slot cross-attention / FFN, head) with the token cross-entropy of steve.py:341-344: logits, loss
    and the gradients of every decoder parameter and of the slots against autograd of the oracle.  257 tokens (16x16 patch
    grid + BOS), 4 slots, 2 blocks."""
    from slotformer_amd import train
    g = gu.load_golden('steve_tokens')
    cfg = gu.steve_tokens_cfg()
    m, sd = build(cfg, g, 601, dev)
    dec = m.trans_decoder
    dec.train()
    _no_dropout(dec)
    slots = gu.seeded_normal((2, 4, 64), 81)
    tgt = torch.from_numpy(g['target_token_id']).to(torch.int64)          # [2, 256]
    names = [n for n, p_ in m.named_parameters() if n.startswith('trans_decoder.') and p_.requires_grad]
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    so = slots.clone().requires_grad_(True)
    dd = cfg['dec_dict']
    ref = oracle.steve_decoder_forward(so, tgt[:, :-1], osd, dd['dec_num_heads'], dd['dec_num_layers'])
    oloss = torch.nn.functional.cross_entropy(ref.flatten(0, 1), tgt.flatten(0, 1))
    oloss.backward()
    sg = slots.to(dev).requires_grad_(True)
    logits = dec(sg, tgt[:, :-1].to(dev))
    loss = train.token_cross_entropy(logits.flatten(0, 1), tgt.flatten(0, 1).to(dev))
    loss.backward()
    assert rel_err(logits, ref) < 1e-4
    assert abs(float(loss.detach()) - float(oloss.detach())) < 1e-5 * float(oloss.detach())
    got = dict(m.named_parameters())
    tol = L2TOL[precision]
    for n in names:
        assert got[n].grad is not None, n
        assert l2_err(got[n].grad, osd[n].grad) < tol, n
    assert l2_err(sg.grad, so.grad) < tol


def test_steve_training_step_golden(dev, precision):
    """STEVE trains end to end on the HIP path (steve.py:242-351): encoder side (conv stack, Slot Attention, Transformer +
    LSTM predictor) -> slots -> teacher-forced Transformer decoder -> token cross-entropy against the frozen dVAE's tokens.
    Loss and gradients against the reference fixture (norms + strided samples) and, in full, against autograd of the oracle."""
    g = gu.load_golden('steve_train')
    cfg = gu.steve_tokens_cfg()
    m, sd = build(cfg, g, 921, dev)
    m.train()
    _no_dropout(m)
    m.testing = False
    img = gu.seeded_img(1, 2, 64, seed=922)
    tok = torch.from_numpy(g['target_token_id']).to(dev).unflatten(0, (1, 2))   # the reference's targets (argmax ties aside)
    data = {'img': img.to(dev), 'token_id': tok}
    out = m(data)
    loss = m.calc_train_loss(data, out)['token_recon_loss']
    loss.backward()
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-4 * float(g['loss'])
    assert rel_err(out['slots'], g['slots']) < 1e-4
    assert out['masks'].shape == (1, 2, 4, 64, 64) and not out['masks'].requires_grad
    names = [str(n) for n in g['grad_names']]
    got = dict(m.named_parameters())
    assert sorted(n for n, p in got.items() if p.grad is not None) == sorted(names)
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    enc = oracle.steve_encode(img, osd, cfg, training=True)
    oracle.steve_forward_tokens(img, enc['slots'], osd, cfg)['token_recon_loss'].backward()
    tol = {'bf16x3': 1e-2, 'f32': 4e-3}[precision]
    for n, norm in zip(names, g['grad_norms']):
        if n == 'slot_attention.project_q.0.bias' or float(norm) == 0.:
            # structurally zero gradients: the LN_q bias (see above) and, with a single predictor step from a zero LSTM
            # state, weight_hh_l0
            assert got[n].grad.abs().max() < 1e-5, n
            continue
        assert l2_err(got[n].grad, osd[n].grad) < tol, n
        assert abs(float(got[n].grad.norm()) - float(norm)) < tol * float(norm), n
    # the computed-on-device tokens path (no 'token_id' given) runs too and gives (almost) the same loss
    for p_ in m.parameters():
        p_.grad = None
    out2 = m({'img': img.to(dev)})
    l2 = m.calc_train_loss({'img': img.to(dev)}, out2)['token_recon_loss']
    l2.backward()
    assert abs(float(l2.detach()) - float(g['loss'])) < 2e-2 * float(g['loss'])


def test_steve_training_with_all_dropouts(dev):
    """STEVE in plain train() mode (the reference's default dropout 0.1 on the embedding, the attention weights, the attention
    outputs and the FFN of the decoder, and inside the Transformer predictor): a few FlatAdam steps on one batch run and
    bring the token loss down."""
    from slotformer_amd import train
    g = gu.load_golden('steve_train')
    m, sd = build(gu.steve_tokens_cfg(), g, 921, dev)
    m.train()
    m.testing = False
    assert m.trans_decoder.tf_dec.blocks[0].self_attn.attn_dropout.p > 0
    data = {'img': gu.seeded_img(2, 2, 64, seed=923).to(dev)}
    opt = train.FlatAdam([p for p in m.parameters() if p.requires_grad], lr=3e-4)
    torch.manual_seed(0)

    def eval_loss():   # dropout-free measurement on the inference path
        m.eval()
        with torch.no_grad():
            v = float(m.calc_train_loss(data, m(data))['token_recon_loss'])
        m.train()
        return v

    before, hist = eval_loss(), []
    for _ in range(8):
        opt.zero_grad()
        out = m(data)
        loss = m.calc_train_loss(data, out)['token_recon_loss']
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
    after = eval_loss()
    assert all(np.isfinite(hist)) and after < before - 1e-3, (before, after, hist)


def test_steve_slotformer_training_vs_oracle(dev, tmp_path):
    """STEVESlotFormer's training objective (steve_slotformer.py:111-161): slot MSE of the rollout plus the token
    cross-entropy of the FROZEN STEVE decoder on the frozen dVAE's tokens of the target frames -- the decoder only passes the
    gradient on to the predicted slots.  Loss terms and rollouter gradients against autograd of the oracle."""
    from slotformer_amd.base_slots import build_model as bb
    from slotformer_amd.video_prediction import build_model as bv
    g = gu.load_golden('steve_slotformer')
    steve = bb(gu.ParamsView(gu.steve_tokens_cfg()))
    path = str(tmp_path / 'steve.pth')
    torch.save({'state_dict': steve.state_dict()}, path)
    cfg = gu.steve_slotformer_cfg()
    cfg['dec_dict']['dec_ckp_path'] = path
    m = bv(gu.ParamsView(cfg))
    shapes = gu.shapes_from_golden(g)
    own = dict(m.state_dict())
    sd = gu.seeded_state_dict(shapes, 701, keep=own)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    _no_dropout(m)
    rd = cfg['rollout_dict']
    hist, S = rd['history_len'], cfg['loss_dict']['rollout_len']
    slots = gu.seeded_normal((1, hist + S, rd['num_slots'], rd['slot_size']), 702)
    tok = torch.from_numpy(g['target_token_id']).to(torch.int64)                  # [S, h*w], the reference's targets
    data = {'slots': slots.to(dev), 'token_id': tok.to(dev).unflatten(0, (1, S))}
    out = m(data)
    terms = m.calc_train_loss(data, out)
    assert abs(float(terms['img_recon_loss'].detach()) - float(g['img_recon_loss'])) < 1e-3 * float(g['img_recon_loss'])
    (terms['slot_recon_loss'] + terms['img_recon_loss']).backward()
    names = [n for n, p_ in m.named_parameters() if p_.requires_grad]
    assert names and all(n.startswith('rollouter.') for n in names)
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    pred = oracle.rollouter_forward(slots[:, :hist], S, osd, rd)
    dd = cfg['dec_dict']
    logits = oracle.steve_decoder_forward(pred.flatten(0, 1), tok[:, :-1], osd, dd['dec_num_heads'], dd['dec_num_layers'], p='decoder.')
    (((pred - slots[:, hist:])**2).mean() + torch.nn.functional.cross_entropy(logits.flatten(0, 1), tok.flatten(0, 1))).backward()
    got = dict(m.named_parameters())
    for n in names:
        assert l2_err(got[n].grad, osd[n].grad) < L2TOL['bf16x3'], n
    assert all(p_.grad is None for n, p_ in m.named_parameters() if not n.startswith('rollouter.'))


# ---- the dVAE's own training (dVAE.py:102-146) ----------------------------------------------------------------------
@pytest.mark.parametrize('F_,H,W,C,relu,shuffle', [(2, 8, 8, 64, True, 1), (3, 4, 6, 256, True, 2), (1, 16, 16, 64, False, 1)])
def test_groupnorm1_backward_vs_torch(dev, F_, H, W, C, relu, shuffle):
    """sf_groupnorm1_nhwc_bwd_f32 against torch autograd of F.group_norm(x, 1) (+ReLU, + PixelShuffle(2)) in NCHW."""
    from slotformer_amd import train
    rs = np.random.RandomState(F_ * 100 + C)
    x = torch.from_numpy(rs.standard_normal((F_, H, W, C)).astype(np.float32) * 2 + 0.3)
    gam = torch.from_numpy(rs.standard_normal(C).astype(np.float32) * 0.5 + 1)
    bet = torch.from_numpy(rs.standard_normal(C).astype(np.float32) * 0.3)
    dy = torch.from_numpy(rs.standard_normal((F_, H * shuffle, W * shuffle, C // shuffle**2)).astype(np.float32))
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gam, bet))
    y = torch.nn.functional.group_norm(xr.permute(0, 3, 1, 2), 1, gr, br, 1e-5)
    y = torch.relu(y) if relu else y
    y = torch.nn.functional.pixel_shuffle(y, 2) if shuffle == 2 else y
    y = y.permute(0, 2, 3, 1)
    (y * dy).sum().backward()
    xd, gd, bd = (t.to(dev).requires_grad_(True) for t in (x, gam, bet))
    yd = train.groupnorm1(xd, gd, bd, relu=relu, pixel_shuffle=shuffle)
    (yd * dy.to(dev)).sum().backward()
    assert rel_err(yd, y.detach()) < 1e-5
    assert l2_err(xd.grad, xr.grad) < 1e-5
    assert l2_err(gd.grad, gr.grad) < 1e-5
    assert l2_err(bd.grad, br.grad) < 1e-5


@pytest.mark.parametrize('hard', [False, True])
def test_gumbel_softmax_node_vs_torch(dev, hard):
    from slotformer_amd import train
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.standard_normal((3, 4, 4, 96)).astype(np.float32))
    gn = torch.from_numpy(rs.gumbel(size=(3, 4, 4, 96)).astype(np.float32))
    dy = torch.from_numpy(rs.standard_normal((3, 4, 4, 96)).astype(np.float32))
    xr = x.clone().requires_grad_(True)
    ys = torch.softmax((torch.log_softmax(xr, -1) + gn) / 0.7, -1)
    if hard:
        yh = torch.zeros_like(ys).scatter_(-1, ys.argmax(-1, keepdim=True), 1.)
        ys = yh - ys.detach() + ys
    (ys * dy).sum().backward()
    xd = x.to(dev).requires_grad_(True)
    yd = train.gumbel_softmax(xd, gn.to(dev), 0.7, hard)
    (yd * dy.to(dev)).sum().backward()
    assert rel_err(yd, ys.detach()) < 1e-5
    assert l2_err(xd.grad, xr.grad) < 1e-5


def test_padded_linear_and_conv3x3_nodes_vs_torch(dev, precision):
    """linear_weight on widths that are not multiples of 64 (the dVAE's 48-wide patch vectors and 3-channel output) and the
    3x3 convolution node, against torch autograd."""
    from slotformer_amd import train
    rs = np.random.RandomState(9)
    tol = {'bf16x3': 2e-5, 'f32': 2e-5}[precision]
    for (M, K, N, bias) in [(70, 48, 64, False), (33, 64, 3, True), (10, 100, 130, True)]:
        x = torch.from_numpy(rs.standard_normal((M, K)).astype(np.float32))
        w = torch.from_numpy(rs.standard_normal((N, K)).astype(np.float32) * 0.2)
        b = torch.from_numpy(rs.standard_normal(N).astype(np.float32)) if bias else None
        dy = torch.from_numpy(rs.standard_normal((M, N)).astype(np.float32))
        ref = [t.clone().requires_grad_(True) if t is not None else None for t in (x, w, b)]
        (torch.nn.functional.linear(*ref) * dy).sum().backward()
        got = [t.to(dev).requires_grad_(True) if t is not None else None for t in (x, w, b)]
        y = train.linear_weight(*got)
        (y * dy.to(dev)).sum().backward()
        assert rel_err(y, torch.nn.functional.linear(x, w, b)) < tol
        for a_, r_ in zip(got, ref):
            if a_ is not None:
                assert l2_err(a_.grad, r_.grad) < tol, (M, K, N)
    x = torch.from_numpy(rs.standard_normal((2, 6, 5, 64)).astype(np.float32))
    w = torch.from_numpy(rs.standard_normal((64, 64, 3, 3)).astype(np.float32) * 0.1)
    dy = torch.from_numpy(rs.standard_normal((2, 6, 5, 64)).astype(np.float32))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr.permute(0, 3, 1, 2), wr, padding=1).permute(0, 2, 3, 1)
    (yr * dy).sum().backward()
    xd, wd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    yd = train.conv3x3_nhwc(xd, wd)
    (yd * dy.to(dev)).sum().backward()
    assert rel_err(yd, yr.detach()) < tol
    assert l2_err(xd.grad, xr.grad) < tol and l2_err(wd.grad, wr.grad) < tol


@pytest.mark.parametrize('name,B,res,vocab,seed', [('dvae_train', 2, 32, 64, 71), ('dvae_train_hard', 1, 16, 128, 73)])
def test_dvae_training_step_golden(dev, precision, name, B, res, vocab, seed):
    """The dVAE trains on the HIP path (model='dVAE', dVAE.py:102-146): loss, reconstruction and every parameter gradient
    against the reference fixture (norms + strided samples) and, in full, against autograd of the oracle."""
    from slotformer_amd.base_slots.models.dVAE import dVAE
    g = gu.load_golden(name)
    shapes = gu.shapes_from_golden(g)
    m = dVAE(vocab)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == shapes
    sd = gu.seeded_state_dict(shapes, seed)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    img = gu.seeded_img(B, 1, res, seed=seed + 1)[:, 0]
    gum = torch.from_numpy(g['gumbel'])
    tau, hard = float(g['tau']), bool(int(g['hard']))
    data = {'img': img.to(dev), 'gumbel': gum.to(dev), 'gumbel_tau': tau, 'hard': hard}
    out = m(data)
    loss = m.calc_train_loss(data, out)['recon_loss']
    loss.backward()
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-4 * float(g['loss'])
    assert rel_err(out['recon'], g['recon']) < 1e-4
    assert rel_err(out['z_logits'][:, ::5], g['z_logits']) < 1e-4
    names = [str(n) for n in g['grad_names']]
    got = dict(m.named_parameters())
    assert sorted(n for n, p in got.items() if p.grad is not None) == sorted(names)
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    oracle.dvae_forward_train(img, gum, osd, tau, hard)['recon_loss'].backward()
    # Exact-f32 contractions reproduce the reference's gradients to ~4e-6.  Under split-bf16 the activations move by ~1e-5,
    # which is enough to carry one of the 8192 pre-activations of a block across its ReLU kink; with only 128 pixel rows a
    # single flipped gate moves every gradient upstream of it by |g_i| / ||g|| ~ 1/64 (measured: 2.7e-2 behind decoder.1,
    # 1.8e-5 in front of it), so that mode is held to a flip-sized bound here and to 2e-5 at op level above.
    tol = {'bf16x3': 8e-2, 'f32': 1e-4}[precision]
    for n, norm in zip(names, g['grad_norms']):
        assert l2_err(got[n].grad, osd[n].grad) < tol, n
        assert abs(float(got[n].grad.norm()) - float(norm)) < tol * float(norm), n
    # a video batch [B,T,...] and a fresh on-device Gumbel draw run as well
    out5 = m({'img': img.to(dev).unsqueeze(0)})
    assert out5['recon'].shape == (1, B, 3, res, res) and out5['z_logits'].shape == (1, B, vocab, res // 4, res // 4)


def test_dvae_training_reduces_loss(dev):
    from slotformer_amd import train
    from slotformer_amd.base_slots.models.dVAE import dVAE
    torch.manual_seed(3)
    m = dVAE(64).to(dev).train()
    data = {'img': gu.seeded_img(4, 1, 32, seed=5)[:, 0].to(dev)}
    opt = train.FlatAdam(m.parameters(), lr=1e-3)
    hist = []
    for _ in range(12):
        opt.zero_grad()
        loss = m.loss_function(data)['recon_loss']
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
    assert all(np.isfinite(hist)) and hist[-1] < 0.9 * hist[0], hist


def test_steve_training_step_with_image_loss_golden(dev, precision):
    """STEVE's optional image term (use_img_recon_loss=True, steve.py:327-335, 345-349) on the HIP path: the predicted token
    logits -> Gumbel-softmax node (tau 0.1, the fixture's noise) -> the frozen dVAE's decoder as differentiable nodes -> MSE.
    Both loss terms and the gradients of their sum against the reference fixture and autograd of the oracle."""
    g = gu.load_golden('steve_train_img')
    cfg = gu.steve_tokens_cfg()
    cfg['loss_dict'] = dict(use_img_recon_loss=True)
    m, sd = build(cfg, g, 931, dev)
    m.train()
    _no_dropout(m)
    m.testing = False
    img = gu.seeded_img(1, 2, 64, seed=932)
    gum = torch.from_numpy(g['gumbel'])
    tok = torch.from_numpy(g['target_token_id']).to(dev).unflatten(0, (1, 2))
    data = {'img': img.to(dev), 'token_id': tok, 'gumbel': gum.to(dev)}
    out = m(data)
    terms = m.calc_train_loss(data, out)
    (terms['token_recon_loss'] + terms['img_recon_loss']).backward()
    assert abs(float(terms['token_recon_loss'].detach()) - float(g['loss'])) < 1e-4 * float(g['loss'])
    assert abs(float(terms['img_recon_loss'].detach()) - float(g['img_loss'])) < 1e-3 * float(g['img_loss'])
    assert rel_err(out['recon_img'], g['recon_img']) < 2e-3   # tau 0.1 multiplies logit differences by 10 before the softmax
    names = [str(n) for n in g['grad_names']]
    got = dict(m.named_parameters())
    assert sorted(n for n, p in got.items() if p.grad is not None) == sorted(names)
    assert all(p.grad is None for p in m.dvae.parameters())
    osd = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    enc = oracle.steve_encode(img, osd, cfg, training=True)
    o = oracle.steve_forward_tokens(img, enc['slots'], osd, cfg, gum)
    (o['token_recon_loss'] + o['img_recon_loss']).backward()
    tol = {'bf16x3': 8e-2, 'f32': 4e-3}[precision]   # bf16x3: ReLU-gate flips in the 8x8 dVAE blocks, see the dVAE test above
    for n, norm in zip(names, g['grad_norms']):
        if n == 'slot_attention.project_q.0.bias' or float(norm) == 0.:
            assert got[n].grad.abs().max() < 1e-5, n
            continue
        assert l2_err(got[n].grad, osd[n].grad) < tol, n
        assert abs(float(got[n].grad.norm()) - float(norm)) < tol * float(norm), n
    # evaluation (no autograd) reports both terms too, with a fresh noise draw
    m.eval()
    with torch.no_grad():
        ev = m.calc_eval_loss({'img': img.to(dev)}, m({'img': img.to(dev)}))
    assert set(ev) == {'token_recon_loss', 'img_recon_loss'} and all(np.isfinite(float(v)) for v in ev.values())


@pytest.mark.parametrize('V', [64, 1000, 4096, 4100, 5000])
def test_in_kernel_gumbel_noise_and_log_softmax(dev, V):
    """sf_gumbel_softmax_rows_f32 draws its noise inside the kernel: the same call with the host restatement of that noise
    (train.gumbel_noise) as an explicit `add` tensor gives the same rows; the noise has Gumbel(0, 1) moments; log-softmax
    rows against torch.  Row lengths on the register-resident path (<= 4096, multiple of 4) and on the generic one."""
    from slotformer_amd import ops, train
    R = 37
    x = torch.from_numpy(np.random.RandomState(V).standard_normal((R, V)).astype(np.float32)).to(dev)
    seed = 0x1234_5678_9abc_def1
    noise = train.gumbel_noise(seed, R * V).reshape(R, V)
    y = ops.gumbel_softmax_rows(x, seed, 1. / 0.7)
    ref = ops.softmax_rows(x, noise.to(dev), 1. / 0.7)
    assert rel_err(y, ref.cpu()) < 1e-4
    assert rel_err(ref, torch.softmax((x.cpu() + noise) / 0.7, -1)) < 1e-5
    assert abs(float(noise.mean()) - 0.5772) < 0.02 and abs(float(noise.var()) - np.pi**2 / 6) < 0.06
    assert not torch.equal(y, ops.gumbel_softmax_rows(x, seed + 1, 1. / 0.7))
    assert rel_err(ops.log_softmax_rows(x), torch.log_softmax(x.cpu(), -1)) < 1e-6
    # the node: backward through the in-kernel noise path equals the backward with the noise given
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    dy = torch.from_numpy(np.random.RandomState(1).standard_normal((R, V)).astype(np.float32)).to(dev)
    (train.gumbel_softmax(xa, None, 0.7, seed=seed) * dy).sum().backward()
    (train.gumbel_softmax(xb, noise.to(dev), 0.7) * dy).sum().backward()
    assert l2_err(xa.grad, xb.grad.cpu()) < 1e-4


@pytest.mark.parametrize('R,V', [(37, 64), (100, 1000), (16, 4096), (9, 4097), (5, 10000)])
def test_token_cross_entropy_backward_vs_torch(dev, R, V):
    """sf_cross_entropy_bwd_f32 (one kernel: softmax - onehot, scaled by the upstream gradient read on the device) against
    torch autograd of F.cross_entropy, on the register-resident row sizes and beyond, with a non-unit upstream factor."""
    from slotformer_amd import train
    rs = np.random.RandomState(R + V)
    x = torch.from_numpy((rs.standard_normal((R, V)) * 3).astype(np.float32))
    tgt = torch.from_numpy(rs.randint(0, V, size=R).astype(np.int64))
    xr = x.clone().requires_grad_(True)
    (torch.nn.functional.cross_entropy(xr, tgt) * 0.37).backward()
    xd = x.to(dev).requires_grad_(True)
    loss = train.token_cross_entropy(xd, tgt.to(dev))
    (loss * 0.37).backward()
    assert abs(float(loss.detach()) - float(torch.nn.functional.cross_entropy(x, tgt))) < 1e-5 * max(1., float(loss.detach()))
    assert l2_err(xd.grad, xr.grad) < 1e-5
