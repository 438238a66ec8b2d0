"""GPU: 9 .. 16 slots through every layer that had an 8-slot bound -- the Slot-Attention iteration kernels (VALU, two-pass MFMA, one-pass tile),
their backward, the training of the module, the encode / rollout / training step of whole models against the fixtures of
tools/gen_golden_slots16.py, and the batch pipeline.  Every tolerance is the one of the 8-slot test of the same thing."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import oracle
import slots16_cases as sc
import test_engine_gpu as teg
import test_pipeline_gpu as tpg
import test_train_gpu as ttg
from test_kernels_gpu import close, rnd

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------
# the iteration
def _iteration_f64(k, v, q, eps=1e-6):
    """savi.py:82-94 in float64: (attention [B, N, HW], updates [B, N, D])"""
    k, v, q = k.double(), v.double(), q.double()
    a = torch.softmax(k.shape[-1]**-0.5 * torch.einsum('bnc,bmc->bnm', k, q), -1)
    ae = a + eps
    return a.permute(0, 2, 1), torch.einsum('bnm,bnc->bmc', ae / ae.sum(1, keepdim=True), v)


def _slot_update_f64(upd, slots, w_ih, w_hh, b_ih, b_hh, g, be, w1, b1, w2, b2):
    """savi.py:95-100 in float64"""
    d = lambda *xs: [x.double() for x in xs]  # noqa: E731
    upd, slots, w_ih, w_hh, b_ih, b_hh, g, be, w1, b1, w2, b2 = d(upd, slots, w_ih, w_hh, b_ih, b_hh, g, be, w1, b1, w2, b2)
    B, N, D = slots.shape
    h = oracle.gru_cell(upd.reshape(B * N, D), slots.reshape(B * N, D), w_ih, w_hh, b_ih, b_hh).view(B, N, D)
    return h + F.linear(F.relu(F.linear(F.layer_norm(h, (D, ), g, be), w1, b1)), w2, b2)


ITER_CASES = [(2, 9, 128, 512), (2, 16, 128, 1024), (2, 11, 192, 256), (1, 16, 256, 256), (2, 13, 64, 256), (2, 16, 128, 80), (3, 11, 128, 4096)]


@pytest.mark.parametrize('B,N,D,HW', ITER_CASES)
def test_iteration_against_float64(dev, B, N, D, HW):
    """One iteration (attention half + slot update) at 9 .. 16 slots against the float64 restatement of savi.py:76-100: separate key and value
    rows (HW % 256 == 0: the two-pass kernel, else the VALU kernel) and, at slot size 128 with HW % 512 == 0, keys == values (the one-pass tile
    kernel: sums in the even partial records, zeros in the odd ones).  Deterministic; a video's records do not depend on its batch."""
    from slotformer_amd import ops
    H = 2 * D
    k, v, q = rnd(B, HW, D, seed=1), rnd(B, HW, D, seed=2), rnd(B, N, D, seed=3)
    slots = rnd(B, N, D, seed=4)
    kd, vd, qd = k.to(dev), v.to(dev), q.to(dev)
    pn, pd, attn = ops.slot_attn_iter(kd, vd, qd, want_attn=True)
    a64, upd64 = _iteration_f64(k, v, q)
    close(attn, a64, rtol=1e-5, atol=1e-6)
    close(pn.sum(1) / pd.sum(1).unsqueeze(-1), upd64, rtol=1e-5, atol=1e-6)
    w_ih, w_hh = rnd(3 * D, D, seed=5, scale=D**-0.5), rnd(3 * D, D, seed=6, scale=D**-0.5)
    b_ih, b_hh = rnd(3 * D, seed=7, scale=0.1), rnd(3 * D, seed=8, scale=0.1)
    g, be = 1 + 0.1 * rnd(D, seed=9), 0.1 * rnd(D, seed=10)
    w1, b1, w2, b2 = rnd(H, D, seed=11, scale=D**-0.5), rnd(H, seed=12, scale=0.1), rnd(D, H, seed=13, scale=H**-0.5), rnd(D, seed=14, scale=0.1)
    ref = _slot_update_f64(upd64, slots, w_ih, w_hh, b_ih, b_hh, g, be, w1, b1, w2, b2)
    t = lambda *xs: [x.to(dev) for x in xs]  # noqa: E731
    out = ops.slot_update(pn, pd, slots.to(dev), t(w_ih, w_hh, b_ih, b_hh), *t(g, be, w1, b1, w2, b2))
    close(out, ref)
    # deterministic, and a video alone gives the records it gives inside the batch
    pnb, pdb, _ = ops.slot_attn_iter(kd, vd, qd)
    assert torch.equal(pnb, pn) and torch.equal(pdb, pd)
    i = B - 1
    pn1, pd1, at1 = ops.slot_attn_iter(kd[i:i + 1].contiguous(), vd[i:i + 1].contiguous(), qd[i:i + 1].contiguous(), want_attn=True)
    assert torch.equal(pn1[0], pn[i]) and torch.equal(pd1[0], pd[i]) and torch.equal(at1[0], attn[i])
    # keys == values: the same rows through one buffer against two separate copies of them
    pna, pda, ata = ops.slot_attn_iter(kd, kd, qd, want_attn=True)
    pns, pds, ats = ops.slot_attn_iter(kd, kd.clone(), qd, want_attn=True)
    a64, upd64 = _iteration_f64(k, k, q)
    close(ata, a64, rtol=1e-5, atol=1e-6)
    close(pna.sum(1) / pda.sum(1).unsqueeze(-1), upd64, rtol=1e-5, atol=1e-6)
    close(pna.sum(1), pns.sum(1).cpu(), rtol=1e-4, atol=1e-3)
    close(pda.sum(1), pds.sum(1).cpu(), rtol=1e-5, atol=1e-4)
    close(ata, ats.cpu(), rtol=1e-5, atol=1e-6)
    tile = D == 128 and HW % 512 == 0
    if tile:   # the tile kernel ran: odd records are zero, and it is another kernel than the two-pass one
        assert torch.equal(pna[:, 1::2], torch.zeros_like(pna[:, 1::2])) and torch.equal(pda[:, 1::2], torch.zeros_like(pda[:, 1::2]))
        assert not torch.equal(pna, pns) and bool((pns[:, 1::2] != 0).any())
        assert pna.shape[1] == HW // 256
    else:      # one kernel for both calls
        assert torch.equal(pna, pns) and torch.equal(pda, pds)
    pn1, pd1, at1 = ops.slot_attn_iter(kd[i:i + 1].contiguous(), kd[i:i + 1].contiguous(), qd[i:i + 1].contiguous(), want_attn=True)
    assert torch.equal(pn1[0], pna[i]) and torch.equal(pd1[0], pda[i]) and torch.equal(at1[0], ata[i])


def test_tile16_switch_sends_keys_equal_values_to_the_two_pass_kernel(dev):
    """sf_set_slot_attn_tile16(0): 9 .. 16 slots with keys == values take the two-pass kernel (dense records) -- the bits of the call on separate
    copies; 8 slots are not touched by the switch."""
    from slotformer_amd import ops, _lib
    lib = _lib.lib()
    x, q16, q8 = rnd(2, 1024, 128, seed=41).to(dev), rnd(2, 16, 128, seed=42).to(dev), rnd(2, 8, 128, seed=43).to(dev)
    on16, on8 = ops.slot_attn_iter(x, x, q16), ops.slot_attn_iter(x, x, q8)
    sep16 = ops.slot_attn_iter(x, x.clone(), q16)
    old = lib.sf_get_slot_attn_tile16()
    lib.sf_set_slot_attn_tile16(0)
    try:
        off16, off8 = ops.slot_attn_iter(x, x, q16), ops.slot_attn_iter(x, x, q8)
    finally:
        lib.sf_set_slot_attn_tile16(old)
    assert torch.equal(off16[0], sep16[0]) and torch.equal(off16[1], sep16[1]) and not torch.equal(off16[0], on16[0])
    assert torch.equal(off8[0], on8[0]) and torch.equal(off8[1], on8[1])


def test_iteration_bf16_storage_16_slots(dev):
    """sf_slot_attn_iter_bf16 at 16 slots (the case B 2, N 16, D 128, HW 1024 of the table above): the bits of the f32 entry point on the
    bf16-ROUNDED rows, and the float64 restatement on those rows."""
    from slotformer_amd._lib import lib, check
    B, HW, N, D = 2, 1024, 16, 128
    rs = np.random.RandomState(21)
    kv = torch.from_numpy(rs.standard_normal((B, HW, 2 * D)).astype(np.float32)).to(dev)
    q = torch.from_numpy(rs.standard_normal((B, N, D)).astype(np.float32)).to(dev)
    kv16 = kv.to(torch.bfloat16).contiguous()
    kvr = kv16.float().contiguous()
    P = lib().sf_slot_attn_num_partials(HW)
    st = torch.cuda.current_stream().cuda_stream

    def run(fn, kvt, esz):
        num, den, at = torch.zeros(B, P, N, D, device=dev), torch.zeros(B, P, N, device=dev), torch.zeros(B, N, HW, device=dev)
        check(fn(C.c_void_p(kvt.data_ptr()), C.c_void_p(kvt.data_ptr() + esz * D), 2 * D, HW * 2 * D, q.data_ptr(),
                 num.data_ptr(), den.data_ptr(), at.data_ptr(), B, HW, N, D, D ** -0.5, 1e-6, st))
        return num, den, at

    n16, d16, a16 = run(lib().sf_slot_attn_iter_bf16, kv16, 2)
    nr, dr, ar = run(lib().sf_slot_attn_iter_f32, kvr, 4)
    torch.cuda.synchronize()
    assert torch.equal(n16, nr) and torch.equal(d16, dr) and torch.equal(a16, ar)
    a64, upd64 = _iteration_f64(kvr[..., :D].cpu(), kvr[..., D:].cpu(), q.cpu())
    close(a16, a64, rtol=1e-5, atol=1e-6)
    close(n16.sum(1) / d16.sum(1).unsqueeze(-1), upd64, rtol=1e-5, atol=1e-6)


def test_8_slots_keep_their_kernels(dev):
    """N = 8 has one route through the new dispatch, the 8-slot instantiations: keys == values at slot size 128 leave the tile kernel's record
    structure (odd records zero, dense under separate copies), whatever sf_set_slot_attn_tile16 says; and the backward by the new entry point
    is the backward by the 8-slot entry point, bit for bit (both run sa_iter_bwd_kernel<D, 8, 0>)."""
    from slotformer_amd import ops
    from slotformer_amd._lib import lib, check
    B, HW, N, D = 2, 1024, 8, 128
    x, q = rnd(B, HW, D, seed=31).to(dev), rnd(B, N, D, seed=32).to(dev)
    pn, pd, _ = ops.slot_attn_iter(x, x, q)
    pns, pds, _ = ops.slot_attn_iter(x, x.clone(), q)
    assert torch.equal(pn[:, 1::2], torch.zeros_like(pn[:, 1::2])) and bool((pns[:, 1::2] != 0).any())
    close(pn.sum(1), pns.sum(1).cpu(), rtol=1e-4, atol=1e-3)
    v = rnd(B, HW, D, seed=33).to(dev)
    pn, pd, _ = ops.slot_attn_iter(x, v, q)
    du = rnd(B, N, D, seed=34).to(dev)
    dq8, dk8, dv8 = ops.slot_attn_iter_bwd(x, v, q, pn, pd, du)          # (N <= 8: sf_slot_attn_iter_bwd_f32)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(x), torch.empty_like(v)
    nb = lib().sf_slot_attn_iter_bwd16_workspace_bytes(B, HW, N, D)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    check(lib().sf_slot_attn_iter_bwd16_f32(x.data_ptr(), v.data_ptr(), D, HW * D, q.data_ptr(), pn.data_ptr(), pd.data_ptr(), pn.shape[1], du.data_ptr(),
                                            dk.data_ptr(), dv.data_ptr(), 0, dq.data_ptr(), B, HW, N, D, D**-0.5, 1e-6, ws.data_ptr(), nb,
                                            torch.cuda.current_stream().cuda_stream))
    assert torch.equal(dq, dq8) and torch.equal(dk, dk8) and torch.equal(dv, dv8)


# ---------------------------------------------------------------------------------------------------------------------------
# backward and training
@pytest.mark.parametrize('B,HW,N,D', [(2, 256, 9, 128), (1, 1024, 16, 256), (2, 256, 11, 192), (2, 512, 16, 64)])
def test_iteration_backward(dev, B, HW, N, D):
    """sf_slot_attn_iter_bwd16_f32 (two launches that share the softmax) against autograd of the oracle's attention half, with the
    accumulate-into-dk/dv second call: tests/test_train_gpu.py's test at 9 .. 16 slots."""
    ttg.test_slot_attention_iteration_backward(dev, B, HW, N, D)


def test_iteration_backward_is_deterministic(dev):
    from slotformer_amd import ops
    B, HW, N, D = 2, 512, 13, 128
    k, v, q, du = (rnd(*s, seed=i).to(dev) for i, s in enumerate([(B, HW, D), (B, HW, D), (B, N, D), (B, N, D)]))
    pn, pd, _ = ops.slot_attn_iter(k, v, q)
    a, b = ops.slot_attn_iter_bwd(k, v, q, pn, pd, du), ops.slot_attn_iter_bwd(k, v, q, pn, pd, du)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_module_backward(dev, precision):
    """SlotAttention under autograd at 11 slots (sf_slot_attention_train_*): tests/test_train_gpu.py's test, L2TOL[precision]."""
    ttg.test_slot_attention_module_backward(dev, precision, 2, 1024, 11, 128, 128, 256, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# whole models
@pytest.mark.parametrize('name', list(sc.SAVI_CASES))
def test_savi_golden(dev, name):
    """savi_n9 (Transformer + LSTM predictor: the unfused predictor chain beyond 8 slots, 3 iterations), savi_n11 (the C2 form: one-launch slot
    prologue, NEXT-form slot update, folded keys == values -> the tile kernel at 16-slot width), savi_n16 (the C1 form): as test_savi_golden."""
    cfg, kw = sc.SAVI_CASES[name]
    teg.test_savi_golden(dev, name, cfg, kw['B'], kw['T'], kw['seed'], kw.get('noise_seed'))


@pytest.mark.parametrize('name', list(sc.ROLL_CASES))
def test_rollout_golden(dev, name):
    cfg, kw = sc.ROLL_CASES[name]
    teg.test_rollout_golden(dev, name, cfg, kw['B'], kw['pred_len'], kw['seed'])


@pytest.mark.parametrize('name', list(sc.SAVI_TRAIN_CASES))
def test_savi_training_step_golden(dev, precision, name):
    cfg, kw = sc.SAVI_TRAIN_CASES[name]
    ttg.test_savi_training_step_golden(dev, precision, name, sc.register(cfg), kw['T'], kw['seed'], kw['noise_seed'])


@torch.no_grad()
def test_predictor_step_beyond_8_slots_is_the_unfused_chain(dev):
    """sf_pred_step_ex declines more than 8 slots and the encode runs the Transformer predictor layer by layer: a second frame (the first one that
    has previous slots) of the 16-slot C1-form model against the oracle, and the 8-slot model of the same form for the fused launch."""
    for N in (16, 8):
        cfg = gu.savi_cfg(64, N)
        torch.manual_seed(3)
        from slotformer_amd.base_slots import build_model
        m = build_model(gu.ParamsView(cfg)).eval()
        m.testing = True
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        img = gu.seeded_img(2, 2, 64, seed=77)
        post = m.to(dev)({'img': img.to(dev)})['post_slots']
        ref = oracle.savi_encode(img, sd, cfg)['post_slots']
        assert teg.rel_err(post, ref) < 5e-5 and teg.elementwise_close(post, ref)


@torch.no_grad()
def test_forward_with_decode_and_boxes_at_11_slots(dev):
    """StoSAVi.forward outside testing mode at 11 slots: encode + decode (the decoder combines up to 16 slots) against the oracle, then the
    segmentation ids and masks_to_boxes over 11 ids (the metrics take 16)."""
    from slotformer_amd.video_prediction import vp_utils as v
    name = 'savi_n11'
    cfg, kw = sc.SAVI_CASES[name]
    g = gu.load_golden(name)
    m, sd = teg.build(cfg, g, kw['seed'], dev)
    B, T, N, D = kw['B'], kw['T'], 11, 128
    img = gu.seeded_img(B, T, 64)
    out = m({'img': img.to(dev), 'noise': gu.seeded_normal((B, T, N, D), kw['noise_seed']).to(dev)})
    assert out['post_recon_combined'].shape == (B, T, 3, 64, 64) and out['post_masks'].shape == (B, T, N, 1, 64, 64)
    assert teg.rel_err(out['post_slots'], g['post_slots']) < 5e-5
    ref_r, ref_recons, ref_masks = oracle.savi_decode(torch.as_tensor(g['post_slots']).flatten(0, 1), sd, cfg)
    assert teg.rel_err(out['post_recon_combined'].flatten(0, 1), ref_r) < 5e-4
    assert teg.rel_err(out['post_recons'].flatten(0, 1), ref_recons) < 5e-4
    assert (out['post_masks'].flatten(0, 1).cpu() - ref_masks).abs().max() < 2e-5
    seg = out['post_masks'].argmax(2).squeeze(2)                          # [B, T, 64, 64] ids 0..10
    top2 = ref_masks.squeeze(2).topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-4                               # away from ties, the ids are the oracle's
    assert torch.equal(seg.flatten(0, 1).cpu()[sure], ref_masks.squeeze(2).argmax(1)[sure])
    for ids in (seg, (seg + 5) % N):                                      # (the second: ids 8, 9 and 10 certainly own pixels)
        boxes = v.masks_to_boxes(ids, N)
        assert boxes.shape == (B, T, N, 4) and torch.equal(boxes.cpu(), v.masks_to_boxes(ids.cpu(), N))


# ---------------------------------------------------------------------------------------------------------------------------
# pipeline and harness
@pytest.mark.parametrize('N', [11, 16])
def test_pipeline_matches_serial(dev, N):
    """Four batches of 4 videos through EncodeRolloutPipeline against the serial module calls, as tests/test_pipeline_gpu.py holds the 7-slot
    pipeline: bit for bit (4 videos per batch: no token-stationary units), the serial schedule of the same graphs too, and reproducible."""
    from slotformer_amd.pipeline import EncodeRolloutPipeline, unit_batches_for, tok_unit_batches
    B, T, H, nbatch = 4, 6, 4, 4
    savi, roll = tpg._models(dev, gu.savi_cfg(64, N, kernel_mlp=False, pred='mlp', rnn=False, kld='var-0.01'), gu.rollout_cfg(N, 128, 6, 256, 4, 8, 1024))
    rs = np.random.RandomState(7)
    imgs = [torch.from_numpy((rs.rand(B, T, 3, 64, 64) * 2 - 1).astype(np.float32)).to(dev) for _ in range(nbatch)]
    noises = [torch.from_numpy(rs.standard_normal((B, T, N, 128)).astype(np.float32)).to(dev) for _ in range(nbatch)]
    with torch.no_grad():
        ref = tpg._serial_reference(savi, roll, imgs, noises, T, H, tpg.PAIR_OPTS)
        assert torch.equal(ref[:2], tpg._serial_reference(savi, roll, imgs[:2], noises[:2], T, H))
        pipe = EncodeRolloutPipeline(savi, roll, B, T, H)
        assert not pipe.tok and pipe.bufs[0].shape == (pipe.G * B, T + H, N, 128)
        out = pipe.run(imgs, noises)
        torch.cuda.synchronize()
        out3 = pipe.run(imgs, noises, serial=True)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), (out - ref).abs().max().item()
        assert torch.equal(out3, ref)
        assert not torch.equal(out[0], out[1])
        out2 = pipe.run(imgs, noises)
        torch.cuda.synchronize()
        assert torch.equal(out2, out)
        pipe.close()
    # the unit plan on the device: within one round of row tiles; token-stationary units only where a 128-token workgroup holds a whole video
    for batch, n in ((4, 40), (32, 20), (32, 100), (2, 40)):
        g = unit_batches_for(roll, batch, n, T)
        gt = tok_unit_batches(roll, batch, T, n)
        assert g is None or gt == g or (5 <= g <= n and g * batch * N * T <= 8192)
        assert gt is None or (N * T <= 96 and 1 <= gt <= 8 and gt * batch >= 96)


@torch.no_grad()
def test_extract_and_rollout_at_16_slots(dev):
    """harness.extract_and_rollout with 16-slot models: 4 full batches of 2 videos through the pipeline + a ragged last video, against the serial
    module calls."""
    from slotformer_amd import harness, engine
    N, B, T, H = 16, 2, 6, 3
    savi, roll = tpg._models(dev, gu.savi_cfg(64, N, kernel_mlp=False, pred='mlp', rnn=False, kld='var-0.01'), gu.rollout_cfg(N, 128, 6, 256, 4, 8, 1024), seed=2)
    rs = np.random.RandomState(9)
    V = 4 * B + 1
    vids = torch.from_numpy((rs.rand(V, T, 3, 64, 64) * 2 - 1).astype(np.float32)).to(dev)
    nz = torch.from_numpy(rs.standard_normal((V, T, N, 128)).astype(np.float32)).to(dev)
    out = harness.extract_and_rollout(savi, roll, vids, H, batch_size=B, noises=nz)
    assert out.shape == (V, T + H, N, 128)
    post = savi({'img': vids, 'noise': nz})['post_slots']
    ref = torch.zeros(V, T + H, N, 128, device=dev)
    ref[:, :T] = post
    engine.rollout(roll, ref, T, H)
    assert tpg._close(out, ref) and torch.equal(out[:, :T], ref[:, :T])
