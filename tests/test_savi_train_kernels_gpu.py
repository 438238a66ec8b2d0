"""GPU: the launches behind SAVi's two convolutional backward passes (csrc/savi_features_train.hip, csrc/savi_decode_train.hip) against float64, one
library call at a time, on the cases of tests/savi_train_kernel_cases.py -- every kernel form, row split and arithmetic mode the host code can pick --
and one decoder small enough to be free of ReLU kinks through the whole module path.

Every comparison is element by element in the close() form of tests/test_train_kernels_gpu.py, |a - b| <= rtol |b| + floor max |b|, at the bounds of
savi_train_kernel_cases.BOUNDS per form and arithmetic mode -- that file's bounds, tightened to about twice what the MI355X measured (the `precision`
fixture: split-bf16 and f32; mode 2, the single bf16 product, set and restored inside the test).  Outputs
and workspaces are NaN-filled before a call and carry NaN guards behind them; operands carry NaN rows past their last row."""
import copy
from contextlib import contextmanager

import pytest
import torch

import decode_cases as dc
import savi_train_kernel_cases as sc
from test_train_kernels_gpu import close

pytestmark = pytest.mark.gpu

GUARD = 256                  # floats of NaN behind every output and workspace, rows of NaN behind every operand
NAN_BITS = 0x7fc00000        # what torch.full(.., nan) writes


def _lib():
    from slotformer_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return _lib().sf_last_error_string().decode()


@contextmanager
def single_pass_bf16():
    lib = _lib()
    old = lib.sf_get_precision()
    lib.sf_set_precision(2)
    try:
        yield 'bf16'
    finally:
        lib.sf_set_precision(old)


def nan_buffer(n, dev):
    return torch.full((n + GUARD, ), float('nan'), device=dev)


def guarded(t, dev):
    """the rows of t [rows, C] on the device with GUARD rows of NaN behind them"""
    rows, C_ = t.shape
    buf = torch.full((rows + GUARD, C_), float('nan'), device=dev)
    buf[:rows] = t.to(dev)
    return buf


def guard_intact(buf, n):
    return bool((buf.view(-1)[n:].view(torch.int32) == NAN_BITS).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# weight gradient: sf_conv_wgrad_f32
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def wgrad_run(dev, a, x, s):
    """one call on NaN-guarded buffers with exactly the partial floats the call's splits need; returns dW [CA,64,5,5] on the device after checking that
    everything the reduction reads was written (empty splits: zeros), that the result is finite and that no guard was touched"""
    F_, H, W, CA = a.shape
    rows, n_out = F_ * H * W, CA * 1600
    _, splits, rps, empty = sc.wgrad_plan(F_, H, W, s, CA)
    need = splits * n_out
    ab, xb = guarded(a.reshape(rows, CA), dev), guarded(x.reshape(-1, 64), dev)
    pb, ob = nan_buffer(need, dev), nan_buffer(n_out, dev)
    rc = _lib().sf_conv_wgrad_f32(ab.data_ptr(), CA, F_, H, W, xb.data_ptr(), H * s, W * s, s, 5, rows, ob.data_ptr(), pb.data_ptr(), need, _stream())
    assert rc == 0, _err()
    assert torch.isfinite(pb[:need]).all(), 'a partial the reduction reads was not written'
    if empty:
        assert (pb[(splits - empty) * n_out:need] == 0).all(), 'an empty split did not write zeros'
    assert torch.isfinite(ob[:n_out]).all()
    assert guard_intact(pb, need) and guard_intact(ob, n_out), 'a write past the end of partial / dW'
    assert guard_intact(ab, rows * CA) and guard_intact(xb, x.numel())
    return ob[:n_out].view(CA, 64, 5, 5)


def wgrad_check(dev, name, tol, what):
    a, x = sc.wgrad_inputs(name)
    s = sc.WGRAD_CASES[name][3]
    out = wgrad_run(dev, a, x, s)
    ratio = close(out, sc.wgrad_reference(name), tol, f'wgrad {name} {what}')
    assert torch.equal(bits(wgrad_run(dev, a, x, s)), bits(out)), 'a second call gave other bits'
    return out, ratio


@pytest.mark.parametrize('name', sc.WGRAD_NAMES)
def test_wgrad_vs_float64(dev, precision, name):
    wgrad_check(dev, name, sc.BOUNDS['wgrad'][precision], precision)


@pytest.mark.parametrize('name', sc.WGRAD_NAMES)
def test_wgrad_single_pass_bf16(dev, name):
    with single_pass_bf16() as what:
        out, _ = wgrad_check(dev, name, sc.BOUNDS['wgrad'][what], what)
    # and mode 2 is really the single product: outside the split-bf16 bound (every case: tests/test_savi_train_kernel_cases.py)
    ref = sc.wgrad_reference(name)
    assert sc.err_over_bound(out, ref, sc.BOUNDS['wgrad']['bf16x3']) > 1.0


@pytest.mark.parametrize('name', sc.WGRAD_NAMES)
def test_wgrad_onehot_is_exact(dev, precision, name):
    """a single 1 in A (at each corner and one interior pixel) against a single 1 in X: one exact 1 at a known [n][k][ky][kx], exact +0.0 elsewhere"""
    F_, H, W, s, CA = sc.WGRAD_CASES[name][:5]
    for i in range(len(sc.onehot_pixels(H, W))):
        a, x = sc.onehot_tensors(name, i)
        out = wgrad_run(dev, a, x, s)
        exp = sc.onehot_expected(name, i)
        if not torch.equal(bits(out), bits(exp)):
            got = out.cpu()
            nz = got.nonzero().tolist()
            raise AssertionError(f'{name} pixel {sc.onehot_case(name, i)}: non-zeros at {nz[:8]} ({len(nz)}), values {[got[tuple(j)].item() for j in nz[:8]]}')


FRAME_CASES = [n for n in sc.WGRAD_NAMES if 2 <= sc.WGRAD_CASES[n][0] <= 3]


@pytest.mark.parametrize('name', FRAME_CASES)
def test_wgrad_frame_contributions_survive_a_permutation(dev, precision, name):
    """with every other frame of A zeroed, frame f contributes its own float64 gradient wherever it stands in the row order (the position moves it
    across other row splits and chunks)"""
    a, x = sc.wgrad_inputs(name)
    F_, s = a.shape[0], sc.WGRAD_CASES[name][3]
    perm = list(range(1, F_)) + [0]
    for f in range(F_):
        ref = sc.wgrad_frame_reference(name, f)
        for order in (list(range(F_)), perm):
            az = torch.zeros_like(a)
            pos = order.index(f)
            az[pos] = a[f]
            close(wgrad_run(dev, az, x[order].contiguous(), s), ref, sc.BOUNDS['wgrad'][precision], f'wgrad {name} frame {f} at {pos}')


def test_wgrad_wrapper_allocates_the_documented_partial(dev, precision):
    from slotformer_amd import ops
    a, x = sc.wgrad_inputs('g_8x8_s2_ca128')
    out = ops.conv_wgrad(a.to(dev), x.to(dev), stride=2)
    close(out, sc.wgrad_reference('g_8x8_s2_ca128'), sc.BOUNDS['wgrad'][precision], 'ops.conv_wgrad')


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# masked data gradient: sf_conv2d_nhwc_bwd_data_f32, sf_pack_conv_bwd_weight_f32, relu = 2 of sf_conv2d_nhwc_f32 / sf_conv5x5_frag_f32
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def dgrad_packed_on_device(dev, name):
    from slotformer_amd import ops
    _, w, _ = sc.dgrad_inputs(name)
    route = sc.DGRAD_CASES[name][6]
    wp = ops.pack_conv_bwd_weight(w.to(dev)) if route == 'conv' else ops.pack_conv_weight(w.to(dev))
    assert torch.equal(bits(wp), bits(sc.dgrad_packed(w, route)))
    return wp


def dgrad_run(dev, name, wp):
    F_, Hin, Win, s, Cin, Cout, _, _ = sc.DGRAD_CASES[name]
    g, _, mask = sc.dgrad_inputs(name)
    n_out = F_ * (Hin // s) * (Win // s) * Cout
    gb = guarded(g.reshape(-1, Cin), dev)
    mb = guarded(mask.reshape(-1, Cout), dev) if mask is not None else None
    ob = nan_buffer(n_out, dev)
    rc = _lib().sf_conv2d_nhwc_bwd_data_f32(gb.data_ptr(), wp.data_ptr(), mb.data_ptr() if mb is not None else None, ob.data_ptr(), F_, Hin, Win, Cin,
                                            Cout, 5, s, _stream())
    assert rc == 0, _err()
    assert guard_intact(ob, n_out) and torch.isfinite(ob[:n_out]).all()
    return ob[:n_out].view(F_, Hin // s, Win // s, Cout)


def dgrad_check(dev, name, tol, what):
    from slotformer_amd import ops
    g, _, mask = sc.dgrad_inputs(name)
    ref = sc.dgrad_reference(name)
    wp = dgrad_packed_on_device(dev, name)
    out = dgrad_run(dev, name, wp)
    close(out, ref, tol, f'dgrad {name} {what} ({sc.dgrad_form(name, what)})')
    if mask is not None:
        assert (out.cpu()[~(mask > 0)] == 0).all(), 'a masked output is not zero'
    assert torch.equal(bits(dgrad_run(dev, name, wp)), bits(out))
    if sc.DGRAD_CASES[name][3] == 1 and mask is not None:      # the public relu = 2 of sf_conv2d_nhwc_f32 is this call
        assert torch.equal(bits(ops.conv2d_nhwc(g.to(dev), wp, None, relu=2, add=mask.to(dev))), bits(out))
    return out, wp


@pytest.mark.parametrize('name', sc.DGRAD_NAMES)
def test_dgrad_vs_float64(dev, precision, name):
    from slotformer_amd import ops
    out, wp = dgrad_check(dev, name, sc.BOUNDS['dgrad'][precision], precision)
    if precision == 'bf16x3' and sc.dgrad_rows4(name):
        # the 4-row-tile kernel on the fragment copy of the same weights: against float64, and bit-identical to the halo kernel as in the forward
        g, _, mask = sc.dgrad_inputs(name)
        assert sc.dgrad_form(name, precision) == 'halo'
        out4 = ops.conv5x5_frag(g.to(dev), ops.pack_conv_frag(wp), None, relu=2, add=mask.to(dev))
        close(out4, sc.dgrad_reference(name), sc.BOUNDS['dgrad'][precision], f'dgrad {name} rows4')
        assert (out4.cpu()[~(mask > 0)] == 0).all()
        assert torch.equal(bits(out4), bits(out)), 'rows4 and halo differ with relu = 2'


@pytest.mark.parametrize('name', sc.DGRAD_NAMES)
def test_dgrad_single_pass_bf16(dev, name):
    with single_pass_bf16() as what:
        out, _ = dgrad_check(dev, name, sc.BOUNDS['dgrad'][what], what)
    assert sc.err_over_bound(out, sc.dgrad_reference(name), sc.BOUNDS['dgrad']['bf16x3']) > 1.0


@pytest.mark.parametrize('Cout,Cin,ks', [(64, 64, 5), (3, 5, 3), (7, 2, 1), (128, 64, 5)])
def test_pack_conv_bwd_weight(dev, Cout, Cin, ks):
    from slotformer_amd import ops
    w = sc.rnd(Cout, Cin, ks, ks, seed=Cout + Cin)
    got = ops.pack_conv_bwd_weight(w.to(dev))
    assert got.shape == (Cin, ks, ks, Cout) and torch.equal(bits(got), bits(w.flip(2, 3).permute(1, 2, 3, 0).contiguous()))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# conv0's weight gradient: sf_conv_first_wgrad_f32
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def first_check(dev, name, tol, what):
    F_, res, gap = sc.FIRST_CASES[name]
    img, dy = sc.first_inputs(name)
    stride = 3 * res * res + gap
    ib = torch.full((F_ * stride + GUARD, ), float('nan'), device=dev)
    for f in range(F_):
        ib[f * stride:f * stride + 3 * res * res] = img[f].reshape(-1).to(dev)
    db, ob = guarded(dy, dev), nan_buffer(64 * 75, dev)
    nb = _lib().sf_conv_first_wgrad_workspace_bytes(F_)
    ws = torch.full((nb // 4 + GUARD, ), float('nan'), device=dev)
    rc = _lib().sf_conv_first_wgrad_f32(ib.data_ptr(), stride, res, db.data_ptr(), F_, ob.data_ptr(), ws.data_ptr(), nb, _stream())
    assert rc == 0, _err()
    assert guard_intact(ob, 64 * 75) and guard_intact(ws, nb // 4)
    close(ob[:64 * 75].view(64, 3, 5, 5), sc.first_closed(img, dy), tol, f'conv0 wgrad {name} {what}')
    return ob[:64 * 75].view(64, 3, 5, 5)


@pytest.mark.parametrize('name', list(sc.FIRST_CASES))
def test_first_wgrad_vs_float64(dev, precision, name):
    from slotformer_amd import ops
    out = first_check(dev, name, sc.BOUNDS['first'][precision], precision)
    if sc.FIRST_CASES[name][2] == 0:
        img, dy = sc.first_inputs(name)
        assert torch.equal(bits(ops.conv_first_wgrad(img.to(dev), dy.to(dev))), bits(out))


@pytest.mark.parametrize('name', list(sc.FIRST_CASES))
def test_first_wgrad_single_pass_bf16(dev, name):
    with single_pass_bf16() as what:
        out = first_check(dev, name, sc.BOUNDS['first'][what], what)
    img, dy = sc.first_inputs(name)
    assert sc.err_over_bound(out, sc.first_closed(img, dy), sc.BOUNDS['first']['bf16x3']) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# position embedding: sf_pos_dense_grad_f32 (float32 sums in every mode)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F_,HW,C_', sc.POS_CASES)
def test_pos_dense_grad_vs_float64(dev, F_, HW, C_):
    d, grid = sc.pos_inputs(F_, HW, C_)
    rw, rb, rtab = sc.pos_reference(d, grid)
    dbuf, gbuf = guarded(d.reshape(F_ * HW, C_), dev), guarded(grid, dev)
    wb, bb, tb = nan_buffer(C_ * 4, dev), nan_buffer(C_, dev), nan_buffer(HW * C_, dev)
    rc = _lib().sf_pos_dense_grad_f32(dbuf.data_ptr(), F_, HW, C_, gbuf.data_ptr(), wb.data_ptr(), bb.data_ptr(), tb.data_ptr(), _stream())
    assert rc == 0, _err()
    assert guard_intact(wb, C_ * 4) and guard_intact(bb, C_) and guard_intact(tb, HW * C_)
    what = f'pos ({F_}, {HW}, {C_})'
    close(tb[:HW * C_].view(HW, C_), rtab, sc.BOUNDS['pos'], what + ' frame sum')
    close(wb[:C_ * 4].view(C_, 4), rw, sc.BOUNDS['pos'], what + ' dw')
    close(bb[:C_], rb, sc.BOUNDS['pos'], what + ' db')


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# head block of the decoder: sf_savi_decode_head_bwd_f32
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def head_run(dev, name, params=True):
    F_, N, HW, Cl, _ = sc.HEAD_CASES[name]
    dec, d_recon, act, out_w = sc.head_inputs(name)
    rows = F_ * N * HW
    decb, actb = guarded(dec.reshape(rows, 4), dev), guarded(act, dev)
    drb, owb = d_recon.to(dev), out_w.to(dev)
    ddb, dab = nan_buffer(rows * 4, dev), nan_buffer(rows * Cl, dev)
    gwb, gbb = nan_buffer(4 * Cl, dev), nan_buffer(4, dev)
    nb = _lib().sf_savi_decode_head_bwd_workspace_bytes(Cl)
    ws = torch.full((nb // 4 + GUARD, ), float('nan'), device=dev)
    rc = _lib().sf_savi_decode_head_bwd_f32(decb.data_ptr(), drb.data_ptr(), actb.data_ptr(), owb.data_ptr(), ddb.data_ptr(),
                                            dab.data_ptr(), gwb.data_ptr() if params else None, gbb.data_ptr() if params else None, F_, N, HW, Cl,
                                            ws.data_ptr(), nb, _stream())
    assert rc == 0, _err()
    torch.cuda.synchronize()
    for b, n in ((ddb, rows * 4), (dab, rows * Cl), (ws, nb // 4)) + (((gwb, 4 * Cl), (gbb, 4)) if params else ()):
        assert guard_intact(b, n)
    return ddb[:rows * 4].view(F_, N, HW, 4), dab[:rows * Cl].view(rows, Cl), gwb[:4 * Cl].view(4, Cl), gbb[:4]


def head_check(dev, name, tol, what):
    F_, N, HW, Cl, _ = sc.HEAD_CASES[name]
    dec, d_recon, act, out_w = sc.head_inputs(name)
    d_dec, d_act, gw, gb = head_run(dev, name)
    ref = sc.head_d_dec_closed(dec, d_recon)
    what = f'head {name} {what}'
    close(d_dec, ref, sc.BOUNDS['head_f32'], what + ' d_dec')          # float32 element-wise arithmetic in every mode
    if N == 1:
        assert (d_dec[..., 3] == 0).all(), 'one slot: the mask-logit gradient is exactly zero'
    rw, rb = sc.head_param_grads(ref, act)
    close(gw, rw, sc.BOUNDS['head_f32'], what + ' d_out_w')
    close(gb, rb, sc.BOUNDS['head_f32'], what + ' d_out_b')
    # the masked K = 4 GEMM, as one launch: against the float64 product of the d_dec it was given
    close(d_act, sc.head_d_act(d_dec.cpu(), act, out_w), tol, what + ' d_act')
    assert (d_act.cpu()[~(act > 0)] == 0).all()
    d2, a2, _, _ = head_run(dev, name, params=False)        # no parameter gradients: the same d_dec and d_act
    assert torch.equal(bits(d2), bits(d_dec)) and torch.equal(bits(a2), bits(d_act))
    return d_act


@pytest.mark.parametrize('name', sc.HEAD_NAMES)
def test_head_bwd_vs_float64(dev, precision, name):
    head_check(dev, name, sc.BOUNDS['head_act'][precision], precision)


@pytest.mark.parametrize('name', sc.HEAD_NAMES)
def test_head_bwd_single_pass_bf16(dev, name):
    with single_pass_bf16() as what:
        head_check(dev, name, sc.BOUNDS['head_act'][what], what)


def test_head_bwd_wrapper_is_the_direct_call(dev):
    """ops.savi_decode_head_bwd, whose workspace comes from _call.scratch, on the smallest case: bit for bit what the entry point gives when it is
    called directly with a workspace of the queried size.  The same library and no atomics in it, so equality is the bar."""
    from slotformer_amd import ops
    dec, d_recon, act, out_w = (t.to(dev).contiguous() for t in sc.head_inputs('n1'))
    for params in (True, False):
        got = ops.savi_decode_head_bwd(dec, d_recon, act, out_w, want_param_grads=params)
        want = head_run(dev, 'n1', params)[:4 if params else 2]
        assert all(torch.equal(bits(g), bits(w)) for g, w in zip(got, want))
        assert params or got[2:] == (None, None)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# module wiring: StoSAVi.decode under autograd on decode_cases.TRAIN_CASE (split-bf16 and f32: the margin that keeps the ReLUs off their kinks is
# sized for those, not for the 2^-8 of mode 2)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def module_run(dev, trained):
    m = copy.deepcopy(dc.train_case()[0]).to(dev)
    m.train()
    if not trained:
        for p in list(m.decoder.parameters()) + list(m.decoder_pos_embedding.parameters()):
            p.requires_grad_(False)
    sg = dc.train_case()[3].to(dev).requires_grad_(True)
    recon = m.decode(sg)[0]
    recon.backward(sc.module_d_recon().to(dev))
    return m, recon.detach(), sg.grad


@pytest.mark.parametrize('trained', [False, True], ids=['frozen', 'trained'])
def test_decoder_module_gradients_element_by_element(dev, precision, trained):
    ref = sc.module_reference()
    m, recon, d_slots = module_run(dev, trained)
    e = ((recon.cpu().double() - ref['recon']).abs().max() / ref['recon'].abs().max()).item()
    print(f'module {precision} recon: max err / max |ref| {e:.2e} (bound {sc.MODULE_RECON_BOUND:.0e})')
    assert e < sc.MODULE_RECON_BOUND
    tol = sc.BOUNDS['module'][precision]
    what = f'module {precision} {"trained" if trained else "frozen"}'
    close(d_slots, ref['d_slots'], tol, what + ' d_slots')
    got = dict(m.named_parameters())
    names = sc.module_param_names()
    assert len(names) == 10
    for n in names:
        if trained:
            assert got[n].grad is not None, n
            close(got[n].grad, ref['grads'][n], tol, f'{what} {n}')
        else:
            assert got[n].grad is None, n
