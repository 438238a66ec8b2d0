"""CPU: the case tables of tests/savi_train_kernel_cases.py say what they claim -- which kernel and which row splits a weight-gradient call takes, two
independent float64 references that agree, bounds that the split-bf16 arithmetic fits with room and the single-bf16 arithmetic breaks, a decoder whose
float64 forward has no ReLU near its kink -- and the new entry points refuse what they cannot compute before touching a device.

What this cannot do: tell arithmetic mode 0 (four split products) from mode 1 (three).  They differ by about 2^-18 of a product, far below any bound a
kernel meets against float64; only bit-level tests of the kernels could, and there is none here."""
import ctypes as C

import pytest
import torch

import decode_cases as dc
import savi_train_kernel_cases as sc
from savi_train_kernel_cases import err_over_bound


def split_bound(form):
    """what the GPU test asserts of `form` in split-bf16 mode"""
    return sc.BOUNDS[form]['bf16x3']


def test_bounds_start_from_those_of_the_training_kernel_tests_and_only_tighten():
    import test_train_kernels_gpu as tk
    assert sc.TOL == tk.TOL and sc.TOL_BF16 == tk.TOL_BF16
    assert sc.module_chain() == 5
    for form, b in sc.BOUNDS.items():
        if form == 'module':
            assert all(b[m][0] <= sc.module_chain() * sc.TOL[m][0] and b[m][1] == b[m][0] for m in b)
        elif isinstance(b, dict):
            assert set(b) == {'f32', 'bf16x3', 'bf16'}
            assert all(2**-23 <= b[m][0] <= sc.PROJECT[m][0] and b[m][1] <= sc.PROJECT[m][1] for m in b), form
        else:
            assert 2**-23 <= b[0] <= sc.TOL['f32'][0] and b[1] <= sc.TOL['f32'][1], form


# ---- weight gradient ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sc.WGRAD_NAMES)
def test_wgrad_plan_is_what_the_table_claims(name):
    F_, H, W, s, CA, form, splits, rps, empty = sc.WGRAD_CASES[name]
    assert sc.wgrad_plan(F_, H, W, s, CA) == (form, splits, rps, empty)
    assert splits <= sc.PARTIAL_SPLITS_MAX and sc.wgrad_partial_floats(F_, H, W, s, CA) == splits * CA * 1600
    assert rps % 32 == 0 and (splits - empty - 1) * rps < F_ * H * W <= (splits - empty) * rps
    assert (form != 'generic') == (W % 32 == 0 and s in (1, 2))


def test_wgrad_table_reaches_every_form_and_edge():
    forms = {c[5] for c in sc.WGRAD_CASES.values()}
    assert forms == {'generic', 'win1', 'win2'}
    assert any(c[5] == 'generic' and c[3] == 1 for c in sc.WGRAD_CASES.values())          # the branch no reference workload takes
    assert any(c[8] > 0 for c in sc.WGRAD_CASES.values())                                   # empty trailing splits
    assert any(c[4] == 128 for c in sc.WGRAD_CASES.values())                                # two n tiles
    assert any((c[0] * c[1] * c[2]) % 32 for c in sc.WGRAD_CASES.values())                  # a ragged last chunk


@pytest.mark.parametrize('name', sc.WGRAD_NAMES)
def test_wgrad_references_agree_and_bounds_bite(name):
    a, x = sc.wgrad_inputs(name)
    s = sc.WGRAD_CASES[name][3]
    ref = sc.wgrad_reference(name)
    scale = ref.abs().max().item()
    assert (sc.wgrad_autograd(a, x, s) - ref).abs().max().item() <= 1e-12 * scale
    if s == 1:
        assert (sc.wgrad_autograd_conv(a, x) - ref).abs().max().item() <= 1e-12 * scale
    split = err_over_bound(sc.wgrad_closed(a, x, s, 'split'), ref, split_bound('wgrad'))
    single = err_over_bound(sc.wgrad_closed(a, x, s, 'single'), ref, split_bound('wgrad'))
    print(f'{name}: split {split:.4f} single {single:.1f} of the split-bf16 bound; single {err_over_bound(sc.wgrad_closed(a, x, s, "single"), ref, sc.BOUNDS["wgrad"]["bf16"]):.3f}'
          ' of the mode-2 bound')
    assert split <= 0.5
    assert single > 1.0            # a split-bf16 mode that launched the single-pass kernel fails every case


@pytest.mark.parametrize('name', [n for n in sc.WGRAD_NAMES if sc.WGRAD_CASES[n][0] * sc.WGRAD_CASES[n][1] * sc.WGRAD_CASES[n][2] <= 2048])
def test_wgrad_onehot_expectation_is_the_closed_form(name):
    F_, H, W, s, CA = sc.WGRAD_CASES[name][:5]
    pixels = sc.onehot_pixels(H, W)
    assert len(pixels) == (1 if H * W == 1 else 5 + (W > 32) if min(H, W) > 2 else len(pixels))
    if W > 32:
        assert sc.onehot_case(name, len(pixels) - 1)[2][3] == 4 and sc.onehot_case(name, len(pixels) - 1)[0][2] == 31
    taps = set()
    for i in range(len(pixels)):
        a, x = sc.onehot_tensors(name, i)
        got = sc.wgrad_closed(a, x, s)
        assert torch.equal(got, sc.onehot_expected(name, i).double()) and got.sum().item() == 1.
        taps.add(sc.onehot_case(name, i)[2][2:])
    if min(H, W) > 2:
        assert len(taps) >= 4, taps      # the corners pull different border taps


# ---- masked data gradient -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sc.DGRAD_NAMES)
def test_dgrad_references_agree_and_bounds_bite(name):
    g, w, mask = sc.dgrad_inputs(name)
    F_, Hin, Win, s, Cin, Cout, route, masked = sc.DGRAD_CASES[name]
    ref = sc.dgrad_reference(name)
    assert ref.shape == (F_, Hin // s, Win // s, Cout)
    assert (sc.dgrad_autograd(g, w, s, route, mask) - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    wp = sc.dgrad_packed(w, route)
    split = err_over_bound(sc.dgrad_closed(g, wp, s, mask, 'split'), ref, split_bound('dgrad'))
    single = err_over_bound(sc.dgrad_closed(g, wp, s, mask, 'single'), ref, split_bound('dgrad'))
    print(f'{name}: split {split:.4f} single {single:.1f} of the split-bf16 bound')
    assert split <= 0.5 and single > 1.0
    if masked:
        off = ~(mask > 0)
        assert 0.6 < off.double().mean().item() < 0.8 and (ref[off] == 0).all()
        assert (mask == 0).any() and (mask[mask == 0].view(torch.int32) < 0).any()        # -0.0 is among the keys
        if F_ > 1:
            assert not torch.equal(mask[0] > 0, mask[1] > 0)                                # a per-frame pattern, not a table


def test_dgrad_table_reaches_every_implementation():
    forms = {(sc.dgrad_form(n, p), p) for n in sc.DGRAD_NAMES for p in ('bf16x3', 'f32', 'bf16')}
    assert {('halo', 'bf16x3'), ('halo', 'bf16'), ('gemm', 'f32'), ('gemm', 'bf16x3'), ('gemm', 'bf16')} <= forms
    rows4 = [n for n in sc.DGRAD_NAMES if sc.dgrad_rows4(n)]
    assert {sc.DGRAD_CASES[n][1] for n in rows4} == {4, 8} and {sc.DGRAD_CASES[n][0] for n in rows4} == {1, 3}
    assert any(sc.dgrad_form(n, 'bf16x3') == 'halo' and not sc.dgrad_rows4(n) for n in sc.DGRAD_NAMES)      # H = 2, 6: halo in split-bf16 mode


# ---- conv0, position embedding, head --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(sc.FIRST_CASES))
def test_first_wgrad_references_agree_and_bounds_bite(name):
    img, dy = sc.first_inputs(name)
    ref = sc.first_closed(img, dy)
    assert (sc.first_autograd(img, dy) - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    split, single = (err_over_bound(sc.first_closed(img, dy, m), ref, split_bound('first')) for m in ('split', 'single'))
    print(f'{name}: split {split:.4f} single {single:.1f} of the split-bf16 bound')
    assert split <= 0.5 and single > 1.0


@pytest.mark.parametrize('F_,HW,C_', sc.POS_CASES)
def test_pos_references_agree(F_, HW, C_):
    d, grid = sc.pos_inputs(F_, HW, C_)
    dw, db, tab = sc.pos_reference(d, grid)
    aw, ab = sc.pos_autograd(d, grid)
    assert (aw - dw).abs().max().item() <= 1e-12 * dw.abs().max().item() and (ab - db).abs().max().item() <= 1e-12 * db.abs().max().item()


@pytest.mark.parametrize('name', sc.HEAD_NAMES)
def test_head_references_agree(name):
    dec, d_recon, act, out_w = sc.head_inputs(name)
    F_, N, HW, Cl, gain = sc.HEAD_CASES[name]
    ref = sc.head_d_dec_closed(dec, d_recon)
    assert (sc.head_d_dec_autograd(dec, d_recon) - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    if N == 1:
        assert (ref[..., 3] == 0).all()
    if gain > 1:
        m = torch.softmax(dec[..., 3].double(), 1)
        assert (m.max(1)[0] > 0.999).double().mean().item() > 0.5      # most pixels saturated
    # the K = 4 product behind d_act: the split-bf16 bound tells the arithmetics apart here too
    d32 = ref.float()
    exact = sc.head_d_act(d32, act, out_w)
    split, single = (err_over_bound(sc.head_d_act(d32, act, out_w, m), exact, split_bound('head_act')) for m in ('split', 'single'))
    print(f'{name}: d_act split {split:.4f} single {single:.1f} of the split-bf16 bound')
    assert split <= 0.5 and single > 1.0
    assert (sc.head_rpg(F_, N, HW) > 4) == (name in ('n3_rows2304', 'cl8'))


# ---- the module-level case --------------------------------------------------------------------------------------------------------------------------
def test_train_decoder_has_no_relu_near_its_kink():
    m, sd64, cfg, slots = dc.train_case()
    res, N, D, ch, r, ks, F_ = dc.TRAIN_CASES[dc.TRAIN_CASE]
    pre = dc.train_preactivations(slots.double(), sd64, cfg)
    assert [tuple(z.shape) for z in pre] == [(F_ * N, 64, 4, 4), (F_ * N, 64, 8, 8), (F_ * N, 64, 8, 8)]
    for i, z in enumerate(pre):
        near = (z.abs() <= dc.KINK_MARGIN * z.abs().max()).sum().item()
        on = (z > 0).double().mean((0, 2, 3), keepdim=True)
        minority = torch.where(on > 0.5, z <= 0, z > 0).double().mean().item()
        print(f'layer {i}: {near} of {z.numel()} units within the margin (nearest {(z.abs().min() / z.abs().max()).item():.2e}), minority {minority:.4f}')
        assert near == 0
        assert minority >= dc.MINORITY
    # the module holds the reference's numbers
    own = m.state_dict()
    for k, v in sd64.items():
        if v.dtype.is_floating_point:
            assert torch.equal(own[k].double(), v), k


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    from slotformer_amd import _lib
    lib = _lib.lib()

    def err():
        return lib.sf_last_error_string().decode()

    p = C.c_void_p(4096)        # a non-null, 16-byte-aligned dummy pointer: every case below is refused before it is dereferenced
    odd = C.c_void_p(4100)      # 4-byte aligned only
    big = 1 << 40

    def wgrad(A=p, CA=64, F_=2, H=3, W=5, X=p, Hx=3, Wx=5, s=1, ks=5, rows=30, dW=p, partial=p, pf=big):
        return lib.sf_conv_wgrad_f32(A, CA, F_, H, W, X, Hx, Wx, s, ks, rows, dW, partial, pf, None)

    assert wgrad(ks=3) < 0 and '5x5' in err()
    assert wgrad(CA=96) < 0 and 'multiple of 64' in err()
    assert wgrad(CA=0) < 0
    assert wgrad(rows=31) < 0 and 'rows' in err()
    assert wgrad(Hx=6) < 0 and 'X grid' in err()
    assert wgrad(s=2) < 0 and 'X grid' in err()
    need = sc.wgrad_partial_floats(2, 3, 5, 1, 64)
    assert wgrad(pf=need - 1) < 0 and 'partial buffer too small' in err()
    assert wgrad(F_=3, H=64, W=64, Hx=64, Wx=64, rows=12288, pf=sc.wgrad_partial_floats(3, 64, 64, 1, 64) - 1) < 0 and 'too small' in err()
    for kw in (dict(A=odd), dict(X=odd), dict(partial=odd)):
        assert wgrad(pf=need, **kw) < 0 and '16-byte' in err(), kw
    assert wgrad(A=None) < 0 and 'null' in err()
    assert lib.sf_conv_wgrad_partial_floats(64, 5) == 160 * 64 * 1600 and lib.sf_conv_wgrad_partial_floats(128, 5) == 160 * 128 * 1600
    for c in sc.WGRAD_CASES.values():
        assert sc.wgrad_partial_floats(*c[:5]) <= lib.sf_conv_wgrad_partial_floats(c[4], 5)

    assert lib.sf_conv2d_nhwc_bwd_data_f32(p, p, None, p, 1, 5, 4, 64, 64, 5, 2, None) < 0 and 'strided conv shape' in err()     # Hin % stride
    assert lib.sf_conv2d_nhwc_bwd_data_f32(p, p, None, p, 1, 4, 4, 6, 64, 5, 2, None) < 0                                      # Cin % 4
    assert lib.sf_conv2d_nhwc_bwd_data_f32(None, p, None, p, 1, 4, 4, 64, 64, 5, 2, None) < 0 and 'null' in err()
    assert lib.sf_pack_conv_bwd_weight_f32(None, p, 64, 64, 5, None) < 0 and 'null' in err()
    assert lib.sf_pack_conv_bwd_weight_f32(p, p, 0, 64, 5, None) < 0 and 'bad shape' in err()

    assert lib.sf_conv_first_wgrad_workspace_bytes(0) == 0 and lib.sf_conv_first_wgrad_workspace_bytes(1) >= 4096 * 128 * 4
    assert lib.sf_conv_first_wgrad_f32(p, 3 * 96 * 96, 96, p, 1, p, p, big, None) < 0 and 'resolution' in err()
    assert lib.sf_conv_first_wgrad_f32(p, 3 * 64 * 64 - 1, 64, p, 1, p, p, big, None) < 0 and 'frame_stride' in err()
    assert lib.sf_conv_first_wgrad_f32(p, 3 * 64 * 64, 64, p, 1, p, p, lib.sf_conv_first_wgrad_workspace_bytes(1) - 1, None) < 0 and 'workspace' in err()
    assert lib.sf_conv_first_wgrad_f32(p, 3 * 64 * 64, 64, odd, 1, p, p, big, None) < 0 and '16-byte' in err()
    assert lib.sf_conv_first_wgrad_f32(p, 3 * 64 * 64, 64, p, 1, None, p, big, None) < 0 and 'null' in err()

    assert lib.sf_pos_dense_grad_f32(p, 0, 4, 64, p, p, p, p, None) < 0 and 'bad shape' in err()
    assert lib.sf_pos_dense_grad_f32(p, 1, 4, 64, p, p, p, None, None) < 0 and 'null' in err()

    def head(Cl=64, ws_bytes=big, dec=p, act=p, d_dec=p, F_=1):
        return lib.sf_savi_decode_head_bwd_f32(dec, p, act, p, d_dec, p, None, None, F_, 2, 16, Cl, p, ws_bytes, None)

    assert head(Cl=128) < 0 and 'at most 64' in err()
    assert head(Cl=6) < 0 and 'multiple of 4' in err()
    assert head(F_=0) < 0 and 'bad shape' in err()
    assert head(dec=odd) < 0 and '16-byte' in err()
    assert lib.sf_savi_decode_head_bwd_workspace_bytes(128) == 0 and lib.sf_savi_decode_head_bwd_workspace_bytes(64) > 0
    assert head(ws_bytes=lib.sf_savi_decode_head_bwd_workspace_bytes(64) - 1) < 0 and 'workspace' in err()
