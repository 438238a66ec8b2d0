"""CPU: the case table of tests/gemm_cases.py covers the tile rule of csrc/gemm.hip, and every bound tests/test_gemm_gpu.py holds a launch to is
neither unreachable nor vacuous.  For every case, the float64 reference evaluated in the arithmetic of the kernel's products (operands as bf16
hi + lo, the lo.lo term dropped) sits within HALF of the split-bf16 bound, the same evaluation without the lo operands breaks that bound and sits
within half of the single-pass bound, and the float32 evaluation sits within half of the exact-f32 bound.  This measures the references and the
bounds, never a kernel; the entry points' argument checks at the end run before any device work.

No case is exempt.  The one that could have been is (1, 1, 4) with a ReLU: were its single output clipped, the result would be the same in any
arithmetic; gemm_cases.linear_inputs draws it positive, and test_linear_bounds holds it to that.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as gc


def name(case):
    return 'x'.join(str(v) for v in case)


def _lib():
    from slotformer_amd._lib import lib
    return lib()


def _err():
    return _lib().sf_last_error_string().decode()


def bounds_hold(what, ref, split, single, f32):
    s = gc.err_over_bound(split, ref, gc.TOL['bf16x3'])
    g = gc.err_over_bound(single, ref, gc.TOL['bf16x3'])
    h = gc.err_over_bound(single, ref, gc.TOL_BF16)
    e = gc.err_over_bound(f32, ref, gc.TOL['f32'])
    print(f'gemm_cpu {what}: split {s:.3f}, single {g:.1f} of the bf16x3 bound; single {h:.3f} of the bf16 bound; f32 {e:.3f} of the f32 bound')
    assert s <= 0.5, f'{what}: the split evaluation uses {s:.3f} of the bf16x3 bound'
    assert g > 1.0, f'{what}: the single-bf16 evaluation stays inside the bf16x3 bound ({g:.3f})'
    assert h <= 0.5, f'{what}: the single-bf16 evaluation uses {h:.3f} of the bf16 bound'
    assert e <= 0.5, f'{what}: the float32 evaluation uses {e:.3f} of the f32 bound'


# ---------------------------------------------------------------------------------------------------------------------
# the table against the rule
# ---------------------------------------------------------------------------------------------------------------------
def test_bounds_are_the_projects():
    import test_train_kernels_gpu as tk
    import savi_train_kernel_cases as sc
    assert gc.TOL == tk.TOL == sc.TOL and gc.TOL_BF16 == tk.TOL_BF16 == sc.TOL_BF16
    assert gc.product is sc.product


@pytest.mark.parametrize('shape', gc.LINEAR_SHAPES, ids=name)
def test_table_ids_are_the_rules(shape):
    lib = _lib()
    split, f32 = gc.LINEAR_CASES[shape]
    assert (lib.sf_linear_config(*shape, 1), lib.sf_linear_config(*shape, 2), lib.sf_linear_config(*shape, 0)) == (split, split, f32)


def test_table_reaches_every_default_configuration():
    lib = _lib()
    reached = {p: {lib.sf_linear_config(*s, p) for s in gc.LINEAR_SHAPES} for p in (0, 1, 2)}
    print('reached:', {p: sorted(v) for p, v in reached.items()})
    assert reached[1] == gc.DEFAULT_IDS_SPLIT and reached[2] == gc.DEFAULT_IDS_SPLIT and reached[0] == gc.DEFAULT_IDS_F32
    assert len(gc.DEFAULT_IDS_SPLIT | gc.DEFAULT_IDS_F32) == 14


def test_default_ids_are_launch_by_ids_cases():
    """every id of the two sets is a case of the switch in launch_by_id, and the switch has no case beyond them and the ones listed as unreachable"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'slotformer_amd', 'csrc', 'gemm.hip')).read()
    body = src[src.index('static int launch_by_id'):src.index('static int linear_config')]
    ids = {int(m) for m in re.findall(r'case (\d+): return launch_cfg<', body)}
    assert ids == gc.DEFAULT_IDS_SPLIT | gc.DEFAULT_IDS_F32 | {100, 102, 103, 105, 121, 123, 130, 28}, sorted(ids)


def test_current_precision_and_thresholds():
    lib = _lib()
    old = lib.sf_get_precision()
    try:
        for p in (0, 1, 2):
            assert lib.sf_set_precision(p) == 0
            for s in gc.LINEAR_SHAPES:
                assert lib.sf_linear_config(*s, -1) == lib.sf_linear_config(*s, p)
    finally:
        lib.sf_set_precision(old)
    # the rule's thresholds, one step to either side (64x64 tiles: 19 x 16 = 304 > 300, 19 x 15 = 285; 12 x 16 = 192)
    assert lib.sf_linear_config(1210, 1000, 256, 1) == 122 and lib.sf_linear_config(1210, 1000, 260, 1) == 107
    assert lib.sf_linear_config(1210, 1000, 508, 1) == 107 and lib.sf_linear_config(1210, 1000, 512, 1) == 109
    assert lib.sf_linear_config(1210, 960, 256, 1) == 108 and lib.sf_linear_config(768, 1024, 256, 1) == 108
    assert lib.sf_linear_config(704, 1024, 256, 1) == 109 and lib.sf_linear_config(511, 40, 36, 1) == 106 and lib.sf_linear_config(512, 40, 36, 1) == 109
    assert lib.sf_linear_config(511, 40, 512, 1) == 115 and lib.sf_linear_config(512, 40, 512, 1) == 109
    assert lib.sf_linear_config(49100, 40, 36, 1) == 133 and lib.sf_linear_config(49024, 40, 36, 1) == 122    # 384 / 383 tiles of 128x64
    assert lib.sf_linear_config(49152, 64, 2048, 1) == 132 and lib.sf_linear_config(49152, 64, 2044, 1) == 133
    assert lib.sf_linear_config(16300, 384, 36, 1) == 131 and lib.sf_linear_config(16300, 385, 36, 1) == 133
    assert lib.sf_linear_config(16300, 511, 36, 1) == 133 and lib.sf_linear_config(16300, 513, 36, 1) == 131
    assert lib.sf_linear_config(4065, 72, 68, 0) == 4 and lib.sf_linear_config(4064, 72, 68, 0) == 3        # 256 / 254 tiles of 32x64
    assert lib.sf_linear_config(70, 40, 508, 0) == 3 and lib.sf_linear_config(70, 40, 512, 0) == 7


# ---------------------------------------------------------------------------------------------------------------------
# the bounds against the arithmetic
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', gc.LINEAR_SHAPES, ids=name)
def test_linear_bounds(shape):
    c = gc.linear_inputs(shape)
    for ln in (False, True):
        modes = [m for m in gc.modes_of(shape) if gc.MODES[m][3] == ln]
        raws = {a: gc.linear_raw(c['x'], c['w'], c['g'] if ln else None, c['be'], gc.LN_EPS, a) for a in ('split', 'single', 'f32')}
        for mode in modes:
            bias, relu, res, _ = gc.MODES[mode]
            ref = gc.linear_eval(shape, mode)
            ev = {a: gc.linear_finish(r, c['b'] if bias else None, relu, c['r'] if res else None) for a, r in raws.items()}
            bounds_hold(f'linear {shape} {mode}', ref, ev['split'], ev['single'], ev['f32'])
    if shape == (1, 1, 4):   # no ReLU clips the case's only output
        assert gc.linear_eval(shape, 'bias_relu').item() > 0 and (gc.linear_eval(shape, 'ln_bias_relu_residual') - c['r'].double()).item() > 0


def _conv_bounds(what, c, raw_of, options):
    raws = {a: raw_of(a) for a in ('split', 'single', 'f32')}
    for relu, bias, table in options:
        fin = lambda r: gc.conv_finish(r, c['b'] if bias else None, relu, c.get('table') if table else None)   # noqa: E731
        bounds_hold(f'{what} relu {relu} bias {int(bias)} table {int(table)}', fin(c['raw']), *(fin(raws[a]) for a in ('split', 'single', 'f32')))


@pytest.mark.parametrize('case', gc.NHWC_CASES, ids=name)
def test_nhwc_convolution_bounds(case):
    c = gc.nhwc_case(case)
    _conv_bounds(f'nhwc {case}', c, lambda a: gc.conv_closed(c['x'], c['w'], 1, a), gc.NHWC_OPTIONS)


@pytest.mark.parametrize('case', gc.NCHW_CASES, ids=name)
def test_nchw_convolution_bounds(case):
    c = gc.nchw_case(case)
    x = c['img'].permute(0, 2, 3, 1).contiguous()
    _conv_bounds(f'nchw {case}', c, lambda a: gc.conv_closed(x, c['w'], case[6], a), [(1, True, True), (0, False, False)])


@pytest.mark.parametrize('case', gc.DECONV_CASES, ids=name)
def test_transposed_convolution_bounds(case):
    c = gc.deconv_case(case)
    _conv_bounds(f'deconv {case}', c, lambda a: gc.deconv_closed(c['x'], c['w'], case[6], a), [(1, True, False), (0, False, False)])


# ---------------------------------------------------------------------------------------------------------------------
# the closed-form references against torch.nn.functional in float64
# ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= 1e-12 * max(b.abs().max().item(), 1.0), err


@pytest.mark.parametrize('case', gc.NHWC_CASES, ids=name)
def test_nhwc_reference_is_conv2d(case):
    c = gc.nhwc_case(case)
    ks = case[5]
    _same(c['raw'], F.conv2d(c['x'].double().permute(0, 3, 1, 2), c['w'].double(), None, padding=ks // 2).permute(0, 2, 3, 1))
    full = gc.conv_finish(c['raw'], c['b'], 1, c['table'])
    ref = torch.relu(F.conv2d(c['x'].double().permute(0, 3, 1, 2), c['w'].double(), c['b'].double(), padding=ks // 2)).permute(0, 2, 3, 1)
    _same(full, ref + c['table'].double().view(1, case[1], case[2], case[4]))


@pytest.mark.parametrize('case', gc.NCHW_CASES, ids=name)
def test_nchw_reference_is_conv2d(case):
    c = gc.nchw_case(case)
    ks, stride = case[5], case[6]
    ref = F.conv2d(c['img'].double(), c['w'].double(), None, stride=stride, padding=ks // 2).permute(0, 2, 3, 1)
    _same(c['raw'], ref)
    assert c['table'].shape[0] == ref.shape[1] * ref.shape[2]


@pytest.mark.parametrize('case', gc.DECONV_CASES, ids=name)
def test_transposed_reference_is_conv_transpose2d(case):
    c = gc.deconv_case(case)
    ks, stride = case[5], case[6]
    ref = F.conv_transpose2d(c['x'].double().permute(0, 3, 1, 2), c['w'].double(), None, stride=stride, padding=ks // 2, output_padding=stride - 1)
    _same(c['raw'], ref.permute(0, 2, 3, 1))
    assert c['raw'].shape[1:3] == (case[1] * stride, case[2] * stride)


def test_linear_reference_is_torch():
    for shape in ((33, 65, 36), (7, 128, 260)):
        c = gc.linear_inputs(shape)
        ref = torch.relu(F.linear(F.layer_norm(c['x'].double(), (shape[2], ), c['g'].double(), c['be'].double(), gc.LN_EPS), c['w'].double(),
                                  c['b'].double())) + c['r'].double()
        _same(gc.linear_eval(shape, 'ln_bias_relu_residual'), ref)
        _same(gc.linear_eval(shape, 'residual'), F.linear(c['x'].double(), c['w'].double()) + c['r'].double())


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: negative return codes with a message, before any device work
# ---------------------------------------------------------------------------------------------------------------------
def test_linear_config_rejects_bad_arguments():
    lib = _lib()
    for args in ((8, 8, 6, 1), (8, 8, 0, 1), (8, 0, 8, 1), (-1, 8, 8, 1)):
        assert lib.sf_linear_config(*args) < 0 and 'multiple of 4' in _err(), args
    for p in (3, -2):
        assert lib.sf_linear_config(8, 8, 8, p) < 0 and 'precision' in _err(), p
    assert lib.sf_linear_config(0, 8, 8, 1) > 0      # M = 0 is a valid (empty) call


def test_entry_points_reject_bad_arguments():
    lib = _lib()
    one = C.c_void_p(16)   # a non-null dummy pointer: every case below is rejected before it is dereferenced

    def linear(lda=8, ldr=8, ldc=8, M=4, N=8, K=8, g=None, b=None, res=None):
        return lib.sf_linear_f32(one, lda, one, None, g, b, 1e-5, res, ldr, one, ldc, M, N, K, 0, None)

    assert linear(K=6) < 0 and 'multiple of 4' in _err()
    assert linear(lda=10) < 0 and 'leading dimension' in _err()        # lda % 4
    assert linear(lda=4) < 0 and 'leading dimension' in _err()         # lda < K
    assert linear(ldc=7) < 0 and 'leading dimension' in _err()         # ldc < N
    assert linear(res=one, ldr=7) < 0 and 'residual leading dimension' in _err()
    assert linear(ldr=7, M=0) == 0                                     # ldr is not looked at without a residual
    assert linear(g=one) < 0 and 'come together' in _err()
    assert linear(b=one) < 0 and 'come together' in _err()
    assert linear(M=-1) < 0
    # Cin % 4 and even ks
    assert lib.sf_conv2d_nhwc_f32(one, one, None, None, one, 1, 4, 4, 6, 8, 3, 0, None) < 0 and 'conv shape' in _err()
    assert lib.sf_conv2d_nhwc_f32(one, one, None, None, one, 1, 4, 4, 8, 8, 4, 0, None) < 0 and 'conv shape' in _err()
    assert lib.sf_conv_transpose2d_nhwc_f32(one, one, None, one, 1, 4, 4, 6, 8, 3, 2, 0, None) < 0 and 'deconv shape' in _err()
    assert lib.sf_conv_transpose2d_nhwc_f32(one, one, None, one, 1, 4, 4, 8, 8, 4, 2, 0, None) < 0 and 'deconv shape' in _err()
    assert lib.sf_conv_transpose2d_nhwc_f32(one, one, None, one, 1, 4, 4, 8, 8, 3, 0, 0, None) < 0 and 'deconv shape' in _err()
    assert lib.sf_conv2d_nchw_in_f32(one, 48, one, None, None, one, 1, 3, 4, 4, 8, 4, 1, 0, None) < 0 and 'conv shape' in _err()
    assert lib.sf_conv2d_nchw_in_f32(one, 48, one, None, None, one, 1, 3, 4, 4, 8, 3, 0, 0, None) < 0 and 'conv shape' in _err()
    assert lib.sf_conv2d_nchw_in_f32(None, 48, one, None, None, one, 1, 3, 4, 4, 8, 3, 1, 0, None) < 0 and 'null pointer' in _err()
