"""GPU: the fused GEMM core (csrc/gemm.hip) against float64, one library call at a time, on the cases of tests/gemm_cases.py -- every tile
configuration the host rule can pick for sf_linear_f32, every K tail its loops can end on, padded leading dimensions, the three convolution loaders
off the shapes their specialised kernels take -- under the three arithmetic modes of the library.

Every comparison is element by element, |a - b| <= rtol |b| + floor max |b|, at the project's bounds (gemm_cases.PROJECT = TOL / TOL_BF16 of
tests/test_train_kernels_gpu.py); tests/test_gemm_cases.py shows on the CPU that these bounds tell the arithmetic modes apart on every case.
Outputs are NaN-filled before a call, so an element no thread wrote fails the comparison; operands and outputs carry NaN pads and guards.
The `arith` fixture is this file's own: tests/conftest.py's `precision` has no single-pass bf16."""
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

ARITHS = ('bf16x3', 'f32', 'bf16')
GUARD = 256                  # floats of NaN behind every flat output
NAN = float('nan')


def _lib():
    from slotformer_amd._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return _lib().sf_last_error_string().decode()


def _p(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(params=ARITHS)
def arith(request):
    """run under one arithmetic mode of the library: split-bf16 (the default), exact f32, single-pass bf16"""
    lib = _lib()
    old = lib.sf_get_precision()
    assert lib.sf_set_precision(gc.PRECISION_MODE[request.param]) == 0
    yield request.param
    lib.sf_set_precision(old)


def name(case):
    return 'x'.join(str(v) for v in case)


def pairs(cases, ariths, keep=lambda c, a: True):
    """(case, arith) parameters, case-major: the float64 references are cached per case"""
    return [pytest.param(c, a, id=f'{name(c)}-{a}') for c in cases for a in ariths if keep(c, a)]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def measure(out, ref, tol, what, failures):
    """prints the largest error over its bound; a miss is collected, so that one case reports all its modes"""
    ratio = gc.err_over_bound(out, ref, tol)
    print(f'gemm_edges {what} ratio {ratio:.3f}')
    if not ratio <= 1.0:
        failures.append(f'{what}: max err / bound {ratio:.3f}')
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# sf_linear_f32
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def rows_on(dev, t, ld=None, guard_rows=2):
    """t [rows, cols] on the device at leading dimension ld, with guard_rows more rows behind it; every pad and guard element is NaN"""
    rows, cols = t.shape
    buf = torch.full((rows + guard_rows, ld or cols), NAN, device=dev)
    buf[:rows, :cols] = t.to(dev)
    return buf


class Linear:
    """the operands of one case on the device (uploaded once per test), and the call"""

    def __init__(self, dev, shape, pad=(0, 0, 0), x=None, w=None):
        c = gc.linear_inputs(shape)
        self.M, self.N, self.K = shape
        self.lda, self.ldc, self.ldr = self.K + pad[0], self.N + pad[1], self.N + pad[2]
        self.dev = dev
        self.x = rows_on(dev, c['x'] if x is None else x, self.lda)
        self.w = (c['w'] if w is None else w).to(dev)
        self.b, self.g, self.be = c['b'].to(dev), c['g'].to(dev), c['be'].to(dev)
        self.r = rows_on(dev, c['r'], self.ldr)

    def __call__(self, mode, eps=gc.LN_EPS, M=None, in_place=False):
        """-> the whole C buffer [M + 2, ldc], NaN wherever the call did not write"""
        bias, relu, res, ln = gc.MODES[mode]
        if in_place:   # C starts as the residual and is its own residual operand
            assert res and self.ldr == self.ldc
            out = self.r.clone()
        else:
            out = torch.full((self.M + 2, self.ldc), NAN, device=self.dev)
        rc = _lib().sf_linear_f32(_p(self.x), self.lda, _p(self.w), _p(self.b) if bias else None, _p(self.g) if ln else None, _p(self.be) if ln else None,
                                  eps, _p(out if in_place else self.r) if res else None, self.ldr, _p(out), self.ldc, self.M if M is None else M,
                                  self.N, self.K, int(relu), _stream())
        assert rc == 0, _err()
        return out

    def result(self, mode, **kw):
        return self(mode, **kw)[:self.M, :self.N]


def expected_config(shape, arith):
    return gc.LINEAR_CASES[shape][1 if arith == 'f32' else 0]


@pytest.mark.parametrize('shape,arith', pairs(gc.LINEAR_SHAPES, ARITHS), indirect=['arith'])
def test_linear_vs_float64(dev, shape, arith):
    """every mode of the case against float64 at the project's bound, every element written, a second call with the same bits; under single-pass
    bf16 the result is also OUTSIDE the split-bf16 bound (it really is the single product)"""
    cfg = _lib().sf_linear_config(*shape, -1)
    assert cfg == expected_config(shape, arith)
    run = Linear(dev, shape)
    failures = []
    for mode in (gc.MODES_BIG if arith == 'bf16' else gc.modes_of(shape)):
        out = run.result(mode)
        ref = gc.linear_eval(shape, mode)
        assert torch.isfinite(out).all(), f'{mode}: an element of C was not written, or is not finite'
        measure(out, ref, gc.PROJECT[arith], f'linear {shape} {mode} {arith} cfg {cfg}', failures)
        if arith == 'bf16' and not gc.err_over_bound(out, ref, gc.TOL['bf16x3']) > 1.0:
            failures.append(f'{mode}: single-pass bf16 is inside the split-bf16 bound')
        if not torch.equal(bits(run.result(mode)), bits(out)):
            failures.append(f'{mode}: a second call gave other bits')
    assert not failures, failures


PADDED_SHAPES = [s for s in gc.LINEAR_SHAPES if s[0] <= 4065]
PAD = (4, 3, 5)              # lda = K + 4, ldc = N + 3, ldr = N + 5


@pytest.mark.parametrize('shape,arith', pairs(PADDED_SHAPES, ('bf16x3', 'f32')), indirect=['arith'])
def test_linear_padded_leading_dimensions(dev, shape, arith):
    """A, C and the residual at leading dimensions past their widths with two guard rows behind them, every pad and guard element NaN: the result is
    within the bound (no pad was read) and every pad and guard element of C is still NaN (none was written); M = 0 returns 0 and leaves C untouched"""
    M, N, K = shape
    run = Linear(dev, shape, PAD)
    failures = []
    for mode in ('residual', 'ln_bias_relu_residual'):
        buf = run(mode)
        assert torch.isfinite(buf[:M, :N]).all()
        measure(buf[:M, :N], gc.linear_eval(shape, mode), gc.PROJECT[arith], f'padded {shape} {mode} {arith} cfg {expected_config(shape, arith)}', failures)
        assert torch.isnan(buf[:M, N:]).all() and torch.isnan(buf[M:]).all(), 'a pad or guard element of C was written'
        assert torch.isnan(run(mode, M=0)).all(), 'M = 0 wrote into C'
    assert not failures, failures


INDEPENDENCE_SHAPES = [(33, 65, 36), (1210, 1000, 200), (70, 40, 516)]


@pytest.mark.parametrize('mode', ['bias', 'ln_only'])
@pytest.mark.parametrize('shape', INDEPENDENCE_SHAPES, ids=name)
@pytest.mark.parametrize('arith', ['bf16x3', 'f32'], indirect=True)
def test_linear_rows_and_columns_are_independent(dev, arith, shape, mode):
    """a NaN at A[i, k] makes row i of C non-finite and leaves every other row with the bits it had; a NaN at W[n, k] does that to column n.  i and n
    lie in the last, ragged tile (whose out-of-range rows are clamped loads of row M - 1 / N - 1) or in the first, k in the K tail or in the first quad
    (k = 0 is also the address every masked tail load is clamped to).  With the LayerNorm prologue a row's statistics must come from that row alone, in
    the register form of configuration 122 and in the separate pass.
    Non-finite and not NaN: prologue and epilogue clip with fmaxf(v, relu ? 0 : -inf), which returns its other operand for a NaN -- a NaN accumulator
    is stored as -inf without a ReLU (and as 0 with one, which is why neither mode here has a ReLU)."""
    M, N, K = shape
    c = gc.linear_inputs(shape)
    clean = Linear(dev, shape).result(mode)
    assert torch.isfinite(clean).all()
    for i, k in ((M - 1, K - 1), (0, 0), (M - 1, 1)):
        x = c['x'].clone()
        x[i, k] = NAN
        out = Linear(dev, shape, x=x).result(mode)
        assert not torch.isfinite(out[i]).any(), (i, k)
        others = torch.arange(M, device=dev) != i
        assert torch.equal(bits(out[others]), bits(clean[others])), f'A[{i}, {k}] reached another row'
    for n, k in ((N - 1, K - 1), (0, 0), (N - 1, 2)):
        w = c['w'].clone()
        w[n, k] = NAN
        out = Linear(dev, shape, w=w).result(mode)
        assert not torch.isfinite(out[:, n]).any(), (n, k)
        others = torch.arange(N, device=dev) != n
        assert torch.equal(bits(out[:, others]), bits(clean[:, others])), f'W[{n}, {k}] reached another column'


LN_EDGE_EPS = 1e-3
CONSTANT = 3.25              # K * 3.25 and every partial sum of it are exact in float32, so is the mean


@pytest.mark.parametrize('mode', ['ln_only', 'ln_bias_relu_residual'])
@pytest.mark.parametrize('shape', [(100, 36, 100), (1210, 1000, 200)], ids=name)
@pytest.mark.parametrize('arith', ['bf16x3', 'f32'], indirect=True)
def test_linear_layernorm_edges(dev, arith, shape, mode):
    """LayerNorm prologue at ln_eps = 1e-3 with two kinds of rows among the random ones, first and last (ragged) row tile:
    * a constant row: the mean is exact and the variance zero, LN(row) = beta, the result act(beta . W^T + bias) + residual -- at the project's bound
      against that row's own largest element.
    * a row of mean 100 and unit spread.  Its mean is a float32 sum of K values near 100 divided by K: each level of the summation tree (two in a
      quad, up to four chunks or strides, the log2 of 8 .. 16 lanes, the division: about eleven) rounds a partial sum of at most K * 100 to half an
      ulp, i.e. adds at most 100 * 2^-24 to the mean, and roundings of independent sign add as the root: sqrt(11) < 4.  The error d of the mean is
      common to all K elements of (x - mean) (the subtraction itself is exact: x and the mean lie within a factor of two), so C[i, n] moves by
      d * rstd * sum_k gamma[k] W[n, k] -- a signed sum the test computes.  The variance is a sum of squares of order 1 and loses nothing (a one-pass
      E[x^2] - mean^2 in float32 would be off by 1e4 * 2^-24 * K^0.5, 1e-2 of the variance).  Bound for such a row:
          the project's bound on the row + 4 * 2^-24 * max |x[i]| * rstd * |sum_k gamma[k] W[n, k]|."""
    M, N, K = shape
    c = gc.linear_inputs(shape)
    const_rows, big_rows = (0, M - 1), (1, M - 2)
    x = c['x'].clone()
    for i in const_rows:
        x[i] = CONSTANT
    for i in big_rows:
        x[i] += 100.0
    bias, relu, res, _ = gc.MODES[mode]
    ref = gc.linear_finish(gc.linear_raw(x, c['w'], c['g'], c['be'], LN_EDGE_EPS, 'f64'), c['b'] if bias else None, relu, c['r'] if res else None)
    out = Linear(dev, shape, x=x).result(mode, eps=LN_EDGE_EPS).cpu().double()
    assert torch.isfinite(out).all()
    tol, failures = gc.PROJECT[arith], []
    plain = [i for i in range(M) if i not in big_rows]
    measure(out[plain], ref[plain], tol, f'ln_edges {shape} {mode} {arith} random and constant rows', failures)
    beta_row = gc.linear_finish(c['be'].double()[None] @ c['w'].double().t(), c['b'] if bias else None, relu, None)
    for i in const_rows:
        want = beta_row + (c['r'][i:i + 1].double() if res else 0)
        assert (want - ref[i:i + 1]).abs().max() <= 1e-12
        measure(out[i:i + 1], want, tol, f'ln_edges {shape} {mode} {arith} constant row {i}', failures)
    gw = (c['w'].double() * c['g'].double()).sum(1).abs()          # |sum_k gamma[k] W[n, k]|, [N]
    for i in big_rows:
        xi = x[i].double()
        rstd = 1 / torch.sqrt(xi.var(unbiased=False) + LN_EDGE_EPS)
        bound = tol[0] * ref[i].abs() + tol[1] * ref[i].abs().max() + 4 * 2.0**-24 * xi.abs().max() * rstd * gw
        ratio = ((out[i] - ref[i]).abs() / bound).max().item()
        print(f'gemm_edges ln_edges {shape} {mode} {arith} mean-100 row {i} ratio {ratio:.3f} (of the project\'s bound alone: '
              f'{gc.err_over_bound(out[i:i + 1], ref[i:i + 1], tol):.3f})')
        if not ratio <= 1.0:
            failures.append(f'mean-100 row {i}: max err / bound {ratio:.3f}')
    assert not failures, failures


@pytest.mark.parametrize('shape', [(33, 65, 36), (70, 40, 516), (520, 40, 516), (1210, 1000, 200), (1210, 1000, 324), (1210, 700, 132), (49100, 40, 36)], ids=name)
@pytest.mark.parametrize('arith', ['bf16x3', 'f32'], indirect=True)
def test_linear_residual_in_place(dev, arith, shape):
    """C as its own residual (the LSTM gates of the engine: gates = h . W_hh^T + b + gates): the epilogue reads each residual element in the thread
    that writes it, so the result has the bits of the out-of-place call"""
    run = Linear(dev, shape)
    for mode in ('residual', 'ln_bias_relu_residual'):
        assert torch.equal(bits(run.result(mode, in_place=True)), bits(run.result(mode))), mode


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the convolution loaders
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def flat_nan(n, dev):
    return torch.full((n + GUARD, ), NAN, device=dev)


def flat_on(dev, t):
    """t flattened on the device with GUARD floats of NaN behind it"""
    buf = flat_nan(t.numel(), dev)
    buf[:t.numel()] = t.reshape(-1).to(dev)
    return buf


def conv_check(dev, call, ref, tol, what, failures):
    """call(out) twice on NaN-filled, NaN-guarded outputs: every element written, the guard intact, within the bound, the same bits"""
    n = ref.numel()
    outs = []
    for _ in range(2):
        out = flat_nan(n, dev)
        assert call(out) == 0, _err()
        assert torch.isfinite(out[:n]).all(), f'{what}: an output element was not written, or is not finite'
        assert torch.isnan(out[n:]).all(), f'{what}: a write past the end of the output'
        outs.append(out[:n].view(ref.shape))
    measure(outs[0], ref, tol, what, failures)
    if not torch.equal(bits(outs[0]), bits(outs[1])):
        failures.append(f'{what}: a second call gave other bits')


@pytest.mark.parametrize('case', gc.NHWC_CASES, ids=name)
def test_conv_nhwc_off_the_halo_shape(dev, arith, case):
    """sf_conv2d_nhwc_f32 on the implicit-GEMM loader (no case is 64 wide, so none goes to csrc/conv_halo.hip): non-square, F >= 2 frames so that the
    table's row modulo matters, every combination of ReLU, bias and table"""
    F_, H, W, Cin, Cout, ks = case
    c = gc.nhwc_case(case)
    x, wp = flat_on(dev, c['x']), flat_on(dev, c['w'].permute(0, 2, 3, 1).contiguous())
    b, table = c['b'].to(dev), flat_on(dev, c['table'])
    failures = []
    for relu, bias, tab in gc.NHWC_OPTIONS:
        ref = gc.conv_finish(c['raw'], c['b'] if bias else None, relu, c['table'] if tab else None)
        call = (lambda out: _lib().sf_conv2d_nhwc_f32(_p(x), _p(wp), _p(b) if bias else None, _p(table) if tab else None, _p(out), F_, H, W,
                                                                 Cin, Cout, ks, relu, _stream()))
        conv_check(dev, call, ref, gc.PROJECT[arith], f'nhwc {case} relu {relu} bias {int(bias)} table {int(tab)} {arith}', failures)
    assert not failures, failures


@pytest.mark.parametrize('case,arith', pairs(gc.NCHW_CASES, ARITHS, lambda c, a: a == 'f32' or c != gc.NCHW_F32_ONLY), indirect=['arith'])
def test_conv_nchw_scalar_loader(dev, case, arith):
    """sf_conv2d_nchw_in_f32 on the generic loader of the GEMM core (scalar loads, K tails of 75 % 32, 9): frames frame_stride apart with NaN in the
    gap.  This loader has no split-bf16 form -- it contracts on the exact-f32 tile whatever the arithmetic mode -- so it is held to the f32 bound
    in all three"""
    F_, Cin, Hin, Win, Cout, ks, stride = case
    c = gc.nchw_case(case)
    fs = Cin * Hin * Win + gc.NCHW_GAP
    img = flat_nan(F_ * fs, dev)
    for f in range(F_):
        img[f * fs:f * fs + Cin * Hin * Win] = c['img'][f].reshape(-1).to(dev)
    w, b, table = flat_on(dev, c['w']), c['b'].to(dev), flat_on(dev, c['table'])
    failures = []
    for relu, bias, tab in ((1, True, True), (0, False, False), (1, True, False), (0, False, True)):
        ref = gc.conv_finish(c['raw'], c['b'] if bias else None, relu, c['table'] if tab else None)
        call = (lambda out: _lib().sf_conv2d_nchw_in_f32(_p(img), fs, _p(w), _p(b) if bias else None, _p(table) if tab else None, _p(out), F_, Cin,
                                                                    Hin, Win, Cout, ks, stride, relu, _stream()))
        conv_check(dev, call, ref, gc.TOL['f32'], f'nchw {case} relu {relu} bias {int(bias)} table {int(tab)} {arith}', failures)
    assert not failures, failures


@pytest.mark.parametrize('case', gc.DECONV_CASES, ids=name)
def test_conv_transpose(dev, arith, case):
    """sf_conv_transpose2d_nhwc_f32, non-square: one launch per output-parity class at stride 2 and 3 (every output pixel belongs to exactly one class:
    the NaN-filled output comes back finite), the single-launch gather at stride 1"""
    F_, H, W, Cin, Cout, ks, stride = case
    c = gc.deconv_case(case)
    x, wp, b = flat_on(dev, c['x']), flat_on(dev, c['w'].permute(1, 2, 3, 0).contiguous()), c['b'].to(dev)
    failures = []
    for relu, bias in ((1, True), (0, False)):
        ref = gc.conv_finish(c['raw'], c['b'] if bias else None, relu, None)
        call = (lambda out: _lib().sf_conv_transpose2d_nhwc_f32(_p(x), _p(wp), _p(b) if bias else None, _p(out), F_, H, W, Cin, Cout, ks, stride,
                                                                           relu, _stream()))
        conv_check(dev, call, ref, gc.PROJECT[arith], f'deconv {case} relu {relu} bias {int(bias)} {arith}', failures)
    assert not failures, failures
