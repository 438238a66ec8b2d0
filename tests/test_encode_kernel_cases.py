"""CPU: every bound tests/test_encode_kernels_gpu.py holds a kernel to is neither unreachable nor vacuous.  For every case, the float64 reference
evaluated in the arithmetic of the kernels' products (operands as bf16 hi + lo, the lo.lo term dropped: tests/encode_kernel_cases.py) sits within HALF of
the bound, and the same evaluation without the lo operands breaks it.  This measures the references and the bounds, never a kernel; the entry points'
argument checks at the end run before any device work.

Two places where `single` cannot break a bound, by construction and not by slack:
  * one slot: the softmax over a single slot is 1 whatever the logits, so the attention and the denominators are exact in any arithmetic; the numerators
    still lose their lo operand.
  * a record's denominator is the SIGNED sum of 512 attention errors against a bound that sums their magnitudes: the single-bf16 errors, each 35 - 60 times
    its own bound, cancel to anything between 0.4 and 8 times the record's.  It is asserted to break the attention and the numerator bounds of the same case.
"""
import ctypes as C

import pytest
import torch

import encode_kernel_cases as ec


def fits_and_breaks(what, split, single):
    print(f'{what}: split {split:.3f}, single {single:.1f} of the bound')
    assert split <= 0.5, f'{what}: the split evaluation uses {split:.3f} of the bound'
    assert single > 1.0, f'{what}: the single-bf16 evaluation stays inside the bound ({single:.3f})'


@pytest.mark.parametrize('bias,relu,table', ec.CONV_OPTIONS)
@pytest.mark.parametrize('res,stride', ec.CONV_SHAPES)
def test_first_convolution_bound(res, stride, bias, relu, table):
    c = ec.conv_case(res, stride)
    ref = ec.conv_finish(c['raw'], c, bias, relu, table)
    fits_and_breaks(f'conv {res} / {stride}', *(ec.conv_over_bound(ec.conv_finish(ec.conv_raw(c['img'], c['w'], stride, m), c, bias, relu, table), ref)
                                                for m in ('split', 'single')))


def test_first_convolution_non_finite_map():
    """the expected map of the non-finite test: a marked input at (y, x) reaches the outputs (y', x') with |stride y' - y| <= 2, |stride x' - x| <= 2"""
    for stride, res in ((1, 64), (2, 128)):
        bad = torch.zeros(1, 3, res, res, dtype=torch.bool)
        bad[0, 1, 10, 0] = True
        hit = ec.conv_nonfinite_expected(bad, stride)[0].nonzero().tolist()
        assert hit == [[y, x] for y in range(64) for x in range(64) if abs(stride * y - 10) <= 2 and abs(stride * x) <= 2], (stride, hit)


@pytest.mark.parametrize('cus,M', ec.PIXEL_CASES)
def test_pixel_chain_bound(cus, M):
    c = ec.pixel_case(M)
    fits_and_breaks(f'pixel chain M {M}', *(ec.pixel_over_bound(ec.pixel_eval(c['x'], m), c['ref']) for m in ('split', 'single')))
    assert ec.pixel_over_bound(ec.pixel_eval(c['x'], 'f32'), c['ref']) <= 0.05   # the float32 stages of the kernel are not what the bound is spent on


def test_planes_are_an_exact_split():
    """hi + lo of a float32 is exact in float32 (what lets the float64 reference of the iteration run on the rows the kernel reads)"""
    planes, x = ec.sa_frame(0, 512)
    assert planes.dtype == torch.bfloat16 and planes.shape == (512, 256)
    assert torch.equal((planes[:, :128].double() + planes[:, 128:].double()).float().double(), planes[:, :128].double() + planes[:, 128:].double())
    assert torch.equal(x.double(), planes[:, :128].double() + planes[:, 128:].double())


@pytest.mark.parametrize('gain', ec.SA_GAINS)
@pytest.mark.parametrize('HW,N', sorted({(HW, N) for _, HW, N in ec.SA_CASES}))
def test_slot_attention_bounds(HW, N, gain):
    c = ec.sa_case(0, HW, N, gain)
    r = {}
    for m in ('split', 'single'):
        attn, num, den = ec.sa_eval(c['x'], c['q'], m)
        r[m] = (ec.over_abs_bound(attn, c['attn'], c['attn_bound']), ec.over_abs_bound(num, c['num'], c['num_bound']),
                ec.over_abs_bound(den, c['den'], c['den_bound']))
        print(f'HW {HW} N {N} gain {gain} {m}: attention {r[m][0]:.3g}, numerators {r[m][1]:.3g}, denominators {r[m][2]:.3g} of the bound; max attention '
              f'error {(attn - c["attn"]).abs().max().item():.2e}')
    assert max(r['split']) <= 0.5, r['split']
    assert r['single'][1] > 1.0, r['single']
    if N > 1:
        assert r['single'][0] > 1.0, r['single']
    assert c['attn'].max() > (0.9 if gain == 32 and N > 1 else 0.0)   # gain 32 is where the softmax is near one-hot


@pytest.mark.parametrize('B,N', ec.PROLOGUE_BN)
@pytest.mark.parametrize('D', ec.PROLOGUE_D)
def test_slot_prologue_bound(D, B, N):
    """exact float32 kernel: a float32 evaluation fits in half of 2e-5 (it uses under 0.03 of it), and even the split evaluation would (0.4)"""
    for with_prev, norm_first, with_noise in ((0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)):
        c = ec.prologue_case(D, B, N, with_prev, norm_first, with_noise)
        r = {}
        for m in ('f32', 'single'):
            out = ec.prologue_eval(c['w'], c['prev'], c['init'], c['noise'], norm_first, m)
            r[m] = max(ec.err_over_bound(a.expand(b.shape), b, ec.SLOT_TOL) for a, b in zip(out, (c['kdist'], c['slots'], c['q'])))
        fits_and_breaks(f'prologue D {D} B {B} N {N} prev {with_prev} norm_first {norm_first} noise {with_noise}', r['f32'], r['single'])
        assert c['kdist'][..., D:].abs().max() <= ec.PROLOGUE_LOGVAR


@pytest.mark.parametrize('p_step', (1, 2))
@pytest.mark.parametrize('B,N,P', ec.UPDATE_CASES)
def test_slot_update_bounds(B, N, P, p_step):
    """the update alone at the bounds of test_slot_update_on_the_matrix_cores, and the whole chain of the NEXT form at the encode's 5e-5"""
    c = ec.update_case(B, N, P, p_step)
    pn, pd = c['pn'][:, ::p_step], c['pd'][:, ::p_step]
    close = lambda a, b, t: ((a - b).abs().max() / (t + t * b.abs().max())).item()   # noqa: E731
    r = {m: ec.update_eval(c['u'], c['pw'], pn, pd, c['prev'], m) for m in ('split', 'single')}
    fits_and_breaks('slots', *(close(r[m][0], c['slots'], ec.UPDATE_TOL_SLOTS) for m in ('split', 'single')))
    fits_and_breaks('q', *(close(r[m][1], c['q'], ec.UPDATE_TOL_Q) for m in ('split', 'single')))
    for nf in (0, 1):
        for wn in (0, 1):
            ref = c['next', nf, wn]
            assert ref[0][..., ec.UPDATE_D:].abs().max() <= ec.PROLOGUE_LOGVAR
            nx = {m: ec.update_next_eval(c['u'], c['pw'], pn, pd, c['prev'], c['noise'] if wn else None, nf, m)[1:] for m in ('split', 'single')}
            for i, name in enumerate(('kernel_dist', 'next_slots', 'q')):
                fits_and_breaks(f'next norm_first {nf} noise {wn} {name}', *(ec.err_over_bound(nx[m][i], ref[i], ec.NEXT_TOL) for m in ('split', 'single')))


def test_case_tables_walk_what_they_claim():
    """the grids and rounds the tables are there for, recomputed from the launch code's formulas"""
    for frames in ec.CONV_FRAMES:
        for cus in (1, 3, 5):
            tiles, grid = 32 * frames, 2 * cus
            assert tiles // grid >= 3, (frames, cus)          # every workgroup prefetches at least twice
    assert 32 % 6 and 96 % 10                                 # ragged walks
    rounds = {}
    for cus, M in ec.PIXEL_CASES:
        tiles = (M + 31) // 32
        grid = min((tiles + 7) // 8, cus or 256)
        rounds[cus, M] = ((tiles + 8 * grid - 1) // (8 * grid), M % 32, tiles % (8 * grid))
    assert sorted(v[0] for v in rounds.values()) == [1, 2, 2, 3, 3, 3]
    assert all(v[1] for v in rounds.values())                 # a ragged last tile everywhere
    assert rounds[1, 609] == (3, 1, 4) and rounds[3, 1633] == (3, 1, 4)   # waves without a tile in the last round
    assert sorted({B * N for B, N in ec.PROLOGUE_BN}) == [1, 7, 8, 9, 35]
    assert [B * N for B, N, _ in ec.UPDATE_CASES] == [3, 35, 72, 224]


def test_entry_points_reject_what_their_kernels_do_not_take():
    """negative return codes with a message, before any device work"""
    from slotformer_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.sf_last_error_string().decode()   # noqa: E731
    one = C.c_void_p(16)   # a non-null dummy pointer: every call below is rejected before it is dereferenced
    # the grouped first convolution has no generic path
    for bad in (dict(Cin=4), dict(Cout=32), dict(ks=3), dict(Hin=32), dict(stride=2), dict(fgroup=0)):
        a = dict(fgroup=2, Cin=3, Hin=64, Win=64, Cout=64, ks=5, stride=1)
        a.update(bad)
        assert lib.sf_conv2d_nchw_in_grouped_f32(one, 3 * 64 * 64, a['fgroup'], 0, one, one, None, one, 2, a['Cin'], a['Hin'], a['Win'], a['Cout'], a['ks'],
                                                 a['stride'], 1, None) < 0, bad
        assert 'sf_conv2d_nchw_in_grouped_f32' in err()
    assert lib.sf_conv2d_nchw_in_grouped_f32(None, 0, 1, 0, one, one, None, one, 1, 3, 64, 64, 64, 5, 1, 1, None) < 0 and 'null pointer' in err()
    assert lib.sf_pixel_feat_f32(*([one] * 10), 32, 1e-5, 5, None) < 0 and '0 .. 4' in err()
    for HW, N in ((256, 7), (4096, 9), (4096, 0)):
        assert lib.sf_slot_attn_iter_planes_f32(one, HW, one, one, one, None, 0, 1, HW, N, 0.1, 1e-6, None) < 0, (HW, N)
        assert 'multiple of 512' in err()
    pro = lambda D, kd_w=one: lib.sf_slot_prologue_f32(None, one, None, None, None, None, None, None, 0, kd_w, one, None, 0, None, 0, one, one, one, one,   # noqa: E731
                                                       one, 1, 7, D, 1e-5, None)
    assert pro(100) < 0 and 'sf_slot_prologue_f32' in err()
    assert pro(448) < 0 and pro(128, None) < 0
    upd = lambda D, H, P, p_step, nxt, q_out=one: lib.sf_slot_update_packed_next_f32(   # noqa: E731
        one, one, P, one, one, one, one, one, one, one, one, one, one, one, one, one, one, one, q_out, 1, 7, D, H, 1e-5, None, 0, p_step, one, one, one, one,
        one, one, 1, one, one, None, 0, None, 0, nxt, None)
    assert upd(192, 384, 16, 1, None) < 0 and 'slot size 128' in err()
    assert upd(128, 256, 65, 1, None) < 0
    assert upd(128, 256, 15, 2, None) < 0 and 'bad slot shape' in err()
    assert upd(128, 256, 16, 3, None) < 0
    assert upd(128, 256, 16, 1, one, q_out=None) < 0 and 'next-step form' in err()
