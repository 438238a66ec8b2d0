"""GPU parity of STEVE's training attention -- sf_slate_attention_train_fwd_f32 / sf_slate_attention_train_bwd_f32 of
csrc/slate_attn_bwd.hip and the TRAIN instantiation of the flash kernels -- against float64 on the CPU, one C ABI call at a time, at
every head dim the entry points take, at the tile edges, in the layouts the callers pass, with and without dropout, with `lse` given
or recomputed (tests/slate_attn_train_cases.py holds the table and the reference, tests/test_slate_attn_train_cases.py checks them
on the CPU).

The backward is fed the REFERENCE's `out` (and `lse`) rounded to float32, so that a forward error can neither hide nor cause a
backward failure.  Every output is filled with NaN before the call and compared in full, element by element, in the form
|a - b| <= rtol |b| + floor max|b| with the bound of the kernel the call takes (slate_attn_train_cases.TOL_FWD / TOL_BWD), and in
the max-norm against the figure tests/test_kernels_gpu.py holds the same kernel to.  dq is accumulated with float atomics: it is held
to the float64 bound on every call and to nothing else; dk, dv, out and lse repeat bit for bit.
"""
import pytest
import torch

import slate_attn_train_cases as tc
import steve_kernel_cases as sc
from test_steve_kernels_gpu import NAN, _err, _lib, _stream, nan_like_bits

pytestmark = pytest.mark.gpu

SPARE_ROWS, PAD_COLS = 7, 4
BWD_IDS = [tc.case_id(c) for c in tc.BWD_CASES]


def nan_dev(dev, *shape):
    return torch.full(shape, NAN, device=dev)


class Buffers:
    """the device tensors of one call in one of the layouts
      dense   q, k, v, out, d_out and the three gradients as contiguous [B, L, d] tensors
      kv_off  dense, but k and v start one float into their allocations (4 bytes off a 16-byte boundary)
      packed  q | k | v as the column blocks of one [B, L, 3d] buffer and dq | dk | dv as those of another, as train._SelfAttention
      padded  q, out, d_out in the first Lq rows and d columns of [B, Lq + 7, d + 4] buffers, k | v side by side in the first Lk rows of
              a [B, Lk + 7, 2d + 4] buffer, the gradients in buffers of the same shapes; explicit batch strides
    Everything the call has no business reading is NaN, and so is every gradient and output buffer, all over."""

    def __init__(self, dev, c, layout, seq=None):
        ref = tc.reference64(c)
        pick = (lambda t: t) if seq is None else (lambda t: t[seq:seq + 1])
        q, k, v, g = (pick(ref[n]) for n in 'qkvg')
        o, lse = pick(ref['out']).float(), pick(ref['lse']).float()
        B, Lq, Lk, d = q.shape[0], c.Lq, c.Lk, c.H * c.hd
        self.B, self.c, self.layout, self.d = B, c, layout, d
        self.lse, self.lse_out = lse.contiguous().to(dev), nan_dev(dev, B, c.H, Lq)
        if layout in ('dense', 'kv_off'):
            off = 1 if layout == 'kv_off' else 0

            def put(t):
                flat = nan_dev(dev, t.numel() + 4)
                view = flat[off:off + t.numel()].view(t.shape)
                view.copy_(t)
                return view
            self.q, self.o, self.g = q.to(dev).contiguous(), o.to(dev).contiguous(), g.to(dev).contiguous()
            self.k, self.v = put(k), put(v)
            assert self.k.data_ptr() % 16 == 4 * off and self.v.data_ptr() % 16 == 4 * off and self.q.data_ptr() % 16 == 0
            self.gq, self.gk, self.gv, self.out = nan_dev(dev, B, Lq, d), nan_dev(dev, B, Lk, d), nan_dev(dev, B, Lk, d), nan_dev(dev, B, Lq, d)
            self.grad_bufs, self.out_buf = [self.gq, self.gk, self.gv], self.out
            self.ld, self.bs = (d, d, d, d), (Lq * d, Lk * d, Lk * d, Lq * d)
        elif layout == 'packed':
            assert Lq == Lk
            buf, gbuf = torch.cat([q, k, v], -1).to(dev).contiguous(), nan_dev(dev, B, Lq, 3 * d)
            self.q, self.k, self.v = buf[..., :d], buf[..., d:2 * d], buf[..., 2 * d:]
            self.gq, self.gk, self.gv = gbuf[..., :d], gbuf[..., d:2 * d], gbuf[..., 2 * d:]
            self.o, self.g, self.out = o.to(dev).contiguous(), g.to(dev).contiguous(), nan_dev(dev, B, Lq, d)
            self.grad_bufs, self.out_buf = [gbuf], self.out
            self.ld, self.bs = (3 * d, 3 * d, 3 * d, d), (Lq * 3 * d, Lq * 3 * d, Lq * 3 * d, Lq * d)
        else:
            assert layout == 'padded'
            rq, rk, wq, wkv = Lq + SPARE_ROWS, Lk + SPARE_ROWS, d + PAD_COLS, 2 * d + PAD_COLS

            def rows(t, n, w):
                b = torch.full((B, n, w), NAN)
                b[:, :t.shape[1], :d] = t
                return b.to(dev)
            qb, ob, gb = rows(q, rq, wq), rows(o, rq, wq), rows(g, rq, wq)
            kvb = torch.full((B, rk, wkv), NAN)
            kvb[:, :Lk, :d], kvb[:, :Lk, d:2 * d] = k, v
            kvb = kvb.to(dev)
            gqb, gkvb, outb = nan_dev(dev, B, rq, wq), nan_dev(dev, B, rk, wkv), nan_dev(dev, B, rq, wq)
            self.q, self.o, self.g, self.k, self.v = qb[:, :Lq, :d], ob[:, :Lq, :d], gb[:, :Lq, :d], kvb[:, :Lk, :d], kvb[:, :Lk, d:2 * d]
            self.gq, self.gk, self.gv, self.out = gqb[:, :Lq, :d], gkvb[:, :Lk, :d], gkvb[:, :Lk, d:2 * d], outb[:, :Lq, :d]
            self.grad_bufs, self.out_buf = [gqb, gkvb], outb
            self.ld, self.bs = (wq, wkv, wkv, wq), (rq * wq, rk * wkv, rk * wkv, rq * wq)
        for t, ld, bs in zip((self.q, self.k, self.v, self.o), self.ld, self.bs):   # the strides handed over are the views' own
            assert all(n == 1 or st == want for n, st, want in zip(t.shape, t.stride(), (bs, ld, 1))), (t.stride(), bs, ld)
        assert self.g.stride() == self.o.stride() == self.out.stride() and self.gq.stride() == self.q.stride()
        assert self.gk.stride() == self.k.stride() and self.gv.stride() == self.v.stride()

    def backward(self, with_lse=True, **over):
        """one sf_slate_attention_train_bwd_f32 call -> its return code"""
        c = self.c
        nb = _lib().sf_slate_attention_bwd_workspace_bytes(self.B, c.Lq, c.H)
        self.ws = torch.empty(nb, dtype=torch.uint8, device=self.q.device)
        a = dict(q=self.q.data_ptr(), k=self.k.data_ptr(), v=self.v.data_ptr(), o=self.o.data_ptr(), g=self.g.data_ptr(),
                 lse=self.lse.data_ptr() if with_lse else None, dq=self.gq.data_ptr(), dk=self.gk.data_ptr(), dv=self.gv.data_ptr(),
                 ld=self.ld, bs=self.bs, Lq=c.Lq, Lk=c.Lk, hd=c.hd, causal=int(c.causal), p=c.p, ws=self.ws.data_ptr(), nb=nb)
        a.update(over)
        return _lib().sf_slate_attention_train_bwd_f32(a['q'], a['k'], a['v'], a['o'], a['g'], a['lse'], a['dq'], a['dk'], a['dv'], *a['ld'],
                                                       *a['bs'], self.B, a['Lq'], a['Lk'], c.H, a['hd'], a['causal'], a['p'], tc.SEED,
                                                       a['ws'], a['nb'], _stream())

    def forward(self):
        """one sf_slate_attention_train_fwd_f32 call into `out` and `lse_out`"""
        c = self.c
        return _lib().sf_slate_attention_train_fwd_f32(self.q.data_ptr(), self.k.data_ptr(), self.v.data_ptr(), self.out.data_ptr(),
                                                       self.lse_out.data_ptr(), *self.ld, *self.bs, self.B, c.Lq, c.Lk, c.H, c.hd,
                                                       int(c.causal), c.p, tc.SEED, _stream())

    def grads(self):
        return dict(dq=self.gq.cpu(), dk=self.gk.cpu(), dv=self.gv.cpu())

    def untouched_outside(self):
        """True if every element of the gradient and output buffers outside the head blocks still holds the fill's bit pattern"""
        ok = True
        for buf, blocks in ([(self.grad_bufs[0], [self.gq]), (self.grad_bufs[-1], [self.gk, self.gv]), (self.out_buf, [self.out])]
                            if self.layout == 'padded' else []):
            probe = nan_like_bits(buf).clone()
            for blk in blocks:   # mark the blocks as fine, whatever they hold
                rows, cols = blk.shape[1], blk.shape[2]
                c0 = (blk.data_ptr() - buf.data_ptr()) // 4 % buf.shape[2]
                probe[:, :rows, c0:c0 + cols] = True
            ok = ok and bool(probe.all())
        return ok


def run_backward(dev, c, layout='dense', with_lse=True, seq=None):
    b = Buffers(dev, c, layout, seq)
    assert b.backward(with_lse) == 0, _err()
    torch.cuda.synchronize()
    return b


def bwd_kernel(c, precision, layout='dense'):
    d = c.H * c.hd
    ld = {'dense': d, 'kv_off': d, 'packed': 3 * d, 'padded': 2 * d + PAD_COLS}[layout]
    return tc.bwd_kernel_of(c.hd, precision, ld, ld, kv_aligned=layout != 'kv_off')


def tol_sum(*tols):
    return tuple(sum(t[i] for t in tols) for i in (0, 1))


def hold(got, ref, c, names, tol, maxnorm, what):
    """every named output: no NaN, element-wise within tol, max-norm within `maxnorm` (None: not asserted); prints the ratios"""
    worst = 0.
    for n in names:
        a, base = got[n], tc.floor_base(c, n)
        assert a.shape == ref[n].shape and not torch.isnan(a).any(), f'{what} {n}: NaN or shape'
        r = tc.ratio(a, ref[n], tol, base)
        m = tc.ratio(a, ref[n], (0., maxnorm), base) if maxnorm else 0.
        print(f'RATIO {what} | {n} | err / bound {r:.3f} | max-norm err / figure {m:.3f}')
        worst = max(worst, r, m)
    assert worst <= 1.0, f'{what}: largest err / bound {worst:.3f}'


def hold_backward(b, c, precision, what, names=('dq', 'dk', 'dv')):
    kernel = bwd_kernel(c, precision, b.layout)
    hold(b.grads(), tc.reference64(c), c, names, tc.TOL_BWD[(kernel, precision)], tc.MAXNORM_BWD[precision],
         f'{kernel} | {precision} | {tc.case_id(c)} {what}')


def hold_forward(b, c, precision, what):
    kernel = tc.fwd_kernel_of(c.hd, c.Lq, c.causal, precision)
    ref, tol = tc.reference64(c), tc.TOL_FWD[(tc.fwd_kernel_of(c.hd, c.Lq, c.causal, precision), precision)]
    hold(dict(out=b.out.cpu()), ref, c, ('out', ), tol, None, f'{kernel} | {precision} | {tc.case_id(c)} {what}')
    lse = b.lse_out.cpu()
    err, bound = (lse.double() - ref['lse']).abs().max().item(), tol[0] * ref['smax'] + tol[1]
    print(f'RATIO {kernel} | {precision} | {tc.case_id(c)} {what} | lse | err / bound {err / bound:.3f} | max-norm err / figure 0.000')
    assert not torch.isnan(lse).any() and err <= bound, (err, bound)


# ---------------------------------------------------------------------------------------------------------------------
# against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', tc.BWD_CASES, ids=BWD_IDS)
def test_backward_against_float64(dev, precision, c):
    """dq, dk, dv from the reference's out, with the reference's lse and with lse recomputed by the stats kernel"""
    print(c.edge)
    for with_lse in (True, False):
        hold_backward(run_backward(dev, c, 'dense', with_lse), c, precision, 'lse given' if with_lse else 'lse recomputed')


@pytest.mark.parametrize('c', tc.CASES, ids=[tc.case_id(c) for c in tc.CASES])
def test_training_forward_against_float64(dev, precision, c):
    """out and lse of the training forward: every even head dim, the cross shapes, dropout; a fully dropped row is a row of zeros"""
    b = Buffers(dev, c, 'dense')
    assert b.forward() == 0, _err()
    hold_forward(b, c, precision, 'forward')
    if c in (tc.DROPPED_CAUSAL, tc.DROPPED_CROSS):
        gone = ((tc.keep_mask(c) & tc.live_mask(c)).sum(-1) == 0)
        assert (b.out.cpu().view(c.B, c.Lq, c.H, c.hd).transpose(1, 2)[gone] == 0).all()


@pytest.mark.parametrize('c', [tc.DROPPED_CAUSAL, tc.DROPPED_CROSS], ids=tc.case_id)
def test_fully_dropped_rows_get_no_gradient(dev, precision, c):
    """dq of a row whose live keys are all dropped: P (dP * 0 - D) with D = dO . 0 -- exactly zero, not merely small"""
    b = run_backward(dev, c)
    gone = ((tc.keep_mask(c) & tc.live_mask(c)).sum(-1) == 0)
    assert gone.any() and (b.gq.cpu().view(c.B, c.Lq, c.H, c.hd).transpose(1, 2)[gone] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------
def layout_check(dev, precision, c, layout):
    dense, other = run_backward(dev, c, 'dense'), run_backward(dev, c, layout)
    assert bwd_kernel(c, precision, layout) == bwd_kernel(c, precision, 'dense')
    for buf in other.grad_bufs:
        if layout == 'packed':
            assert not torch.isnan(buf).any()           # every element of the packed gradient is written
    assert other.untouched_outside()
    assert torch.equal(other.gk, dense.gk) and torch.equal(other.gv, dense.gv)
    hold_backward(other, c, precision, layout)
    # the forward in the same layout: bit for bit the dense call's
    assert dense.forward() == 0 and other.forward() == 0, _err()
    assert other.untouched_outside()
    assert not torch.isnan(other.out).any() and torch.equal(other.out, dense.out) and torch.equal(other.lse_out, dense.lse_out)


@pytest.mark.parametrize('c', tc.LAYOUT_CAUSAL, ids=tc.case_id)
def test_packed_qkv_as_self_attention_passes_it(dev, precision, c):
    """q | k | v and dq | dk | dv as column blocks of [B, L, 3d] buffers: dq is cleared by one strided memset over all B L rows"""
    layout_check(dev, precision, c, 'packed')


@pytest.mark.parametrize('c', tc.LAYOUT_CROSS, ids=tc.case_id)
def test_padded_rows_and_batches(dev, precision, c):
    """spare rows after every sequence and pad columns after every row: dq is cleared sequence by sequence; NaN everywhere the call
    must not read, and the fill's bit pattern everywhere it must not write"""
    layout_check(dev, precision, c, 'padded')


def test_k_and_v_off_16_bytes_take_the_generic_kernel(dev, precision):
    """hd 48 with k and v one float into their allocations (ldk % 4 == 0): the 48-wide kernel's 16-byte loads are not for them"""
    c = tc.find(False, 130, 65, 48, 0.)
    assert bwd_kernel(c, 'bf16x3', 'kv_off') == 'bwd<64>' and bwd_kernel(c, 'bf16x3', 'dense') == 'bwd48v2'
    hold_backward(run_backward(dev, c, 'kv_off'), c, precision, 'k, v off by 4 bytes')


# ---------------------------------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', tc.LAYOUT_CAUSAL + tc.LAYOUT_CROSS, ids=tc.case_id)
def test_two_calls_repeat(dev, precision, c):
    """dk, dv, out and lse bit for bit; dq (float atomics) within the float64 bound on each call"""
    one, two = run_backward(dev, c), run_backward(dev, c)
    assert torch.equal(one.gk, two.gk) and torch.equal(one.gv, two.gv)
    for n, b in enumerate((one, two)):
        hold_backward(b, c, precision, f'call {n}', ('dq', ))
        assert b.forward() == 0, _err()
    assert torch.equal(one.out, two.out) and torch.equal(one.lse_out, two.lse_out) and not torch.isnan(one.out).any()


@pytest.mark.parametrize('c', tc.INDEPENDENT, ids=tc.case_id)
def test_sequences_of_a_batch_do_not_see_each_other(dev, precision, c):
    """p = 0: dk and dv of a sequence are bit for bit those of the sequence run alone.  (With dropout the mask index contains b, so a
    sequence run alone as b = 0 draws another mask: nothing to assert there.)"""
    assert c.p == 0
    whole = run_backward(dev, c)
    for s in range(c.B):
        alone = run_backward(dev, c, seq=s)
        assert torch.equal(whole.gk[s:s + 1], alone.gk) and torch.equal(whole.gv[s:s + 1], alone.gv), s


# ---------------------------------------------------------------------------------------------------------------------
# the autograd nodes
# ---------------------------------------------------------------------------------------------------------------------
def test_slate_attention_node(dev, precision):
    """train._SlateAttention, cross-attention with dropout 0.1: the node's backward takes the kernel's own out and lse, so its
    gradients carry the forward's error too -- the two bounds added"""
    from slotformer_amd import train
    c = tc.CROSS_NODE
    ref = tc.reference64(c)
    q, k, v = (ref[n].to(dev).requires_grad_(True) for n in 'qkv')
    out = train._SlateAttention.apply(q, k, v, c.H, c.causal, c.p, tc.SEED)
    out.backward(ref['g'].to(dev))
    fwd = tc.TOL_FWD[(tc.fwd_kernel_of(c.hd, c.Lq, c.causal, precision), precision)]
    bwd = tc.TOL_BWD[(bwd_kernel(c, precision), precision)]
    hold(dict(out=out.detach().cpu()), ref, c, ('out', ), fwd, None, f'node | {precision} | _SlateAttention')
    hold(dict(dq=q.grad.cpu(), dk=k.grad.cpu(), dv=v.grad.cpu()), ref, c, ('dq', 'dk', 'dv'), tol_sum(fwd, bwd), None,
         f'node | {precision} | _SlateAttention')


def test_self_attention_node(dev, precision):
    """train._SelfAttention, causal L 129 with dropout 0.1, from x and the three weights: out through the packed projection (one
    product at the mode's matrix bound) and the forward; dx and the weight gradients through those two, the attention backward and
    the projection's backward -- a chain whose stages' bounds add"""
    from slotformer_amd import train
    c, n = tc.SELF_NODE, tc.self_attention_node_case()
    x = n['x'].to(dev).requires_grad_(True)
    ws = [w.to(dev).requires_grad_(True) for w in n['w']]
    out = train._SelfAttention.apply(x, *ws, c.H, True, c.p, tc.SEED)
    out.backward(n['g'].to(dev))
    d = c.H * c.hd
    fwd = tc.TOL_FWD[(tc.fwd_kernel_of(c.hd, c.Lq, True, precision), precision)]
    bwd = tc.TOL_BWD[(tc.bwd_kernel_of(c.hd, precision, 3 * d, 3 * d), precision)]
    mm = sc.TOL[precision]
    ref = dict(out=n['out'], dx=n['dx'], dwq=n['dw'][0], dwk=n['dw'][1], dwv=n['dw'][2])
    got = dict(out=out.detach().cpu(), dx=x.grad.cpu(), dwq=ws[0].grad.cpu(), dwk=ws[1].grad.cpu(), dwv=ws[2].grad.cpu())
    hold(got, ref, c, ('out', ), tol_sum(mm, fwd), None, f'node | {precision} | _SelfAttention')
    hold(got, ref, c, ('dx', 'dwq', 'dwk', 'dwv'), tol_sum(mm, fwd, bwd, mm), None, f'node | {precision} | _SelfAttention')


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_gradients_alone(dev):
    """an error code, a message, and dq, dk, dv still NaN all over: every check sits in front of the memset and the launches.  The
    buffers are those of a valid call, so an argument that slipped through would still stay inside them."""
    c = tc.Case(2, 2, 16, 9, 9, False, 0., True, 'refusals')
    d = c.H * c.hd

    def refused(word, **over):
        b = Buffers(dev, c, 'padded')
        rc = b.backward(**over)
        torch.cuda.synchronize()
        assert rc != 0 and word in _err(), (word, over, rc, _err())
        assert all(nan_like_bits(buf).all() for buf in b.grad_bufs), (word, over)
        return b

    b = Buffers(dev, c, 'padded')
    ld, bs, nb = b.ld, b.bs, _lib().sf_slate_attention_bwd_workspace_bytes(c.B, c.Lq, c.H)
    assert b.backward() == 0, _err()                 # the same arguments, unchanged, are accepted
    refused('head_dim', hd=18)                       # 2 * 18 = 36 columns of the 36 the rows hold
    refused('head_dim', hd=6)
    refused('16-byte aligned', ld=(ld[0] - 2, ld[1], ld[2], ld[3]))
    refused('16-byte aligned', ld=(ld[0], ld[1], ld[2], ld[3] - 2))
    refused('workspace too small', nb=nb - 1)
    refused('q_bs too small', bs=((c.Lq - 1) * ld[0] + d - 4, bs[1], bs[2], bs[3]))
    refused('Lq == Lk', causal=1, Lk=c.Lk - 2)
    refused('dropout_p', p=1.0)
    for name in ('q', 'k', 'v', 'o', 'g', 'dq', 'dk', 'dv', 'ws'):
        refused('null pointer', **{name: None})
    # the alignment the 16-byte loads of q and d_out assume: the base address and the batch stride
    refused('q and d_out must be 16-byte aligned', q=b.q.data_ptr() + 4)
    refused('q and d_out must be 16-byte aligned', g=b.g.data_ptr() + 8)
    refused('batch strides', bs=(bs[0] - 2, bs[1], bs[2], bs[3]))
    refused('batch strides', bs=(bs[0], bs[1], bs[2], bs[3] - 1))
