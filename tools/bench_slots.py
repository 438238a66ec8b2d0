"""What more slots cost (profiles/slots16.md): the Slot-Attention iteration in each of its forms, the encode and the StoSAVi training step at
7, 8 (the 8-slot instantiations) and 9, 11, 16 slots (the 16-slot instantiations).

  python tools/bench_slots.py [--what iter,encode,train] [--reps 5]

  iter   : microseconds per launch, 32 frames x 4096 keys of slot size 128 -- one-pass tile kernel (keys == values), two-pass MFMA kernel on the
           same rows (9 .. 16 slots: sf_set_slot_attn_tile16(0); up to 8: a second copy of the rows, i.e. twice the unique bytes) and on separate
           key / value rows, VALU kernel (4080 keys: no multiple of 256), and the backward
  encode : milliseconds per StoSAVi encode of 32 videos x 6 frames at 128 x 128 (the CLEVRER form of configs.C2_SAVI at N slots)
  train  : milliseconds per training step of the CLEVRER form at 64 x 64, 16 clips x 6 frames (tools/bench_train_savi.py's step) at 7 and 11 slots

Every figure: device work between two synchronisations, `inner` launches per window after a warm-up of the same shape, the window repeated
`--reps` times with the shapes interleaved; median and the min .. max spread of the windows.  One JSON line per figure."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

import golden_util as gu  # noqa: E402
from slotformer_amd import _lib  # noqa: E402

SLOTS = (7, 8, 9, 11, 16)


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def measure(cases, inner, reps, unit, scale):
    """cases: {name: fn}.  Warm every shape up, then `reps` rounds over all of them (interleaved: a drift of the box hits every case alike)."""
    for fn in cases.values():
        window(fn, max(3, inner // 10))
    times = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            times[k].append(window(fn, inner) * scale)
    for k, v in times.items():
        print(json.dumps({'case': k, 'unit': unit, 'median': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2),
                          'windows': reps, 'launches_per_window': inner}), flush=True)


class tile16:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = _lib.lib().sf_get_slot_attn_tile16()
        _lib.lib().sf_set_slot_attn_tile16(self.on)

    def __exit__(self, *exc):
        _lib.lib().sf_set_slot_attn_tile16(self.old)


def bench_iter(dev, reps):
    """(the C entry points on preallocated buffers: the launches are ~20 us, a torch.empty per call would show in them)"""
    lib = _lib.lib()
    B, HW, D = 32, 4096, 128
    x, x2, v = (torch.randn(B, HW, D, device=dev) for _ in range(3))
    x2.copy_(x)
    xv, vv = torch.randn(B, 4080, D, device=dev), torch.randn(B, 4080, D, device=dev)
    dk, dv = torch.empty_like(x), torch.empty_like(x)
    st = torch.cuda.current_stream().cuda_stream
    keep = []

    def fwd(k, val, q, pn, pd, N):
        hw = k.shape[1]
        return lambda: _lib.check(lib.sf_slot_attn_iter_f32(k.data_ptr(), val.data_ptr(), D, hw * D, q.data_ptr(), pn.data_ptr(), pd.data_ptr(), None,
                                                            B, hw, N, D, D**-0.5, 1e-6, st))

    cases = {}
    for N in SLOTS:
        q, du, dq = (torch.randn(B, N, D, device=dev) for _ in range(3))
        P = lib.sf_slot_attn_num_partials(HW)
        pn, pd = torch.empty(B, P, N, D, device=dev), torch.empty(B, P, N, device=dev)
        pnv, pdv = torch.empty(B, 64, N, D, device=dev), torch.empty(B, 64, N, device=dev)
        same = fwd(x, x, q, pn, pd, N)

        def two_pass_same_rows(N=N, same=same, other=fwd(x, x2, q, pn, pd, N)):
            if N <= 8:
                return other()
            with tile16(0):
                return same()
        bwd_bytes, bwd = ((lib.sf_slot_attn_iter_bwd_workspace_bytes, lib.sf_slot_attn_iter_bwd_f32) if N <= 8 else
                          (lib.sf_slot_attn_iter_bwd16_workspace_bytes, lib.sf_slot_attn_iter_bwd16_f32))
        nb = bwd_bytes(B, HW, N, D)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        pnb, pdb = torch.empty(B, P, N, D, device=dev), torch.empty(B, P, N, device=dev)
        fwd(x, v, q, pnb, pdb, N)()   # the records the backward reads
        keep.append((q, du, dq, pn, pd, pnv, pdv, ws, pnb, pdb))
        cases[f'iter N={N} tile (keys == values)'] = same
        cases[f'iter N={N} two-pass, the same rows'] = two_pass_same_rows
        cases[f'iter N={N} two-pass, separate k / v'] = fwd(x, v, q, pn, pd, N)
        cases[f'iter N={N} VALU (4080 keys)'] = fwd(xv, vv, q, pnv, pdv, N)
        cases[f'iter N={N} backward'] = lambda q=q, du=du, dq=dq, ws=ws, nb=nb, pnb=pnb, pdb=pdb, bwd=bwd, N=N: _lib.check(bwd(
            x.data_ptr(), v.data_ptr(), D, HW * D, q.data_ptr(), pnb.data_ptr(), pdb.data_ptr(), P, du.data_ptr(), dk.data_ptr(), dv.data_ptr(), 0,
            dq.data_ptr(), B, HW, N, D, D**-0.5, 1e-6, ws.data_ptr(), nb, st))
    measure(cases, 200, reps, 'us per launch', 1e6)


def bench_encode(dev, reps):
    from slotformer_amd.base_slots import build_model
    B, T = 32, 6
    img = torch.rand(B, T, 3, 128, 128, device=dev) * 2 - 1
    cases = {}
    for N in SLOTS:
        torch.manual_seed(0)
        m = build_model(gu.ParamsView(gu.savi_cfg(128, N, iters=2, kernel_mlp=False, pred='mlp', rnn=False, kld='var-0.01'))).eval().to(dev)
        m.testing = True
        data = {'img': img, 'noise': torch.randn(B, T, N, 128, device=dev)}

        @torch.no_grad()
        def run(m=m, data=data):
            return m(data)['post_slots']

        @torch.no_grad()
        def run_two_pass(m=m, data=data):
            with tile16(0):
                return m(data)['post_slots']
        cases[f'encode N={N}'] = run
        if N > 8:
            cases[f'encode N={N}, two-pass iterations'] = run_two_pass
    measure(cases, 10, reps, 'ms per encode of 32 x 6 frames at 128 px', 1e3)


def bench_train(dev, reps):
    from slotformer_amd.base_slots import build_model
    B, T = 16, 6
    img = torch.rand(B, T, 3, 64, 64, device=dev) * 2 - 1
    cases = {}
    for N in (7, 11):
        torch.manual_seed(0)
        m = build_model(gu.ParamsView(gu.savi_cfg(64, N, iters=2, kernel_mlp=False, pred='mlp', rnn=False, kld='var-0.01'))).to(dev).train()
        m.testing = False
        data = {'img': img, 'noise': torch.randn(B, T, N, 128, device=dev)}
        opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4)

        def step(m=m, data=data, opt=opt):
            opt.zero_grad(set_to_none=True)
            out = m(data)
            terms = m.calc_train_loss(data, out)
            (terms['post_recon_loss'] + 1e-4 * terms['kld_loss']).backward()
            opt.step()
        cases[f'train step N={N}'] = step
    measure(cases, 10, reps, 'ms per training step, 16 clips x 6 frames at 64 px', 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='iter,encode,train')
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_slots.py measures on a GPU; none found')
    dev = torch.device('cuda:0')
    for what in a.what.split(','):
        {'iter': bench_iter, 'encode': bench_encode, 'train': bench_train}[what](dev, a.reps)


if __name__ == '__main__':
    main()
