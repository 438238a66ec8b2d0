"""The OBJ3D rollout (d_model 128, 8 heads of 16, ffn 512; 6 + 10 frames of 6 slots) with the three layers before the last as ONE token-stationary launch
per step (sf_rollout_opts.layer_tok; csrc/layer_tok128.hip) against the generic GEMM path (layer_tok off: the path every OBJ3D rollout took before the
kernel existed, bit for bit -- the baseline).  hipGraph replays of the two forms ALTERNATE in one process on one card, both warmed; every timed window
lasts at least --window seconds; --rounds rounds; median and spread (max - min) per form, and the max relative difference of the two outputs.

    python tools/rollout_tok128_probe.py [B ...] [--rounds 3] [--window 0.5]      (default batches 32 64 192 512)"""
import argparse
import os
import statistics
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from slotformer_amd import configs, engine  # noqa: E402
from slotformer_amd.build import source_tree_hash  # noqa: E402
from slotformer_amd.video_prediction.models import SlotRollouter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('batches', nargs='*', type=int, default=[32, 64, 192, 512])
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--window', type=float, default=0.5)
args = ap.parse_args()

dev = torch.device('cuda:0')
rd = configs.C1_ROLL['rollout_dict']
HIST, PRED, N, CS = rd['history_len'], 10, rd['num_slots'], rd['slot_size']
torch.manual_seed(0)
roll = SlotRollouter(**rd).eval().to(dev)
TOK, GEN = {'layer_tok': True}, {'layer_tok': False}


def capture(buf, opts):
    for _ in range(2):
        engine.rollout(roll, buf, HIST, PRED, opts=opts)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        engine.rollout(roll, buf, HIST, PRED, opts=opts)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def window_ms(g, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


print(f'source tree {source_tree_hash()}   {torch.cuda.get_device_name(0)}   OBJ3D rollout {HIST} + {PRED} frames x {N} slots, '
      f'{args.rounds} alternating rounds, windows >= {args.window} s')
print('| videos | layer_tok on: ms / rollout (us / step) | spread | layer_tok off: ms / rollout (us / step) | spread | off / on | max rel diff |')
print('|---|---|---|---|---|---|---|')
with torch.no_grad():
    for B in args.batches:
        torch.manual_seed(B)
        x0 = torch.randn(B, HIST, N, CS, device=dev)

        def fresh():
            buf = torch.zeros(B, HIST + PRED, N, CS, device=dev)
            buf[:, :HIST] = x0
            return buf

        a = engine.rollout(roll, fresh(), HIST, PRED, opts=TOK).clone()
        b = engine.rollout(roll, fresh(), HIST, PRED, opts=GEN).clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(a).all())
        diff = ((a - b).abs().max() / b.abs().max()).item()
        buf_t, buf_g = fresh(), fresh()
        g_t, g_g = capture(buf_t, TOK), capture(buf_g, GEN)
        n_t = max(10, int(args.window / (window_ms(g_t, 10) * 1e-3)) + 1)
        n_g = max(10, int(args.window / (window_ms(g_g, 10) * 1e-3)) + 1)
        ms_t, ms_g = [], []
        for _ in range(args.rounds):
            ms_t.append(window_ms(g_t, n_t))
            ms_g.append(window_ms(g_g, n_g))
        mt, mg = statistics.median(ms_t), statistics.median(ms_g)
        print(f'| {B} | {mt:.3f} ({mt * 1e3 / PRED:.1f}) | {max(ms_t) - min(ms_t):.3f} | {mg:.3f} ({mg * 1e3 / PRED:.1f}) | {max(ms_g) - min(ms_g):.3f} | '
              f'{mg / mt:.2f} | {diff:.1e} |', flush=True)
