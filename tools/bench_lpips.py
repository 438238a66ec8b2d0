"""LPIPS measurements (profiles/lpips.md).   python tools/bench_lpips.py [--md profiles/lpips.md] [--json PATH] [--seconds 1.0]

At 32 videos x 50 steps of 128 x 128 (1600 pairs, in chunks of 32) and at one step of 32 pairs:

  * milliseconds per call of `slotformer_amd.lpips.LPIPS.distances` (csrc/lpips.hip);
  * the algorithm's FLOPs -- 2 * 9 * Cin * Cout per output pixel of the thirteen convolutions, both images of every pair, computed from the shapes
    below -- over that time, and that rate as a fraction of the split-bf16 MFMA roof (2500 / 3 TFLOP/s: three bf16 MFMA flops per algorithmic flop);
  * the same network restated with torch's own float32 convolutions (F.conv2d / F.max_pool2d, the vendor libraries) on the same GPU and the same
    chunks: what a user without this library would run.

Both paths run in the same process, alternating call by call after a warm-up of each, timed with device events until each has run for at least
`--seconds`.  The table replaces the text between the two `bench_lpips` marker lines of the --md file.  No GPU: the tool fails, it measures nothing."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

BEGIN, END = '<!-- bench_lpips:begin -->', '<!-- bench_lpips:end -->'
ROOF_TFLOPS = 2500.0 / 3


def flops_per_pair(H, W):
    """FLOPs of the thirteen convolutions on the two images of a pair (the taps and pools are not counted)"""
    from slotformer_amd.lpips import CONVS
    first_of_stage = {'slice1': 0, 'slice2': 1, 'slice3': 2, 'slice4': 3, 'slice5': 4}
    fl = 0
    for s, _, cin, cout in CONVS:
        k = first_of_stage[s]
        fl += 2 * 9 * cin * cout * (H >> k) * (W >> k)
    return 2 * fl


def torch_lpips(sd, x, y, chunk):
    """the definition through torch's float32 operators, in the same chunks; sd: the module's state dict on the device"""
    from slotformer_amd.lpips import CONVS, TAP_CHANNELS
    out = []
    for f0 in range(0, x.shape[0], chunk):
        a = torch.cat([x[f0:f0 + chunk], y[f0:f0 + chunk]])
        n = a.shape[0] // 2
        a = (a - sd['scaling_layer.shift']) / sd['scaling_layer.scale']
        total, prev = 0., 'slice1'
        for i, (s, idx, _, _) in enumerate(CONVS):
            if s != prev:
                total = total + _tap(a, n, sd[f'lin{int(prev[-1]) - 1}.model.1.weight'])
                a = F.max_pool2d(a, 2, 2)
                prev = s
            a = F.relu(F.conv2d(a, sd[f'net.{s}.{idx}.weight'], sd[f'net.{s}.{idx}.bias'], padding=1))
        total = total + _tap(a, n, sd[f'lin{len(TAP_CHANNELS) - 1}.model.1.weight'])
        out.append(total)
    return torch.cat(out)


def _tap(a, n, w):
    nx = a[:n] / (a[:n].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    ny = a[n:] / (a[n:].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return (w * (nx - ny) ** 2).sum(1).mean((1, 2))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(model, sd, F_, H, W, chunk, seconds):
    dev = next(model.parameters()).device
    g = torch.Generator(device='cpu').manual_seed(F_)
    x = (torch.rand(F_, 3, H, W, generator=g) * 2 - 1).to(dev)
    y = (x + 0.1 * torch.randn(F_, 3, H, W, generator=g).to(dev)).clamp(-1, 1)
    out = torch.empty(F_, device=dev)
    hip = lambda: model.distances(x, y, out=out, chunk=chunk)   # noqa: E731
    ref = lambda: torch_lpips(sd, x, y, chunk)                  # noqa: E731
    print(f'[{F_} pairs {H}x{W}] warm-up: hip', flush=True)
    for _ in range(2):
        hip()
    torch.cuda.synchronize()
    print(f'[{F_} pairs {H}x{W}] warm-up: torch', flush=True)
    with torch.no_grad():
        for _ in range(2):
            r = ref()
        torch.cuda.synchronize()
        agree = ((out - r).abs() / r.abs()).max().item()
        print(f'[{F_} pairs {H}x{W}] max rel |hip - torch f32| {agree:.2e}; timing', flush=True)
        th, tt = [], []
        while sum(th) < seconds * 1e3 or sum(tt) < seconds * 1e3 or len(th) < 5:
            th.append(timed(hip))
            tt.append(timed(ref))
    fl = flops_per_pair(H, W) * F_
    mh, mt = statistics.median(th), statistics.median(tt)
    row = {'pairs': F_, 'H': H, 'W': W, 'chunk': chunk, 'calls_each': len(th), 'gflop_per_call': round(fl / 1e9, 1),
           'hip_ms': round(mh, 3), 'hip_ms_min_max': [round(min(th), 3), round(max(th), 3)], 'hip_tflops': round(fl / mh / 1e9, 1),
           'hip_frac_of_bf16x3_roof': round(fl / mh / 1e9 / ROOF_TFLOPS, 3),
           'torch_f32_ms': round(mt, 3), 'torch_f32_ms_min_max': [round(min(tt), 3), round(max(tt), 3)], 'torch_f32_tflops': round(fl / mt / 1e9, 1),
           'hip_over_torch_time': round(mh / mt, 3), 'max_rel_hip_vs_torch_f32': agree}
    print(json.dumps(row), flush=True)
    return row


def table(rows, device_name):
    lines = [f'Measured by `tools/bench_lpips.py` on {device_name} (torch {torch.__version__}); medians of alternating calls, device events.', '',
             '| pairs x H x W (chunk) | GFLOP per call | HIP ms (min - max) | HIP TFLOP/s | fraction of the split-bf16 roof | torch f32 ms (min - max) | '
             'torch TFLOP/s | HIP time / torch time | calls each |', '|---|---|---|---|---|---|---|---|---|']
    for r in rows:
        lines.append(f"| {r['pairs']} x {r['H']} x {r['W']} ({r['chunk']}) | {r['gflop_per_call']} | {r['hip_ms']} ({r['hip_ms_min_max'][0]} - "
                     f"{r['hip_ms_min_max'][1]}) | {r['hip_tflops']} | {r['hip_frac_of_bf16x3_roof']} | {r['torch_f32_ms']} "
                     f"({r['torch_f32_ms_min_max'][0]} - {r['torch_f32_ms_min_max'][1]}) | {r['torch_f32_tflops']} | {r['hip_over_torch_time']} | "
                     f"{r['calls_each']} |")
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=os.path.join(ROOT, 'profiles', 'lpips.md'))
    ap.add_argument('--json', default=None)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--chunk', type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_lpips: no GPU; nothing is measured without one')
    from slotformer_amd.lpips import LPIPS
    dev = torch.device('cuda:0')
    model = LPIPS().to(dev)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    rows = [measure(model, sd, 32, 128, 128, a.chunk, a.seconds), measure(model, sd, 32 * 50, 128, 128, a.chunk, a.seconds)]
    text = table(rows, torch.cuda.get_device_name(0))
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)
    if a.md and os.path.exists(a.md):
        src = open(a.md).read()
        if BEGIN in src and END in src:
            src = src[:src.index(BEGIN) + len(BEGIN)] + '\n' + text + '\n' + src[src.index(END):]
            with open(a.md, 'w') as f:
                f.write(src)


if __name__ == '__main__':
    main()
