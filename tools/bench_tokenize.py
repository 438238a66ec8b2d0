"""dVAE tokenisation measurements (profiles/tokenize.md).   python tools/bench_tokenize.py [--md profiles/tokenize.md] [--json PATH] [--seconds 0.5]

At the Physion shape (128 x 128 frames, vocabulary 4096, 32 x 32 tokens) and at 64 x 64, for chunks of 1, 12, 64 and 192 frames:

  * milliseconds per chunk and frames per second of `dVAE.tokenize_ids` (csrc/dvae_tokens.hip: patch embedding from NCHW, the argmax inside the
    vocabulary head) and of the unchanged `dVAE.tokenize(one_hot=False)` (patchify copy, `sf_linear_f32` logits in memory, `sf_argmax_rows_f32`);
  * the head kernel alone (`ops.linear_argmax` on the chunk's features): its milliseconds, the algorithm's FLOPs -- 2 * 64 * V per token -- over that
    time, and that rate as a fraction of the split-bf16 MFMA roof (2500 / 3 TFLOP/s: three bf16 MFMA flops per algorithmic flop);
  * the peak of device memory either path allocates during a call, above what is allocated before it (torch's allocator statistics).

Both paths run in the same process on the same GPU, alternating call by call after a warm-up of each, timed with device events until each has run
for at least `--seconds`.  The table replaces the text between the two `bench_tokenize` marker lines of the --md file.  No GPU: the tool fails, it
measures nothing."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

BEGIN, END = '<!-- bench_tokenize:begin -->', '<!-- bench_tokenize:end -->'
ROOF_TFLOPS = 2500.0 / 3
CHUNKS = (1, 12, 64, 192)
SHAPES = ((128, 4096), (64, 4096))   # (frame side, vocabulary)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_above_baseline(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return peak


@torch.no_grad()
def measure(model, res, V, chunk, seconds):
    from slotformer_amd import ops
    dev = model.device
    img = torch.randn(chunk, 3, res, res, generator=torch.Generator().manual_seed(chunk + res)).to(dev)
    tokens = chunk * (res // 4) ** 2
    feat = torch.randn(tokens, 64, generator=torch.Generator().manual_seed(1)).abs().to(dev)
    out = torch.empty(chunk, res // 4, res // 4, device=dev, dtype=torch.int16)
    head_out = torch.empty(tokens, device=dev, dtype=torch.int16)
    packed, bias = model._head_packed(), model.encoder[7].bias.detach()
    new = lambda: model.tokenize_ids(img, out=out, dtype=torch.int16)                  # noqa: E731
    old = lambda: model.tokenize(img, one_hot=False)                                   # noqa: E731
    head = lambda: ops.linear_argmax(feat, packed, bias, V, out_i16=head_out)          # noqa: E731
    for fn in (new, old, head):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    differ = int((new().long() != old()).sum())
    mem_new, mem_old = peak_above_baseline(new), peak_above_baseline(old)
    tn, to, th = [], [], []
    while sum(tn) < seconds * 1e3 or sum(to) < seconds * 1e3 or len(tn) < 5:
        tn.append(timed(new))
        to.append(timed(old))
        th.append(timed(head))
    mn, mo, mh = statistics.median(tn), statistics.median(to), statistics.median(th)
    fl = 2. * 64 * V * tokens
    row = {'res': res, 'V': V, 'chunk': chunk, 'calls_each': len(tn),
           'tokenize_ids_ms': round(mn, 4), 'tokenize_ids_ms_min_max': [round(min(tn), 4), round(max(tn), 4)], 'tokenize_ids_fps': round(chunk / mn * 1e3),
           'tokenize_ms': round(mo, 4), 'tokenize_ms_min_max': [round(min(to), 4), round(max(to), 4)], 'tokenize_fps': round(chunk / mo * 1e3),
           'new_over_old_time': round(mn / mo, 3), 'ids_differ': differ, 'tokens': tokens,
           'head_ms': round(mh, 4), 'head_tflops': round(fl / mh / 1e9, 2), 'head_frac_of_bf16x3_roof': round(fl / mh / 1e9 / ROOF_TFLOPS, 4),
           'peak_bytes_tokenize_ids': mem_new, 'peak_bytes_tokenize': mem_old}
    print(json.dumps(row), flush=True)
    return row


def mib(n):
    return f'{n / 2**20:.1f}'


def table(rows, device_name):
    lines = [f'Measured by `tools/bench_tokenize.py` on {device_name} (torch {torch.__version__}); medians of alternating calls, device events.', '',
             '| frames x side (V) | `tokenize_ids` ms (min - max) | frames/s | `tokenize` ms (min - max) | frames/s | new time / old time | '
             'head alone ms | head TFLOP/s | fraction of the split-bf16 roof | peak MiB new | peak MiB old | ids that differ | calls each |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    for r in rows:
        lines.append(f"| {r['chunk']} x {r['res']} ({r['V']}) | {r['tokenize_ids_ms']} ({r['tokenize_ids_ms_min_max'][0]} - {r['tokenize_ids_ms_min_max'][1]}) | "
                     f"{r['tokenize_ids_fps']} | {r['tokenize_ms']} ({r['tokenize_ms_min_max'][0]} - {r['tokenize_ms_min_max'][1]}) | {r['tokenize_fps']} | "
                     f"{r['new_over_old_time']} | {r['head_ms']} | {r['head_tflops']} | {r['head_frac_of_bf16x3_roof']} | {mib(r['peak_bytes_tokenize_ids'])} | "
                     f"{mib(r['peak_bytes_tokenize'])} | {r['ids_differ']} of {r['tokens']} | {r['calls_each']} |")
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=os.path.join(ROOT, 'profiles', 'tokenize.md'))
    ap.add_argument('--json', default=None)
    ap.add_argument('--seconds', type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_tokenize: no GPU; nothing is measured without one')
    from slotformer_amd.base_slots.models.dVAE import dVAE
    dev = torch.device('cuda:0')
    rows = []
    for res, V in SHAPES:
        torch.manual_seed(0)
        model = dVAE(V).eval().to(dev)
        with torch.no_grad():
            model.encoder[7].bias.normal_(0., 0.1)
        for chunk in CHUNKS:
            rows.append(measure(model, res, V, chunk, a.seconds))
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
