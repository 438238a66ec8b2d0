"""STEVE render measurements (profiles/steve_render.md).   python tools/bench_steve_render.py [--md profiles/steve_render.md] [--json PATH] [--reps 3]

At the Physion decoder shape (V 4096, d 192, 4 heads of 48, 4 blocks, 6 slots) and 1024 token steps:

  * microseconds per token step of greedy generation, for B in {1, 12, 64, 192} frames: the launch chain (`sf_slate_generate_f32`, the code
    `generate_cached` runs: unchanged by the one-launch step, so it is the number to beat) and the one-launch step (`sf_slate_generate_tok_f32`,
    csrc/slate_step.hip) at 1, 2 and 4 frames per workgroup.  Both are called through the C ABI on the same buffers, no logits written, so that
    nothing but the generation loop is inside the timed window;
  * milliseconds per frame of `steve_render.render_slots` (hard only, and hard + soft) beside `STEVESlotFormer.decode` -- the method body as it
    stands, bound to the same decoder and dVAE -- at 12 and 64 frames of 128 x 128.

All forms run in the same process, alternating call by call after a warm-up of each, timed with device events around whole calls.  The tables replace the
text between the two `bench_steve_render` marker lines of the --md file.  `--counter-run` does one fused generation (12 frames, one frame per
workgroup) and nothing else: the command a counter pass (rocprofv3 --pmc FETCH_SIZE, in a run of its own: tools/pmc_cmd.sh) is made over.
No GPU: the tool fails, it measures nothing."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

BEGIN, END = '<!-- bench_steve_render:begin -->', '<!-- bench_steve_render:end -->'
SHAPE = (4096, 192, 4, 1023, 6, 4)   # V, d, heads, max_len, slots, blocks
STEPS = 1024
FORMS = (0, 1, 2, 4)                 # 0: the launch chain; else frames per workgroup of the one-launch step


def step_bytes(B, fr):
    """bytes one token step must stream, from the shapes: (the weights once per workgroup, this workgroup's K/V at the mean prefix length)"""
    V, d, _, _, _, L = SHAPE
    weights = 4 * (L * 14 * d * d + V * d)
    kv_mean = 4 * L * 2 * d * (STEPS / 2)
    wgs = -(-B // fr)
    return weights, kv_mean * fr, wgs * weights + B * kv_mean


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Generator:
    """both generation forms on one set of buffers"""

    def __init__(self, dec, B, steps):
        from slotformer_amd._lib import lib
        self.lib, self.dec, self.B, self.steps = lib(), dec, B, steps
        self.keep = dec._slate_plan()
        self.m = self.keep.struct
        dev = dec.head.weight.device
        self.slots = torch.randn(B, SHAPE[4], SHAPE[1], generator=torch.Generator().manual_seed(B)).to(dev)
        self.tokens = torch.zeros(B, steps, dtype=torch.int64, device=dev)
        self.nb = self.lib.sf_slate_generate_tok_workspace_bytes(C.byref(self.m), B, steps)
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=dev)

    def run(self, form, steps=None):
        from slotformer_amd._lib import check
        steps = steps or self.steps
        st = torch.cuda.current_stream().cuda_stream
        if form == 0:
            check(self.lib.sf_slate_generate_f32(C.byref(self.m), self.slots.data_ptr(), self.B, steps, self.tokens.data_ptr(), None,
                                                 self.ws.data_ptr(), self.nb, st))
        else:
            ran = C.c_int(-1)
            check(self.lib.sf_slate_generate_tok_f32(C.byref(self.m), self.slots.data_ptr(), self.B, steps, self.tokens.data_ptr(), None, form,
                                                     self.ws.data_ptr(), self.nb, st, C.byref(ran)))
            assert ran.value == form, (ran.value, form)


def measure_generation(dec, B, reps):
    g = Generator(dec, B, STEPS)
    toks = {}
    for f in FORMS:                      # warm-up of every form at this shape: the same kernels, a short run
        g.run(f, 48)
    torch.cuda.synchronize()
    times = {f: [] for f in FORMS}
    for r in range(reps):
        for f in FORMS:
            times[f].append(timed(lambda: g.run(f)))
            if r == 0:
                toks[f] = g.tokens.clone()
    row = {'B': B, 'steps': STEPS, 'reps': reps}
    chain = statistics.median(times[0])
    for f in FORMS:
        name = 'chain' if f == 0 else f'fused_fr{f}'
        med = statistics.median(times[f])
        row[name + '_us_per_step'] = round(med * 1e3 / STEPS, 1)
        row[name + '_min_max'] = [round(min(times[f]) * 1e3 / STEPS, 1), round(max(times[f]) * 1e3 / STEPS, 1)]
        if f:
            row[name + '_over_chain'] = round(med / chain, 3)
            row[name + '_token_mismatch'] = int((toks[f] != toks[0]).sum())   # near ties between fp32 forms may flip a token; random weights
    print(json.dumps(row), flush=True)
    return row


def measure_render(dec, dvae, F_, reps):
    from slotformer_amd import steve_render
    from slotformer_amd.video_prediction.models.steve_slotformer import STEVESlotFormer
    dev = dec.head.weight.device
    slots = torch.randn(F_, SHAPE[4], SHAPE[1], generator=torch.Generator().manual_seed(100 + F_)).to(dev)
    # STEVESlotFormer.decode as it stands, on the same two networks
    shim = types.SimpleNamespace(decoder=dec, dvae=dvae, num_patches=STEPS, h=32, w=32)
    shim._token_map = types.MethodType(STEVESlotFormer._token_map, shim)
    forms = {'decode': lambda: STEVESlotFormer.decode(shim, slots),
             'render_hard': lambda: steve_render.render_slots(dec, dvae, slots),
             'render_soft': lambda: steve_render.render_slots(dec, dvae, slots, soft=True, seed=1)}
    # warm-up: the generation kernels on a short run, the dVAE stack and the softmax at full size through one call of each form
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            times[k].append(timed(fn))
    row = {'frames': F_, 'reps': reps, 'fused_form': dec.last_generate_form}
    for k in forms:
        row[k + '_ms_per_frame'] = round(statistics.median(times[k]) / F_, 2)
        row[k + '_min_max'] = [round(min(times[k]) / F_, 2), round(max(times[k]) / F_, 2)]
    print(json.dumps(row), flush=True)
    return row


def tables(gen, ren, device_name):
    out = [f'Measured by `tools/bench_steve_render.py` on {device_name} (torch {torch.__version__}); medians of alternating whole calls '
           f'({STEPS} token steps each), device events.', '',
           '| frames B | chain us/step (min - max) | fused, 1 frame/WG | fused, 2 frames/WG | fused, 4 frames/WG | fused / chain (1, 2, 4) | '
           'tokens differing from the chain (1, 2, 4) | calls each |', '|---|---|---|---|---|---|---|---|']
    for r in gen:
        cell = lambda n: f"{r[n + '_us_per_step']} ({r[n + '_min_max'][0]} - {r[n + '_min_max'][1]})"   # noqa: E731
        out.append(f"| {r['B']} | {cell('chain')} | {cell('fused_fr1')} | {cell('fused_fr2')} | {cell('fused_fr4')} | "
                   f"{r['fused_fr1_over_chain']}, {r['fused_fr2_over_chain']}, {r['fused_fr4_over_chain']} | "
                   f"{r['fused_fr1_token_mismatch']}, {r['fused_fr2_token_mismatch']}, {r['fused_fr4_token_mismatch']} of {r['B'] * STEPS} | {r['reps']} |")
    out += ['', '| frames | `STEVESlotFormer.decode` ms/frame (min - max) | `render_slots` hard ms/frame | `render_slots` hard + soft ms/frame | '
            'generation form of render | calls each |', '|---|---|---|---|---|---|']
    for r in ren:
        cell = lambda n: f"{r[n + '_ms_per_frame']} ({r[n + '_min_max'][0]} - {r[n + '_min_max'][1]})"   # noqa: E731
        form = 'launch chain' if r['fused_form'] == 0 else f"one launch per token, {r['fused_form']} frame(s) per workgroup"
        out.append(f"| {r['frames']} | {cell('decode')} | {cell('render_hard')} | {cell('render_soft')} | {form} | {r['reps']} |")
    w, kv1, _ = step_bytes(1, 1)
    out += ['', f'From the shapes: a step streams {w / 1e6:.1f} MB of weights into every workgroup and, at the mean prefix length, '
            f'{kv1 / 1e6:.2f} MB of cached keys and values per frame.']
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=os.path.join(ROOT, 'profiles', 'steve_render.md'))
    ap.add_argument('--json', default=None)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--batches', default='1,12,64,192')
    ap.add_argument('--render-frames', default='12,64')
    ap.add_argument('--counter-run', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_steve_render: no GPU; nothing is measured without one')
    from slotformer_amd.base_slots.models.dVAE import dVAE
    from slotformer_amd.base_slots.models.steve_transformer import STEVETransformerDecoder
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    dec = STEVETransformerDecoder(*SHAPE).eval().to(dev)
    with torch.no_grad():
        if a.counter_run:
            g = Generator(dec, 12, STEPS)
            g.run(1)
            torch.cuda.synchronize()
            print('counter run done: 12 frames, 1 frame per workgroup,', STEPS, 'steps')
            return
        dvae = dVAE(SHAPE[0]).eval().to(dev)
        gen = [measure_generation(dec, int(b), a.reps) for b in a.batches.split(',') if b]
        ren = [measure_render(dec, dvae, int(f), max(2, a.reps - 1)) for f in a.render_frames.split(',') if f]
    text = tables(gen, ren, torch.cuda.get_device_name(0))
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump({'generation': gen, 'render': ren}, f, indent=1)
    if a.md and os.path.exists(a.md):
        src = open(a.md).read()
        if BEGIN in src and END in src:
            src = src[:src.index(BEGIN) + len(BEGIN)] + '\n' + text + '\n' + src[src.index(END):]
            with open(a.md, 'w') as f:
                f.write(src)


if __name__ == '__main__':
    main()
