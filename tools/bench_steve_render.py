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
No GPU: the tool fails, it measures nothing.

`--soft` measures the head epilogues of the fused step instead (profiles/steve_render_soft.md), at 12 and 64 frames, every pair of forms in one
process in alternating windows of `--window` seconds (1 s or more) of whole calls:
  (a) microseconds per token step, greedy against greedy + soft rows (C ABI, no logits written); with `--other-lib PATH` also the greedy step of
      another build of the library (the parent commit's) in the same alternation;
  (b) milliseconds per soft frame, `render_slots(soft=True, fused=True)` against `render_slots(soft=True)`;
  (c) `torch.cuda.max_memory_allocated` of one call of each;
  (d) 64 sampled steps, `generate(sample=True, seed=...)` (the fused step) against `generate(sample=True)` (prefix re-run + torch.multinomial)."""
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


def windows(forms, window_s, rounds):
    """forms: name -> callable.  `rounds` alternating windows per form, each of whole calls until window_s seconds have passed (at least two calls);
    returns name -> list of per-window mean milliseconds per call"""
    import time
    out = {k: [] for k in forms}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in forms.items():
            t0, n, ms = time.perf_counter(), 0, 0.
            while n < 2 or time.perf_counter() - t0 < window_s:
                ms += timed(fn)
                n += 1
            out[k].append(ms / n)
    return out


def summary(v, scale=1.0, nd=1):
    return {'median': round(statistics.median(v) * scale, nd), 'min': round(min(v) * scale, nd), 'max': round(max(v) * scale, nd), 'windows': len(v)}


def measure_soft(dec, dvae, B, window_s, rounds, other_lib):
    from slotformer_amd import steve_render
    from slotformer_amd._lib import SIGNATURES, check, sf_slate_step_opts
    g = Generator(dec, B, STEPS)
    dev = dec.head.weight.device
    table = dvae.conv0_table()
    rows = torch.empty(B, STEPS, 64, device=dev)
    o = sf_slate_step_opts()
    o.soft_rows, o.conv0_t, o.conv0_width, o.soft_scale, o.soft_seed = rows.data_ptr(), table.data_ptr(), 64, 10.0, 1
    st = torch.cuda.current_stream().cuda_stream

    def soft_step():
        check(g.lib.sf_slate_generate_tok_opts_f32(C.byref(g.m), g.slots.data_ptr(), B, STEPS, g.tokens.data_ptr(), None, 1, g.ws.data_ptr(), g.nb,
                                                   st, None, C.byref(o)))

    forms = {'greedy': lambda: g.run(1), 'greedy_soft': soft_step}
    if other_lib:
        h = C.CDLL(other_lib)
        fn = h.sf_slate_generate_tok_f32
        fn.restype, fn.argtypes = SIGNATURES['sf_slate_generate_tok_f32']

        def other():
            assert fn(C.byref(g.m), g.slots.data_ptr(), B, STEPS, g.tokens.data_ptr(), None, 1, g.ws.data_ptr(), g.nb, st, None) == 0

        forms['greedy_other_lib'] = other
    row = {'frames': B, 'steps': STEPS, 'window_s': window_s}
    for k, v in windows(forms, window_s, rounds).items():
        row[k + '_us_per_step'] = summary(v, 1e3 / STEPS)
    g.run(1)
    greedy_tokens = g.tokens.clone()
    soft_step()
    row['tokens_equal_with_soft_rows'] = bool(torch.equal(g.tokens, greedy_tokens))
    # (b), (c): whole soft frames
    slots = g.slots
    del g, rows
    render = {'unfused': lambda: steve_render.render_slots(dec, dvae, slots, soft=True, seed=1),
              'fused': lambda: steve_render.render_slots(dec, dvae, slots, soft=True, seed=1, fused=True)}
    for k, v in windows(render, window_s, rounds).items():
        row['render_soft_' + k + '_ms_per_frame'] = summary(v, 1.0 / B, 2)
    for k, fn in render.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        row['render_soft_' + k + '_peak_MiB'] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
        del out
    a, b = render['unfused'](), render['fused']()
    row['soft_image_fused_vs_unfused_rel_err'] = float((a['soft'] - b['soft']).abs().max() / a['soft'].abs().max())
    del a, b
    # (d) 64 sampled steps
    sampled = {'fused_step': lambda: dec.generate(slots, 64, sample=True, temperature=1.0, seed=3),
               'prefix_rerun': lambda: dec.generate(slots, 64, sample=True, temperature=1.0)}
    for k, v in windows(sampled, window_s, rounds).items():
        row['sample64_' + k + '_ms'] = summary(v, 1.0, 2)
    print(json.dumps(row), flush=True)
    return row


def soft_tables(rows, device_name, other):
    cell = lambda d: f"{d['median']} ({d['min']} - {d['max']})"   # noqa: E731
    out = [f'Measured by `tools/bench_steve_render.py --soft` on {device_name} (torch {torch.__version__}): every pair of forms in one process, in '
           f"alternating windows of {rows[0]['window_s']} s of whole calls; medians over the windows (min - max of the window means), device events.", '',
           '| frames | greedy us/step | greedy + soft rows us/step | ' + ('greedy, other build us/step | ' if other else '') +
           'soft frame, unfused ms | soft frame, fused ms | peak MiB unfused | peak MiB fused | 64 sampled steps, fused step ms | prefix re-run ms |',
           '|---|---|---|' + ('---|' if other else '') + '---|---|---|---|---|---|']
    for r in rows:
        out.append(f"| {r['frames']} | {cell(r['greedy_us_per_step'])} | {cell(r['greedy_soft_us_per_step'])} | " +
                   (f"{cell(r['greedy_other_lib_us_per_step'])} | " if other else '') +
                   f"{cell(r['render_soft_unfused_ms_per_frame'])} | {cell(r['render_soft_fused_ms_per_frame'])} | "
                   f"{r['render_soft_unfused_peak_MiB']} | {r['render_soft_fused_peak_MiB']} | {cell(r['sample64_fused_step_ms'])} | "
                   f"{cell(r['sample64_prefix_rerun_ms'])} |")
    return '\n'.join(out)


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
    ap.add_argument('--soft', action='store_true')
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--other-lib', default=None)
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
        if a.soft:
            if a.window < 1.0:
                raise SystemExit('bench_steve_render --soft: windows of 1 s or more')
            rows = [measure_soft(dec, dvae, int(f), a.window, a.rounds, a.other_lib) for f in a.render_frames.split(',') if f]
            text = soft_tables(rows, torch.cuda.get_device_name(0), bool(a.other_lib))
            print(text)
            if a.json:
                os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
                with open(a.json, 'w') as f:
                    json.dump({'soft': rows, 'table': text}, f, indent=1)
            return
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
