"""PHYRE planning measurements (profiles/phyre_planning.md).   python tools/bench_phyre_planning.py [--json PATH] [--md PATH] [--seconds 0.5]

On one GPU, at the reference shape (readout_phyre_params-fold0.py: 8 slots of 128, sel_slots [0, 3], 4 layers of d 128 / 8 heads / ffn 512, 17
tokens per action), on seeded weights and slots:

  * the readout alone at B 128 and B 1024 -- `PHYREReadout.logits_of` (three launches: embed, the layers, the head) and the same three launches
    straight on the C entry point with a preallocated workspace (`reps` calls back to back, so that the wrapper's host time is not counted) --
    against a torch-eager restatement of the same model in this project's own words (index -> linear -> cat -> per layer layer_norm, linear,
    softmax attention, linear, layer_norm, linear, relu, linear -> linear, relu, linear) and against torch's own nn.TransformerEncoder module on
    the same parameters, on the same device; with the largest distance of the three from each other;
  * the readout's share of one `harness.phyre_plan` chunk: 128 first frames at 128 x 128 through the C5 models (PHYRE SAVi + SingleStepSlotFormer,
    seeded weights), encode -> 3 rollout steps -> readout, the whole call against the readout on its slots.

The paths alternate call by call after a warm-up of each, timed with device events until each has run for `--seconds`; medians, with the minimum
and maximum.  No GPU: the tool fails, it measures nothing."""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402
import torch.nn.functional as tnf  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, seconds, min_calls=5, max_calls=2000):
    """{name: [ms, ...]} of the callables run in turn until every one has run for `seconds`."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    while (min(sum(v) for v in ts.values()) < seconds * 1e3 or len(next(iter(ts.values()))) < min_calls) and len(next(iter(ts.values()))) < max_calls:
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    return ts


def stats(v):
    return {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4), 'calls': len(v)}


def eager_tokens(m, slots):
    """[B, 1 + T N, d]: CLS, then the projected slots of the selected frames + their frame's position row (t-major, slot-minor)"""
    x = m.in_proj(slots[:, list(m.sel_slots)]) + m.enc_t_pe[0][None, :, None, :]
    return torch.cat([m.CLS.expand(x.shape[0], 1, -1), x.flatten(1, 2)], 1)


@torch.no_grad()
def eager_readout(m, slots):
    """PHYREReadout.forward on torch operators, one call per step of the definition."""
    x = eager_tokens(m, slots)
    B, L, D = x.shape
    for layer in m.transformer_encoder.layers:
        h = tnf.layer_norm(x, (D, ), layer.norm1.weight, layer.norm1.bias, 1e-5)
        q, k, v = tnf.linear(h, layer.self_attn.in_proj_weight, layer.self_attn.in_proj_bias).split(D, -1)
        nh = layer.self_attn.num_heads
        sp = lambda t: t.reshape(B, L, nh, D // nh).transpose(1, 2)  # noqa: E731
        a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / (D // nh) ** 0.5, -1) @ sp(v)
        x = x + tnf.linear(a.transpose(1, 2).reshape(B, L, D), layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias)
        h = tnf.layer_norm(x, (D, ), layer.norm2.weight, layer.norm2.bias, 1e-5)
        x = x + tnf.linear(torch.relu(tnf.linear(h, layer.linear1.weight, layer.linear1.bias)), layer.linear2.weight, layer.linear2.bias)
    return m.cls_mlp(x[:, 0]).squeeze(1)


@torch.no_grad()
def module_readout(m, slots):
    """the same with torch's nn.TransformerEncoder module (whichever path torch takes for it in eval mode)"""
    return m.cls_mlp(m.transformer_encoder(eager_tokens(m, slots))[:, 0]).squeeze(1)


def planning_models(dev):
    import golden_util as gu
    from slotformer_amd.base_slots import build_model as bb
    from slotformer_amd.video_prediction import build_model as bv
    torch.manual_seed(77)
    savi = bb(gu.ParamsView(gu.C5_SAVI))
    path = os.path.join(tempfile.mkdtemp(), 'savi.pth')
    torch.save({'state_dict': savi.state_dict()}, path)
    rcfg = copy.deepcopy(gu.C5_ROLL)
    rcfg['dec_dict'] = dict(gu.C5_SAVI['dec_dict'], dec_ckp_path=path)
    sf = bv(gu.ParamsView(rcfg))
    savi.testing = True
    return savi.eval().to(dev), sf.eval().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None)
    ap.add_argument('--seconds', type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_phyre_planning: no GPU; nothing is measured without one')
    import golden_util as gu
    import phyre_readout_cases as cases
    from slotformer_amd import engine, harness
    from slotformer_amd._lib import lib, check
    from slotformer_amd.phyre_planning import frame_table
    from slotformer_amd.phyre_planning.models import PHYREReadout
    import ctypes as C
    dev = torch.device('cuda:0')
    rd = cases.readout_dict()
    m = PHYREReadout(rd)
    m.load_state_dict(cases.seeded_weights(rd, 1))
    m = m.eval().to(dev)
    N, Cs, T_all = rd['num_slots'], rd['slot_size'], 4
    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'readout_dict': rd}
    plan = engine.phyre_readout_plan(m)
    stream, reps = torch.cuda.current_stream().cuda_stream, 20
    sel = (C.c_int * 2)(*rd['sel_slots'])
    for B in (128, 1024):
        slots = torch.from_numpy(cases.seeded_slots(B, B, T_all, N, Cs)).to(dev)
        logits = torch.empty(B, device=dev)
        ws = torch.empty(int(lib().sf_phyre_readout_workspace_bytes(B, N, 2)), dtype=torch.uint8, device=dev)

        def entry():
            for _ in range(reps):
                check(lib().sf_phyre_readout_fwd_f32(slots.data_ptr(), slots.stride(0), slots.stride(1), B, T_all, None, sel, m.in_proj.weight.data_ptr(),
                                                     m.in_proj.bias.data_ptr(), m.enc_t_pe.data_ptr(), m.CLS.data_ptr(), plan.layers, 4, 128, 8, 512,
                                                     m.cls_mlp[0].weight.data_ptr(), m.cls_mlp[0].bias.data_ptr(), m.cls_mlp[2].weight.data_ptr(),
                                                     m.cls_mlp[2].bias.data_ptr(), logits.data_ptr(), None, None, None, 0, B, 2, N, Cs, ws.data_ptr(),
                                                     ws.numel(), stream))

        def eager_reps():
            for _ in range(reps):
                eager_readout(m, slots)

        def module_reps():
            for _ in range(reps):
                module_readout(m, slots)

        ts = alternate({'native_wrapper': lambda: m.logits_of(slots), 'eager': lambda: eager_readout(m, slots),
                        'torch_module': lambda: module_readout(m, slots)}, a.seconds)
        sec = {k: stats(v) for k, v in ts.items()}
        ts = alternate({'native_entry_point': entry, 'eager_back_to_back': eager_reps, 'torch_module_back_to_back': module_reps}, a.seconds)
        sec.update({k: stats([t / reps for t in v]) for k, v in ts.items()})
        nat, eag, mod = m.logits_of(slots)[0], eager_readout(m, slots), module_readout(m, slots)
        sec['max_abs_difference'] = {'native_vs_eager': float((nat - eag).abs().max()), 'module_vs_eager': float((mod - eag).abs().max()),
                                     'largest_abs_logit': float(eag.abs().max())}
        sec['eager_over_native'] = {'calls': round(sec['eager']['median_ms'] / sec['native_wrapper']['median_ms'], 2),
                                    'back_to_back': round(sec['eager_back_to_back']['median_ms'] / sec['native_entry_point']['median_ms'], 2),
                                    'module_back_to_back': round(sec['torch_module_back_to_back']['median_ms'] / sec['native_entry_point']['median_ms'], 2)}
        res[f'readout_B{B}'] = sec

    # ---- the readout's share of one phyre_plan chunk ----
    B = 128
    savi, sf = planning_models(dev)
    frames = gu.seeded_img(B, 1, 128, seed=9).to(dev)
    table = frame_table(rd['sel_slots'])
    slots = harness.extract_and_rollout(savi, sf.rollouter, frames, max(rd['sel_slots']), batch_size=B)
    ts = alternate({'phyre_plan_chunk': lambda: harness.phyre_plan(savi, sf, m, frames, batch_size=B, to_host=False),
                    'readout_on_its_slots': lambda: m.logits_of(slots, sel=table)}, a.seconds)
    sec = {k: stats(v) for k, v in ts.items()}
    sec['readout_share'] = round(sec['readout_on_its_slots']['median_ms'] / sec['phyre_plan_chunk']['median_ms'], 4)
    res['plan_chunk_B128'] = sec
    harness.release_pipelines()

    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(text + '\n')
    if a.md:
        rows = ['| measurement | path | median ms | min - max ms | calls |', '|---|---|---|---|---|']
        for name in ('readout_B128', 'readout_B1024', 'plan_chunk_B128'):
            for k, s in res[name].items():
                if isinstance(s, dict) and 'median_ms' in s:
                    rows.append(f"| {name} | {k} | {s['median_ms']} | {s['min_ms']} - {s['max_ms']} | {s['calls']} |")
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, 'w') as f:
            f.write(f"Measured by `tools/bench_phyre_planning.py` on {res['device']} (torch {res['torch']}).\n\n" + '\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
