"""One library (SF_LIB_PATH picks it) per process: a 3-layer token-stationary launch of 64 workgroups (192 videos, L = 42) on a stream masked to 128 CUs
 - alone,
 - two such streams side by side (the two rollout units of the pipeline's 'pair' partition),
 - beside conv5x5_ws_kernel looping on the complementary 128 CUs (the encode lane of the pipeline),
and alone on the whole chip: us per launch, median (min - max) of ROUNDS rounds of N back-to-back launches between device events.  With SF_DBG=lt and a
-DLT_STAMPS build also the shader cycles of workgroup 0's wave 0 over the first layer of the last launch and the clock they imply.

    [SF_LIB_PATH=...] [SF_DBG=lt] python tools/layer_tok_shape_probe.py [tag]      (profiles/layer_tok_mfma_shape.md)"""
import ctypes as C
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402
import golden_util as gu  # noqa: E402
from slotformer_amd import _lib, engine, ops  # noqa: E402
from slotformer_amd.pipeline import ENC_WORDS_P, ROLL_WORDS_P  # noqa: E402
from slotformer_amd.video_prediction.models import SlotRollouter  # noqa: E402

TAG = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.environ.get('SF_LIB_PATH', 'library'))
ROUNDS, N, NL, B, L = int(os.environ.get('LT_ROUNDS', '7')), 50, 3, 192, 42
dev = torch.device('cuda:0')
lib = _lib.lib()
torch.manual_seed(3)
r = SlotRollouter(**dict(gu.C2_ROLL['rollout_dict'])).eval().to(dev)
plan = engine.rollouter_plan(r)


def masked(words):
    h = C.c_void_p()
    _lib.check(lib.sf_stream_create_cu_mask(C.byref(h), (C.c_uint * 8)(*words), 8))
    return torch.cuda.ExternalStream(h.value, device=dev)


roll = [masked(ROLL_WORDS_P), masked(ROLL_WORDS_P)]
lane = masked(ENC_WORDS_P)
whole = torch.cuda.Stream(dev)
xs = [torch.randn(B, L, 256, device=dev) for _ in range(2)]
ys = [torch.empty_like(x) for x in xs]
x64 = torch.relu(torch.randn(192, 64, 64, 64, device=dev))
wf = ops.pack_conv_frag(ops.pack_conv_weight(0.05 * torch.randn(64, 64, 5, 5, device=dev)))
cb = 0.1 * torch.randn(64, device=dev)


def launches(k, st, n=N):
    for _ in range(n):
        _lib.check(lib.sf_layer_tok_block_f32(plan.struct.layers, NL, xs[k].data_ptr(), ys[k].data_ptr(), B, L, st.cuda_stream))


def timed(streams, background=0):
    """us per launch on each of `streams` (launched together); `background` convolution launches queued on the lane first"""
    torch.cuda.synchronize()
    el = torch.cuda.Event(enable_timing=True)
    if background:
        with torch.cuda.stream(lane):
            for _ in range(background):
                ops.conv5x5_ws(x64, wf, cb)
            el.record(lane)
    evs = []
    for k, st in enumerate(streams):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        launches(k, st)
        e1.record(st)
        evs.append((e0, e1))
    torch.cuda.synchronize()
    busy = evs[-1][1].elapsed_time(el) > 0 if background else None    # the background outlasted the timed launches
    return [a.elapsed_time(b) * 1e3 / N for a, b in evs], busy


def report(name, streams, background=0):
    vals, still = [], True
    for _ in range(ROUNDS):
        t, busy = timed(streams, background)
        vals += t
        still = still and busy is not False
    print(f'{TAG:12s} {name:44s} {statistics.median(vals):7.1f} ({min(vals):.1f} - {max(vals):.1f}) us per launch'
          + ('' if still else '   (the background ended before the timed launches did)'), flush=True)
    if os.environ.get('LT_ALL'):
        print(' ' * 13 + 'rounds: ' + ' '.join(f'{v:.1f}' for v in vals), flush=True)


with torch.no_grad():
    for k in range(2):
        launches(k, roll[k], 10)
    ops.conv5x5_ws(x64, wf, cb)
    torch.cuda.synchronize()
    report('128 CUs, alone', roll[:1])
    report('128 CUs, two units side by side', roll)
    report('128 CUs, conv5x5_ws on the other 128', roll[:1], background=70)
    report('whole chip, alone', [whole])
    if 'lt' in os.environ.get('SF_DBG', ''):
        for name, streams, bg in (('alone', roll[:1], 0), ('beside conv5x5_ws', roll[:1], 70)):
            timed(streams, bg)
            ts = (C.c_longlong * 16)()
            lib.sf_debug_read_ts_layer_tok(ts)
            att, ffn = ts[8] + ts[9] + ts[10], ts[11] + ts[12] + ts[13] - (ts[8] + ts[9] + ts[10])
            wa, wf_ = (ts[4] - ts[2]) / 100, (ts[6] - ts[4]) / 100    # us (the wall clock counts 100 MHz); LN1 .. C_8, LN2 .. last slice
            print(f'{TAG:12s} stamps {name:18s} attention block {att} cycles (DMA waits {ts[8]}, barrier waits {ts[9]}) in {wa:.1f} us; FFN block {ffn} cycles '
                  f'(DMA waits {ts[11] - ts[8]}, barrier waits {ts[12] - ts[9]}) in {wf_:.1f} us; implied clock {(att + ffn) / (wa + wf_) / 1e3:.2f} GHz', flush=True)
