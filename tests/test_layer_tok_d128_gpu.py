"""Token-stationary whole-layer launches for the OBJ3D Transformer -- d_model 128, 8 heads of 16, ffn 512 (csrc/layer_tok128.hip; sf_rollout_opts.layer_tok
on the generic rollout path).  Kernel level against a float64 PyTorch restatement of the layer (slotformer.py:72-80); the rollout with them against the
REFERENCE's fixture, against the committed CPU restatement at a larger batch, captured into a graph; the plan predicate against what ran."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import golden_util as gu

pytestmark = pytest.mark.gpu

D, NH, FFN = 128, 8, 512


def _rollouter(dev, seed=3):
    from slotformer_amd.video_prediction.models import SlotRollouter
    torch.manual_seed(seed)
    r = SlotRollouter(**dict(gu.C1_ROLL['rollout_dict'])).eval().to(dev)
    with torch.no_grad():   # biases / LayerNorm parameters away from their (zero / one) initial values: a wrong index must show
        for p in r.parameters():
            if p.dim() == 1:
                p.add_(0.3 * torch.randn_like(p))
    return r


def _layer64(layer, x):
    """x [B, L, 128] -> the layer in float64"""
    d = lambda t: t.detach().double()  # noqa: E731
    xx = x.double()
    B, L, Dm = xx.shape
    h = F.layer_norm(xx, (Dm, ), d(layer.norm1.weight), d(layer.norm1.bias))
    q, k, v = F.linear(h, d(layer.self_attn.in_proj_weight), d(layer.self_attn.in_proj_bias)).split(Dm, dim=-1)
    hd = lambda t: t.reshape(B, L, 8, 16).transpose(1, 2)  # noqa: E731
    a = torch.softmax(hd(q) @ hd(k).transpose(-1, -2) / 16 ** 0.5, dim=-1) @ hd(v)
    x2 = xx + F.linear(a.transpose(1, 2).reshape(B, L, Dm), d(layer.self_attn.out_proj.weight), d(layer.self_attn.out_proj.bias))
    h2 = F.layer_norm(x2, (Dm, ), d(layer.norm2.weight), d(layer.norm2.bias))
    return x2 + F.linear(F.relu(F.linear(h2, d(layer.linear1.weight), d(layer.linear1.bias))), d(layer.linear2.weight), d(layer.linear2.bias))


@pytest.fixture
def process_defaults():
    """split-bf16, token-stationary layers off -- restored afterwards"""
    from slotformer_amd import _lib
    lib = _lib.lib()
    old = lib.sf_get_precision(), lib.sf_get_layer_tok()
    lib.sf_set_precision(1)
    lib.sf_set_layer_tok(0)
    yield lib
    lib.sf_set_precision(old[0])
    lib.sf_set_layer_tok(old[1])


# (videos, tokens per video): the OBJ3D window (36: three videos per 128-token workgroup, 20 padding rows) at the probe's batches, a single video, a
# last workgroup with one video (4); one key block per video (8, 16, 32), two videos per workgroup (50 would put a wave's keys in four blocks: one), 64;
# one video per workgroup with idle waves (65, 90, 96)
@pytest.mark.parametrize('B,L', [(32, 36), (64, 36), (192, 36), (1, 36), (3, 36), (4, 36), (2, 6), (4, 24), (35, 16), (256, 8), (9, 32), (5, 64), (4, 50),
                                 (2, 90), (3, 96), (1, 65)])
@pytest.mark.parametrize('nl', [1, 3])
@torch.no_grad()
def test_layer_tok_d128_block_vs_float64(dev, process_defaults, B, L, nl):
    from slotformer_amd import _lib, engine
    lib = _lib.lib()
    r = _rollouter(dev)
    plan = engine.rollouter_plan(r)
    st = torch.cuda.current_stream().cuda_stream
    x = gu.seeded_normal((B, L, D), 100 * B + L).to(dev)
    ref = x
    for k in range(nl):
        ref = _layer64(r.transformer_encoder.layers[k], ref)
    y = torch.full((B, L, D), float('nan'), device=dev)
    _lib.check(lib.sf_layer_tok_block_ex_f32(plan.struct.layers, nl, D, NH, FFN, x.data_ptr(), y.data_ptr(), B, L, st))
    torch.cuda.synchronize()
    err = ((y.double() - ref).abs().max() / ref.abs().max()).item()
    print(f'd128 B {B} L {L} layers {nl}: rel err vs float64 {err:.2e}')
    assert err < 1e-5      # the bar of the same three-pass arithmetic at d 256 (test_layer_tok_gpu.py); NaN (an unwritten row) fails it
    # the other sequences of a call do not matter (a workgroup holds several; keys of other sequences are masked): replace all but one
    if B >= 2:
        x2 = gu.seeded_normal((B, L, D), 7).to(dev)
        keep = B // 2
        x2[keep] = x[keep]
        y2 = torch.empty_like(y)
        _lib.check(lib.sf_layer_tok_block_ex_f32(plan.struct.layers, nl, D, NH, FFN, x2.data_ptr(), y2.data_ptr(), B, L, st))
        torch.cuda.synchronize()
        assert torch.equal(y2[keep], y[keep])
    y3 = torch.empty_like(y)
    _lib.check(lib.sf_layer_tok_block_ex_f32(plan.struct.layers, nl, D, NH, FFN, x.data_ptr(), y3.data_ptr(), B, L, st))
    torch.cuda.synchronize()
    assert torch.equal(y3, y)


@torch.no_grad()
def test_layer_tok_d128_argument_errors(dev, process_defaults):
    """Refused arguments only: nothing here launches."""
    from slotformer_amd import _lib, engine
    lib = _lib.lib()
    r = _rollouter(dev)
    plan = engine.rollouter_plan(r)
    layers = plan.struct.layers
    x = torch.zeros(2, 97, D, device=dev)
    y = torch.full_like(x, 5.0)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda nl, shape, L: lib.sf_layer_tok_block_ex_f32(layers, nl, *shape, x.data_ptr(), y.data_ptr(), 2, L, st)  # noqa: E731
    assert call(1, (D, NH, FFN), 97) != 0      # more than 96 tokens per sequence
    assert call(0, (D, NH, FFN), 36) != 0      # no layer
    assert call(9, (D, NH, FFN), 36) != 0      # more than 8 layers per launch
    assert call(1, (128, 4, 512), 36) != 0     # neither supported shape
    assert call(1, (64, 8, 256), 36) != 0
    lib.sf_set_precision(0)
    assert call(1, (D, NH, FFN), 36) != 0      # split-bf16 mode only
    lib.sf_set_precision(1)
    torch.cuda.synchronize()
    assert bool((y == 5.0).all())
    assert lib.sf_layer_tok_packed_bytes_ex(128, 4, 512) == 0 and lib.sf_layer_tok_packed_bytes_ex(64, 8, 256) == 0
    assert lib.sf_layer_tok_packed_bytes_ex(256, 8, 1024) == lib.sf_layer_tok_packed_bytes()
    assert 0 < lib.sf_layer_tok_packed_bytes_ex(D, NH, FFN) < lib.sf_layer_tok_packed_bytes()
    bad = torch.empty(16, dtype=torch.uint8, device=dev)
    assert lib.sf_pack_layer_tok_weights(layers, bad.data_ptr(), 128, 4, 512, st) != 0
    assert lib.sf_rollout_tok_ok(C.byref(plan.struct)) == 0 and lib.sf_rollout_is_fused(C.byref(plan.struct)) == 0


def _fixture_rollout(dev):
    from test_engine_gpu import build
    from slotformer_amd import engine
    name, cfg, B, pred_len, seed = 'roll_c1', gu.C1_ROLL, 3, 10, 201
    g = gu.load_golden(name)
    m, _ = build(cfg, g, seed, dev, vp=True)
    rd = cfg['rollout_dict']
    hist, N, Cs = rd['history_len'], rd['num_slots'], rd['slot_size']
    T_in = engine.burn_in_of(m.rollouter)
    slots = gu.seeded_normal((B, hist + pred_len, N, Cs), seed + 1).to(dev)
    buf = torch.zeros(B, T_in + pred_len, N, Cs, device=dev)
    buf[:, :T_in] = slots[:, :T_in]
    return m, g, buf, T_in, pred_len


@torch.no_grad()
def test_rollout_obj3d_with_layer_tok_vs_reference_fixture(dev, process_defaults):
    """The OBJ3D rollout (6 + 10, three videos) with the three layers before the last in ONE token-stationary launch per step against the reference's own
    outputs, and against the generic path: d > 0 is what shows that the new form ran."""
    from slotformer_amd import engine
    m, g, buf, T_in, pred_len = _fixture_rollout(dev)
    engine.rollout(m.rollouter, buf, T_in, pred_len, opts={'layer_tok': True})
    ref = torch.as_tensor(g['pred_slots']).to(dev)
    e = ((buf[:, T_in:] - ref).abs().max() / ref.abs().max()).item()
    other = buf.clone()
    other[:, T_in:] = 0
    engine.rollout(m.rollouter, other, T_in, pred_len, opts={'layer_tok': False})
    d = ((buf - other).abs().max() / ref.abs().max()).item()
    print('roll_c1 token-stationary layers vs the reference fixture', e, ' vs the generic path', d)
    assert e < 5e-5 and 0 < d < 5e-5


@torch.no_grad()
def test_rollout_obj3d_64_videos_vs_cpu_restatement_and_graph(dev, process_defaults):
    import oracle
    from slotformer_amd import engine
    from slotformer_amd.video_prediction.models import SlotRollouter
    rd = gu.C1_ROLL['rollout_dict']
    torch.manual_seed(11)
    roll = SlotRollouter(**rd).eval()
    rsd = {'rollouter.' + k: v.clone() for k, v in roll.state_dict().items()}
    B, hist, N, Cs, pred_len = 64, rd['history_len'], rd['num_slots'], rd['slot_size'], 10
    x = gu.seeded_normal((B, hist, N, Cs), 12)
    ref = oracle.rollouter_forward(x, pred_len, rsd, rd)
    roll = roll.to(dev)

    def fresh():
        buf = torch.zeros(B, hist + pred_len, N, Cs, device=dev)
        buf[:, :hist] = x.to(dev)
        return buf

    buf = fresh()
    engine.rollout(roll, buf, hist, pred_len, opts={'layer_tok': True})
    torch.cuda.synchronize()
    e = ((buf[:, hist:].cpu() - ref).abs().max() / ref.abs().max()).item()
    print('OBJ3D 64 videos x (6 + 10), token-stationary layers vs the CPU restatement', e)
    assert e < 5e-5
    # the same call captured into a graph on one stream, replayed twice: the bits of the eager call
    gbuf = fresh()
    engine.rollout(roll, gbuf, hist, pred_len, opts={'layer_tok': True})   # (warm: workspace and packed copies exist before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (one capture stream: the rollout is one chain of launches)
        engine.rollout(roll, gbuf, hist, pred_len, opts={'layer_tok': True})
    for _ in range(2):
        gbuf[:, hist:] = 0
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gbuf, buf)


@torch.no_grad()
def test_rollout_tok_layers_agrees_with_what_ran(dev, process_defaults):
    from slotformer_amd import engine
    lib = process_defaults
    m, g, buf, T_in, pred_len = _fixture_rollout(dev)
    plan = engine.rollouter_plan(m.rollouter)
    B = buf.shape[0]
    count = lambda o: lib.sf_rollout_tok_layers(C.byref(plan.struct), B, C.byref(engine.rollout_opts(o)))  # noqa: E731
    assert count({'layer_tok': True}) == 3
    assert count({'layer_tok': False}) == 0
    assert count({'layer_tok': True, 'precision': 'f32'}) == 0
    assert lib.sf_rollout_tok_layers(C.byref(plan.struct), B, None) == 0

    def run(o):
        b = buf.clone()
        engine.rollout(m.rollouter, b, T_in, pred_len, opts=o)
        return b

    generic = run({'layer_tok': False})
    assert not torch.equal(run({'layer_tok': True}), generic)                       # three layers ran in another form
    assert torch.equal(run(None), generic)                                           # the process default is off
    assert torch.equal(run({'layer_tok': True, 'precision': 'f32'}), run({'layer_tok': False, 'precision': 'f32'}))   # 0 layers: the same path
    lib.sf_set_layer_tok(1)
    assert lib.sf_rollout_tok_layers(C.byref(plan.struct), B, None) == 3
    assert torch.equal(run(None), run({'layer_tok': True}))
