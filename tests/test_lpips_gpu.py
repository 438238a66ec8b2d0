"""GPU: the LPIPS kernels (csrc/lpips.hip) against the float64 restatement of tests/lpips_cases.py, their exact properties (zero on equal
inputs, independence of batch position and chunking, run-to-run equality), and the wiring into pred_eval_step / pred_eval_step_device.

Bound: per case, the device may lie from float64 four times as far as the float32 emulation of its arithmetic does on the same inputs (computed
here, on the CPU), and never further than the project's parity bar of 1e-3.  Measured on an MI355X: profiles/lpips.md."""
import pytest
import torch

import lpips_cases as lc

pytestmark = pytest.mark.gpu

PARITY = 1e-3
# (pairs, H, W, chunk).  The convolution's tile is 64 flattened pixels per wave and 256 per workgroup, the tap's 256 pixels of one image:
#   16 x 16    stages of 16, 8, 4, 2 and 1 pixels a side
#   20 x 28    odd sizes under the floor of the pool (5 x 7 -> 2 x 3 -> 1 x 1)
#   32 x 32
#   36 x 70    3 pairs: 6 * 2520 pixels = 236.25 wave tiles and 59.06 workgroup tiles, 9.84 tap tiles per image; the later stages (18 x 35, 9 x 17,
#              4 x 8, 2 x 4) are ragged too.  Three pairs, so that the bound -- a maximum over the pairs -- does not hang on one lucky pair
#   128 x 128  2 pairs: the workload's own map sizes (128, 64, 32, 16, 8)
#   16 x 16    5 pairs in chunks of 2: the ragged last chunk
CASES = [(2, 16, 16, None), (2, 20, 28, None), (2, 32, 32, None), (3, 36, 70, None), (2, 128, 128, None), (5, 16, 16, 2)]


@pytest.fixture(scope='module')
def model(dev):
    from slotformer_amd.lpips import LPIPS
    m = LPIPS()
    m.load_state_dict(lc.seeded_weights(0))
    return m.to(dev)


def bound_of(ref, emu):
    return min(4. * lc.rel(emu, ref), PARITY)


@pytest.mark.parametrize('n,H,W,chunk', CASES, ids=[f'{n}x{H}x{W}' + (f'-chunk{c}' if c else '') for n, H, W, c in CASES])
def test_matches_float64(dev, model, n, H, W, chunk):
    _, x, y, ref, emu = lc.case(n, H, W)
    got = model.distances(x.to(dev), y.to(dev), chunk=chunk).cpu()
    d, bound = lc.rel(got, ref), bound_of(ref, emu)
    print(f'\nlpips {n}x{H}x{W} chunk {chunk}: max rel |device - float64| {d:.3e}  bound {bound:.3e}  (emulation {lc.rel(emu, ref):.3e}, '
          f'device vs emulation {lc.rel(got, emu):.3e})')
    assert got.shape == (n, ) and got.dtype == torch.float32
    assert d <= bound


def test_forward_shape_and_perceptual_dist(dev, model):
    from slotformer_amd.video_prediction.vp_utils import perceptual_dist
    _, x, y, ref, emu = lc.case(2, 16, 16)
    out = model(x.to(dev), y.to(dev))
    assert out.shape == (2, 1, 1, 1)
    assert torch.equal(out.flatten(), model.distances(x.to(dev), y.to(dev)))
    pd = perceptual_dist(x.to(dev), y.to(dev), model)
    assert abs(pd.item() - ref.mean().item()) <= bound_of(ref, emu) * ref.mean().item() + 1e-7 * ref.mean().item()   # + the f32 mean


def test_identical_inputs_give_exactly_zero(dev, model):
    for n, H, W in ((2, 16, 16), (1, 36, 70)):
        x, _ = lc.frames(n, H, W)
        got = model.distances(x.to(dev), x.to(dev).clone())
        assert torch.equal(got.cpu(), torch.zeros(n))


def test_bitwise_independence_of_batch_chunk_and_run(dev, model):
    _, x, y, _, _ = lc.case(5, 16, 16)
    x, y = x.to(dev), y.to(dev)
    full = model.distances(x, y, chunk=5).clone()
    assert torch.equal(full, model.distances(x, y, chunk=5))            # two runs
    assert torch.equal(full, model.distances(x, y, chunk=2))            # chunks of 2, 2, 1
    for i in range(5):
        assert torch.equal(full[i:i + 1], model.distances(x[i:i + 1], y[i:i + 1])), i
    # a pair's score does not depend on its neighbours either: pairs 3 and 1 side by side
    idx = torch.tensor([3, 1], device=dev)
    assert torch.equal(full[idx], model.distances(x[idx], y[idx]))
    # and at a size where a wave's tile spans two images (20 x 28: 560 pixels per image)
    _, x2, y2, _, _ = lc.case(2, 20, 28)
    x2, y2 = x2.to(dev), y2.to(dev)
    both = model.distances(x2, y2)
    assert torch.equal(both[1:], model.distances(x2[1:], y2[1:]))


def test_normalize_flag(dev, model):
    _, x, y, ref, emu = lc.case(2, 32, 32)
    got = model.distances(((x + 1) / 2).to(dev), ((y + 1) / 2).to(dev), normalize=True).cpu()
    d, bound = lc.rel(got, ref), bound_of(ref, emu)
    print(f'\nlpips normalize=True 2x32x32: max rel |device - float64| {d:.3e}  bound {bound:.3e}')
    assert d <= bound


def test_pred_eval_step_takes_the_module(dev, model):
    from slotformer_amd.video_prediction import vp_utils as vu
    B, T = 2, 3
    x, y = lc.frames(B * T, 32, 32, seed=5)
    gt, pred = x.view(B, T, 3, 32, 32).to(dev), y.view(B, T, 3, 32, 32).to(dev)
    per_pair = model.distances(gt.view(-1, 3, 32, 32), pred.view(-1, 3, 32, 32)).cpu().double().view(B, T)
    with_lp = vu.pred_eval_step(gt, pred, model, eval_traj=False)
    without = vu.pred_eval_step(gt, pred, None, eval_traj=False)
    want = [sum(per_pair[b, t].item() for b in range(B)) / B for t in range(T)]   # summed in the order of b, in double
    assert with_lp['percept_dist'] == want
    assert without['percept_dist'] == [0.] * T
    for m in vu.METRICS:
        assert with_lp[m] == without[m], m
    # any other callable keeps the per-step path: the same module behind a lambda gives the per-step float32 means
    wrapped = vu.pred_eval_step(gt, pred, lambda a, b: model(a, b), eval_traj=False)
    for t in range(T):
        assert wrapped['percept_dist'][t] == float(model(gt[:, t], pred[:, t]).mean())
        assert abs(wrapped['percept_dist'][t] - want[t]) <= 1e-6 * want[t]
    for m in vu.METRICS:
        assert wrapped[m] == without[m], m


def test_pred_eval_step_device_gains_two_keys(dev, model):
    from slotformer_amd.video_prediction import vp_utils as vu
    B, T = 2, 3
    x, y = lc.frames(B * T, 32, 32, seed=5)
    gt, pred = x.view(B, T, 3, 32, 32).to(dev), y.view(B, T, 3, 32, 32).to(dev)
    plain = {k: v.clone() for k, v in vu.pred_eval_step_device(gt, pred, eval_traj=False).items()}
    out = vu.pred_eval_step_device(gt, pred, eval_traj=False, lpips=model)
    assert set(out) == set(plain) | {'percept_dist', 'percept_dist_per_video'}
    assert 'percept_dist' not in plain
    for k, v in plain.items():
        assert torch.equal(out[k], v, ), k
    per_pair = model.distances(gt.view(-1, 3, 32, 32), pred.view(-1, 3, 32, 32)).double().view(B, T)
    assert out['percept_dist_per_video'].dtype == torch.float64 and torch.equal(out['percept_dist_per_video'], per_pair)
    assert out['percept_dist'].shape == (T, ) and torch.equal(out['percept_dist'], (per_pair[0] + per_pair[1]) / 2)


def test_plan_is_rebuilt_after_load_state_dict(dev):
    from slotformer_amd.lpips import LPIPS
    _, x, y, ref0, emu0 = lc.case(2, 16, 16)
    m = LPIPS()
    m.load_state_dict(lc.seeded_weights(0))
    m = m.to(dev)
    a = m.distances(x.to(dev), y.to(dev)).cpu()
    plan = m._plan()
    assert m.distances(x.to(dev), y.to(dev)) is not None and m._plan() is plan                    # kept while nothing changes
    _, _, _, ref1, emu1 = lc.case(2, 16, 16, 0, 1)                                                # the same frames, other weights
    m.load_state_dict(lc.seeded_weights(1))
    b = m.distances(x.to(dev), y.to(dev)).cpu()
    assert m._plan() is not plan
    assert not torch.equal(a, b)
    assert lc.rel(a, ref0) <= bound_of(ref0, emu0)
    d, bound = lc.rel(b, ref1), bound_of(ref1, emu1)
    print(f'\nlpips after load_state_dict 2x16x16: max rel |device - float64| {d:.3e}  bound {bound:.3e}')
    assert d <= bound
