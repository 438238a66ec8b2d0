"""GPU: the Physion VQA readout kernels (csrc/physion_readout.hip) and what is built on them, against the float64 restatements of
tests/physion_readout_cases.py.

Forward tolerance (the rule of tests/test_dvae_tokens_gpu.py): four times the distance of the float32 split-bf16 emulation from float64 for the
same case, never above 1e-3, both of the largest |logit|.  A recorded route (t_star, pair_star) is valid when the float64 value AT the recorded
place is within that bound of the float64 maximum.  Gradients are compared with the float64 restatement fed the kernel's OWN route, each tensor
within 2e-4 of its largest magnitude (the project's bound for composed results); the measured distances are printed."""
import json
import os

import numpy as np
import pytest
import torch

import physion_readout_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'physion_readout.npz')
GRAD_BOUND = 2e-4
DEV = 'cuda'


def ids(shape):
    return '-'.join(map(str, shape))


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def forward_bound(case, agg, ref):
    """absolute: min(4 x emulation distance, 1e-3) x the largest |logit|"""
    emu = cases.emulate_f32(*case, agg)
    top = np.abs(ref['logits']).max()
    d = np.abs(emu - ref['steps']).max() / top
    return min(4 * d, 1e-3) * top, d


def run_forward(case, agg, **kw):
    from slotformer_amd import ops
    slots, W1, b1, w2, b2 = dev(*case)
    out = ops.physion_readout_fwd(slots, W1, b1, w2, b2, agg, want_steps=True, want_pairs=True, **kw)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize('shape', cases.FORWARD_CASES, ids=ids)
def test_forward_and_route_against_float64(shape):
    B, T, N, C, F, K, agg = shape
    case = cases.forward_case(shape)
    ref = cases.forward64(*case, agg)
    bound, emu_d = forward_bound(case, agg, ref)
    logits, t_star, steps, pairs = run_forward(case, agg)
    assert logits.shape == (K, B) and t_star.shape == (K, B) and steps.shape == (K, B, T) and pairs.shape == (K, B, F)
    top = np.abs(ref['logits']).max()
    d_steps, d_logits = np.abs(steps - ref['steps']).max(), np.abs(logits - ref['logits']).max()
    print(f'{shape}: steps {d_steps / top:.3e}, logits {d_logits / top:.3e} (emulation {emu_d:.3e}, bound {bound / top:.3e}) of the largest |logit|')
    assert d_steps <= bound and d_logits <= bound
    # the route: the logit IS the step logit at t_star, the first of its maxima, and float64 agrees within the bound -- for every video and head
    kk, bb = np.meshgrid(np.arange(K), np.arange(B), indexing='ij')
    assert t_star.min() >= 0 and t_star.max() < T
    assert np.array_equal(logits, steps[kk, bb, t_star]) and np.array_equal(t_star, steps.argmax(2))
    assert (ref['steps'][kk, bb, t_star] >= ref['logits'] - bound).all()
    if agg != 'max':
        assert not pairs.any()
        return
    P = N * (N - 1) // 2
    assert pairs.max() < P
    for k in range(K):
        rel = ref['rel'][k][np.arange(B), t_star[k]]   # [B,pairs,F] at the recorded frame
        at = np.take_along_axis(rel, pairs[k][:, None, :].astype(np.int64), 1)[:, 0]
        assert (at >= rel.max(1) - bound).all()


@pytest.mark.parametrize('shape', cases.BACKWARD_CASES, ids=ids)
def test_backward_against_float64_at_the_recorded_route(shape):
    from slotformer_amd import ops
    B, T, N, C, F, agg = shape
    case = cases.backward_case(shape)
    slots, W1, b1, w2, b2 = dev(*case)
    logits, t_star, _, pairs = ops.physion_readout_fwd(slots, W1, b1, w2, b2, agg, want_pairs=True)
    labels = (np.random.default_rng(cases.case_seed(shape)).uniform(size=B) > 0.5).astype(np.float32)
    g = cases.dloss64(logits[0].cpu().numpy(), labels).astype(np.float32)
    got = ops.physion_readout_bwd(slots, W1, b1, w2, torch.from_numpy(g).to(DEV), t_star, agg, pair_star=pairs if agg == 'max' else None)
    again = ops.physion_readout_bwd(slots, W1, b1, w2, torch.from_numpy(g).to(DEV), t_star, agg, pair_star=None)   # the pairs found again
    want = cases.grads64(case[0], case[1][0], case[2][0], case[3][0], agg, g.astype(np.float64), t_star[0].cpu().numpy(),
                         pairs[0].cpu().numpy().astype(np.int64))
    for name, a, a2, w in zip(('dW1', 'db1', 'dw2', 'db2'), got, again, want):
        a, w = a.cpu().numpy().astype(np.float64), np.asarray(w, np.float64).reshape(a.shape)
        d = np.abs(a - w).max() / np.abs(w).max()
        print(f'{shape} {name}: {d:.3e} of the largest magnitude')
        assert d <= GRAD_BOUND, name
        assert torch.equal(a2.cpu(), torch.from_numpy(a).float()), name


def test_two_backward_runs_are_bit_identical():
    from slotformer_amd import ops
    shape = (64, 7, 6, 192, 192, 'max')
    slots, W1, b1, w2, b2 = dev(*cases.backward_case(shape))
    _, t_star, _, pairs = ops.physion_readout_fwd(slots, W1, b1, w2, b2, 'max', want_pairs=True)
    g = torch.from_numpy(np.random.default_rng(3).standard_normal(64).astype(np.float32)).to(DEV)
    for agg in cases.AGGS:
        a = torch.cat([x.flatten() for x in ops.physion_readout_bwd(slots, W1, b1, w2, g, t_star, agg, pair_star=pairs)]).clone()
        b = torch.cat([x.flatten() for x in ops.physion_readout_bwd(slots, W1, b1, w2, g, t_star, agg, pair_star=pairs)])
        assert torch.equal(a, b) and torch.isfinite(a).all(), agg


def load_fixture_model(agg):
    from slotformer_amd.physion_vqa.models import PhysionReadout
    s = cases.FIXTURE_SHAPE
    slots, W1, b1, w2, b2, labels = cases.fixture_case(agg)
    m = PhysionReadout(dict(num_slots=s['N'], slot_size=s['C'], agg_func=agg, feats_dim=s['F']))
    m.load_state_dict({'comb_idx': m.comb_idx, 'linear1.weight': torch.from_numpy(W1[0]), 'linear1.bias': torch.from_numpy(b1[0]),
                       'linear2.weight': torch.from_numpy(w2[0])[None], 'linear2.bias': torch.from_numpy(b2)})
    return m.to(DEV), (slots, W1, b1, w2, b2), labels


@pytest.mark.parametrize('agg', cases.AGGS)
def test_reference_fixture_through_the_model(agg):
    golden = np.load(GOLDEN)
    m, case, labels = load_fixture_model(agg)
    ref = cases.forward64(*case, agg)
    bound, _ = forward_bound(case, agg, ref)
    f32 = 1e-6 * np.abs(golden[f'{agg}_logits']).max()   # the fixture is float32 (tests/test_physion_readout.py holds it to float64 at 1e-6)
    data = {'slots': torch.from_numpy(case[0]).to(DEV), 'label': torch.from_numpy(labels).to(DEV)}
    out = m(data, return_steps=True)
    assert out['logits'].shape == (4, ) and out['step_logits'].shape == (4, 5) and out['logits'].requires_grad
    logits = out['logits'].detach().cpu().numpy()
    print(f'{agg}: logits {np.abs(logits - golden[f"{agg}_logits"]).max():.3e} (bound {bound:.3e})')
    assert np.abs(logits - golden[f'{agg}_logits']).max() <= bound + f32
    assert np.abs(out['step_logits'].cpu().numpy() - ref['steps'][0]).max() <= bound
    loss = m.calc_train_loss(data, out)
    assert list(loss) == ['vqa_loss'] and loss['vqa_loss'].dim() == 0
    assert abs(loss['vqa_loss'].item() - float(golden[f'{agg}_vqa_loss'])) <= bound + 1e-6 * float(golden[f'{agg}_vqa_loss'])   # BCE is 1-Lipschitz
    loss['vqa_loss'].backward()
    step = int(golden['dW1_row_step'])
    for name, got, want in (('dW1', m.linear1.weight.grad[::step], golden[f'{agg}_dW1_rows']), ('db1', m.linear1.bias.grad, golden[f'{agg}_db1']),
                            ('dw2', m.linear2.weight.grad[0], golden[f'{agg}_dw2']), ('db2', m.linear2.bias.grad, golden[f'{agg}_db2'])):
        d = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
        print(f'{agg} {name}: {d:.3e}')
        assert d <= GRAD_BOUND, name
    ev = m.calc_eval_loss(data, {'logits': out['logits'].detach()})
    assert list(ev) == ['vqa_loss'] + json.loads(str(golden[f'{agg}_acc_keys']))
    assert abs(ev['vqa_loss'].item() - loss['vqa_loss'].item()) < 1e-7
    assert np.array_equal(np.float32([ev[k].item() for k in list(ev)[1:]]), golden[f'{agg}_acc'])
    assert not ev['vqa_loss'].requires_grad
    with torch.no_grad():
        assert torch.equal(m(data)['logits'], out['logits'].detach())


def test_ties_and_planted_maxima():
    T, N = 12, 6   # (two chunks of eight timesteps)
    case = cases.seeded_case(77, 3, T, N, 192, 192)
    logits, t_star, steps, pairs = run_forward(case, 'max')
    slots = case[0]
    # two identical frames: the copy of the winning frame sits later (or, when the winner is the last frame, earlier): the FIRST of the two is reported
    dup, expect = slots.copy(), []
    for b in range(3):
        t = int(t_star[0, b])
        src, dst = (t, T - 1) if t < T - 1 else (t, 0)
        dup[b, dst] = dup[b, src]
        expect.append(min(src, dst))
    l2, t2, s2, _ = run_forward((dup, ) + case[1:], 'max')
    assert t2[0].tolist() == expect and np.array_equal(l2, logits)
    for b in range(3):
        assert (s2[0, b] == l2[0, b]).sum() == 2   # bit-equal step logits of the two copies, whatever their place in a chunk
    # a planted largest logit at frame 0 and at frame T - 1
    for place in (0, T - 1):
        moved = slots.copy()
        for b in range(3):
            t = int(t_star[0, b])
            moved[b, [t, place]] = moved[b, [place, t]]
        l3, t3, _, p3 = run_forward((moved, ) + case[1:], 'max')
        assert t3[0].tolist() == [place] * 3 and np.array_equal(l3, logits) and np.array_equal(p3, pairs)
    # two identical slots (3 = 1): the pairs (0,3), (3,4), (3,5) tie with (0,1), (1,4), (1,5) bit for bit and must never be the recorded one
    same = slots.copy()
    same[:, :, 3] = same[:, :, 1]
    ref = cases.forward64(same, *case[1:], 'max')
    bound, _ = forward_bound((same, ) + case[1:], 'max', ref)
    l4, t4, _, p4 = run_forward((same, ) + case[1:], 'max')
    pr = cases.pairs_of(N)
    later, first = [pr.index(p) for p in ((0, 3), (3, 4), (3, 5))], [pr.index(p) for p in ((0, 1), (1, 4), (1, 5))]
    assert not np.isin(p4, later).any() and np.isin(p4, first).any()
    rel = ref['rel'][0][np.arange(3), t4[0]]
    assert (np.take_along_axis(rel, p4[0][:, None, :].astype(np.int64), 1)[:, 0] >= rel.max(1) - bound).all()


def test_strided_views_and_video_index_read_only_what_they_name():
    from slotformer_amd import ops
    N, C, F = 6, 192, 192
    _, W1, b1, w2, b2 = cases.seeded_case(5, 1, 1, N, C, F)
    rng = np.random.default_rng(6)
    big = np.full((5, 150, N, C), np.nan, np.float32)
    index = [3, 1]
    big[index, :75] = rng.standard_normal((2, 75, N, C)).astype(np.float32)
    big_d, W1, b1, w2, b2 = dev(big, W1, b1, w2, b2)
    idx = torch.tensor(index, dtype=torch.int32, device=DEV)
    got = ops.physion_readout_fwd(big_d, W1, b1, w2, b2, 'max', video_index=idx, video_len=75, want_steps=True, want_pairs=True)
    tight = big_d[index, :75].contiguous()
    want = ops.physion_readout_fwd(tight, W1, b1, w2, b2, 'max', want_steps=True, want_pairs=True)
    view = ops.physion_readout_fwd(big_d[:, :75], W1, b1, w2, b2, 'max', video_index=idx, want_steps=True, want_pairs=True)
    for a, b, c in zip(got, want, view):
        assert torch.equal(a, b) and torch.equal(c, b) and not torch.isnan(a.float()).any()
    g = torch.tensor([0.3, -0.2], device=DEV)
    ga = ops.physion_readout_bwd(big_d, W1, b1, w2, g, got[1], 'max', pair_star=got[3], video_index=idx, video_len=75)
    gb = ops.physion_readout_bwd(tight, W1, b1, w2, g, want[1], 'max', pair_star=want[3])
    for a, b in zip(ga, gb):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    # repeated and unordered entries: every row is the row of that video's own run
    case = cases.seeded_case(8, 3, 9, N, C, F, K=3)
    slots, W1, b1, w2, b2 = dev(*case)
    order = [2, 0, 2, 1]
    rows = ops.physion_readout_fwd(slots, W1, b1, w2, b2, 'sum', video_index=order, want_steps=True)
    for r, v in enumerate(order):
        one = ops.physion_readout_fwd(slots, W1, b1, w2, b2, 'sum', video_index=[v], want_steps=True)
        assert torch.equal(rows[0][:, r], one[0][:, 0]) and torch.equal(rows[1][:, r], one[1][:, 0]) and torch.equal(rows[2][:, r], one[2][:, 0])
    # a video that does not exist is NaN, never an access
    bad = ops.physion_readout_fwd(slots, W1, b1, w2, b2, 'sum', video_index=[1, 3, -1])
    assert torch.isnan(bad[0][:, 1:]).all() and torch.isfinite(bad[0][:, 0]).all()


def test_score_loss_gradient_and_counts():
    from slotformer_amd import ops
    K, B, n_tasks = 3, 37, 4
    rng = np.random.default_rng(11)
    logits = (rng.standard_normal((K, B)) * 2).astype(np.float32)
    logits[0, :4] = [30., -30., 0., 88.]
    labels = (rng.uniform(size=B) > 0.5).astype(np.float32)
    task = rng.integers(0, n_tasks, B).astype(np.int32)
    threshs = (0.4, 0.45, 0.5, 0.55, 0.6, 0.65)
    lg, lb, tk = dev(logits, labels, task)
    loss, g, counts, tcounts = ops.physion_readout_score(lg, lb, threshs=threshs, task_idx=tk, n_tasks=n_tasks)
    for k in range(K):
        assert abs(loss[k].item() - cases.loss64(logits[k], labels)) <= 1e-6 * cases.loss64(logits[k], labels)
        assert np.abs(g[k].cpu().numpy() - cases.dloss64(logits[k], labels)).max() <= 1e-6 / B
    counts, tcounts = counts.cpu().numpy(), tcounts.cpu().numpy()
    assert counts.dtype == np.int32 and counts.shape == (K, 6) and tcounts.shape == (K, n_tasks, 6)
    for k in range(K):
        for i, th in enumerate(threshs):
            unsafe = int((np.abs(cases.sigmoid64(logits[k]) - float(np.float32(th))) <= 1e-6).sum())
            assert abs(int(counts[k, i]) - int(cases.hits64(logits[k], labels, th).sum())) <= unsafe
            for t in range(n_tasks):
                sel = task == t
                unsafe_t = int((np.abs(cases.sigmoid64(logits[k][sel]) - float(np.float32(th))) <= 1e-6).sum())
                assert abs(int(tcounts[k, t, i]) - int(cases.hits64(logits[k][sel], labels[sel], th).sum())) <= unsafe_t
    assert np.array_equal(tcounts.sum(1), counts)
    # ragged batches accumulate into the same counters
    acc = tacc = None
    for a, b in ((0, 16), (16, 32), (32, 37)):
        _, _, acc, tacc = ops.physion_readout_score(lg[:, a:b], lb[a:b], threshs=threshs, task_idx=tk[a:b], n_tasks=n_tasks, want_loss=False,
                                                    want_grad=False, counts=acc, task_counts=tacc)
    assert np.array_equal(acc.cpu().numpy(), counts) and np.array_equal(tacc.cpu().numpy(), tcounts)
    with pytest.raises(ValueError, match='at most 16 thresholds'):
        ops.physion_readout_score(lg, lb, threshs=[0.5] * 17)


def test_evaluate_is_the_sweep_of_single_runs():
    from slotformer_amd.physion_vqa import evaluate
    from slotformer_amd.physion_vqa.models import PhysionReadout
    V, T, N, C, F = 20, 5, 6, 64, 32
    rng = np.random.default_rng(21)
    slots = torch.from_numpy(rng.standard_normal((V, T, N, C)).astype(np.float32)).to(DEV)
    labels = torch.from_numpy((rng.uniform(size=V) > 0.5).astype(np.float32)).to(DEV)
    task = torch.from_numpy(rng.integers(0, 3, V).astype(np.int32)).to(DEV)
    heads = []
    for seed in range(3):
        torch.manual_seed(seed)
        m = PhysionReadout(dict(num_slots=N, slot_size=C, agg_func='max', feats_dim=F))
        with torch.no_grad():
            m.linear2.bias += 0.3 * seed   # (spread the heads' accuracies)
        heads.append(m)
    res = evaluate([heads[0], heads[1].state_dict(), {'state_dict': heads[2].state_dict()}], slots, labels, task_idx=task, batch_size=8)
    assert res['acc'].shape == (3, 6) and res['task_acc'].shape == (3, 3, 6)
    for k, m in enumerate(heads):
        one = evaluate(m.to(DEV), slots, labels, task_idx=task, batch_size=128)
        assert torch.equal(one['acc'][0], res['acc'][k]) and torch.equal(one['task_acc'][0], res['task_acc'][k])
    # the reference script's pick: per threshold the first best checkpoint, then the first best threshold
    acc = res['acc'].numpy()
    per_thresh = [(int(np.argmax(acc[:, i])), acc[:, i].max()) for i in range(6)]
    ti = int(np.argmax([a for _, a in per_thresh]))
    assert res['best'] == (per_thresh[ti][0], ti) and res['best_acc'] == per_thresh[ti][1]
    assert int(res['counts'].max()) <= V and np.array_equal(res['task_counts'].sum(1).numpy(), res['counts'].numpy())


def planted_set(seed=0, V=32, T=6, N=6, C=64):
    """A separable set: in a positive video one frame carries a pattern on slot 1 AND its partner on slot 4; a negative video carries nothing."""
    rng = np.random.default_rng(seed)
    slots = (0.3 * rng.standard_normal((V, T, N, C))).astype(np.float32)
    p, q = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    labels = (np.arange(V) % 2).astype(np.float32)
    for v in range(V):
        if labels[v]:
            t = int(rng.integers(0, T))
            slots[v, t, 1] += 3 * p / np.linalg.norm(p)
            slots[v, t, 4] += 3 * q / np.linalg.norm(q)
    return slots, labels


def test_fit_learns_a_planted_pair_and_is_deterministic():
    from slotformer_amd.physion_vqa import evaluate, fit
    from slotformer_amd.physion_vqa.models import PhysionReadout
    slots, labels = dev(*planted_set())

    def run(seed):
        torch.manual_seed(0)
        m = PhysionReadout(dict(num_slots=6, slot_size=64, agg_func='max', feats_dim=32)).to(DEV)
        losses = fit(m, slots, labels, epochs=50, batch_size=8, lr=1e-3, seed=seed)
        return m, losses

    m, losses = run(1)
    assert losses.shape == (50, ) and torch.isfinite(losses).all() and losses[-1] < losses[0]
    res = evaluate(m, slots, labels, threshs=(0.5, ))
    print(f'fit: loss {losses[0].item():.4f} -> {losses[-1].item():.4f}, accuracy {res["best_acc"]:.3f}')
    assert res['best_acc'] == 1.0
    m2, losses2 = run(1)
    m3, _ = run(2)
    for a, b, c in zip(m.parameters(), m2.parameters(), m3.parameters()):
        assert torch.equal(a, b)
    assert torch.equal(losses, losses2)
    assert any(not torch.equal(a, c) for a, c in zip(m.parameters(), m3.parameters()))


def test_readout_video_slots_chunks_and_pinned_host_memory():
    from slotformer_amd import harness
    from slotformer_amd.physion_vqa.models import PhysionReadout
    torch.manual_seed(3)
    m = PhysionReadout(dict(num_slots=6, slot_size=64, agg_func='mean', feats_dim=32)).to(DEV)
    slots = torch.from_numpy(np.random.default_rng(4).standard_normal((12, 80, 6, 64)).astype(np.float32))
    whole = harness.readout_video_slots(m, slots.to(DEV), 12, to_host=False)
    chunks = harness.readout_video_slots(m, slots, 5)
    assert chunks.is_pinned() and not chunks.is_cuda and chunks.shape == (12, ) and chunks.dtype == torch.float32
    assert whole.is_cuda and torch.equal(whole.cpu(), chunks)
    assert (chunks > 0).all() and (chunks < 1).all()
    want = torch.sigmoid(m({'slots': slots[:, :75].to(DEV)})['logits']).cpu()
    assert torch.equal(want, chunks)
    short = harness.readout_video_slots(m, slots, 7, video_len=3)
    assert torch.equal(short, torch.sigmoid(m({'slots': slots[:, :3].to(DEV)})['logits']).cpu())
