"""GPU: CLEVRER VQA on the device (csrc/aloe.hip + the library's GEMM) -- the Aloe forward against the float64 restatement of
tests/clevrer_vqa_cases.py at every shape edge and against the REFERENCE's fixture, answers compared exactly (every case clears the bar:
tests/test_clevrer_vqa.py), in-place reads, dead padding, determinism, the score kernel's bookkeeping against the numpy restatement of
calc_eval_loss, harness.clevrer_answers against the module called batch by batch, and the plan's rebuild after a weight change.  The bound on the
logits is the project's 1e-3 relative bar (measured: profiles/clevrer_vqa.md)."""
import json
import os

import numpy as np
import pytest
import torch

import clevrer_vqa_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clevrer_aloe.npz')


@pytest.fixture(autouse=True)
def split_bf16():
    """the reasoner exists in split-bf16 only (the process default) -- restored afterwards"""
    from slotformer_amd import _lib
    lib = _lib.lib()
    old = lib.sf_get_precision()
    lib.sf_set_precision(1)
    yield lib
    lib.sf_set_precision(old)


def rel_err(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(b).max())


def model_on(dev, cfg, sd):
    from slotformer_amd.clevrer_vqa.models import CLEVRERAloe, CLEVRERTransformerModel
    tm = CLEVRERTransformerModel(*cfg)
    tm.load_state_dict(sd)
    return CLEVRERAloe(tm).eval().to(dev)


def answers64(logits, mc):
    return (np.asarray(logits) > 0).astype(np.int32) if mc else np.argmax(logits, -1).astype(np.int32)


def run_case(dev, fc, m=None, slots=None, **over):
    m = model_on(dev, fc['cfg'], fc['sd']) if m is None else m
    s = torch.from_numpy(fc['slots']).to(dev) if slots is None else slots
    kw = dict(tokens=fc['tokens'], pad=fc['pad'], video_index=fc['video_index'], start=fc['start'])
    kw.update(over)
    t = lambda v, dt: None if v is None else torch.as_tensor(np.asarray(v)).to(dev, dt)  # noqa: E731
    logits, ans = m.transformer_model.answer(s, t(kw['tokens'], torch.int64), t(kw['pad'], torch.bool), fc['mc'], video_index=t(kw['video_index'], torch.int32),
                                             start=t(kw['start'], torch.int32), frame_offset=fc['frame_offset'], num_frames=fc['T'], want_answers=True)
    torch.cuda.synchronize()
    return m, (logits[:, 0] if fc['mc'] else logits), ans


@pytest.mark.parametrize('case', cases.FORWARD_CASES, ids=lambda c: c['name'])
@torch.no_grad()
def test_forward_vs_float64(dev, case):
    fc = cases.forward_case(case)
    ref = cases.reference64(fc)
    s = torch.from_numpy(fc['slots']).to(dev)
    if case.get('strided'):
        # every second video of a buffer that holds two slot sets per frame: video and frame strides larger than the extents, NaN in between
        V, T_all, N, C = s.shape
        big = torch.full((2 * V, T_all, 2, N, C), float('nan'), device=dev)
        big[::2, :, 0] = s
        s = big[::2, :, 0]
        assert not s.is_contiguous() and s.stride(1) == 2 * N * C
    m, logits, ans = run_case(dev, fc, slots=s)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == ref.shape
    e = rel_err(logits, ref)
    live = 1 + case['T'] * case['N'] + (~fc['pad']).sum(1)
    print(f"{case['name']}: B {case['B']} L {1 + case['T'] * case['N'] + case['text_len']} live {live.tolist()} d {cases.dims(fc['cfg'])['d']} "
          f"layers {case['nl']}: rel err vs float64 {e:.2e}")
    assert e < cases.DEVICE_BAR      # NaN (an unwritten row) fails it
    assert np.array_equal(ans.cpu().numpy(), answers64(ref, fc['mc']))   # exactly: every case clears the bar (tests/test_clevrer_vqa.py)
    # twice the same bits
    _, again, _ = run_case(dev, fc, m=m, slots=s)
    assert torch.equal(again, logits)
    # the padding is dead: other ids at the padded places -- one of them outside the vocabulary -- the same BITS
    if fc['pad'].any():
        tokens = fc['tokens'].copy()
        tokens[fc['pad']] = np.resize(np.array([3, 7, 99999, 1]), int(fc['pad'].sum()))
        _, other, _ = run_case(dev, fc, m=m, slots=s, tokens=tokens)
        assert torch.equal(other, logits)
    # a sequence does not depend on the others of the call
    if case['B'] >= 2:
        k = case['B'] // 2
        vi = [k if fc['video_index'] is None else fc['video_index'][k]]
        _, alone, _ = run_case(dev, fc, m=m, slots=s, tokens=fc['tokens'][k:k + 1], pad=fc['pad'][k:k + 1], video_index=vi,
                               start=None if fc['start'] is None else fc['start'][k:k + 1])
        assert rel_err(alone, ref[k:k + 1]) < cases.DEVICE_BAR


@torch.no_grad()
def test_reference_fixture_forward_losses_and_eval(dev):
    """The golden fixture (the reference shape, 12 layers) through forward / calc_train_loss / calc_eval_loss: the reference's keys and values."""
    g = np.load(GOLDEN)
    fc = cases.fixture_case()
    m = model_on(dev, fc['cfg'], fc['sd'])
    slots = torch.from_numpy(fc['slots']).to(dev)
    t = lambda k, dt=None: torch.from_numpy(fc[k]).to(dev) if dt is None else torch.from_numpy(fc[k]).to(dev, dt)  # noqa: E731
    data = {'cls_video_emb': slots, 'cls_q_tokens': t('cls_tokens'), 'cls_q_pad_mask': t('cls_pad'), 'cls_label': t('cls_label'),
            'mc_video_emb': slots[t('mc_video')], 'mc_q_tokens': t('mc_tokens'), 'mc_q_pad_mask': t('mc_pad'), 'mc_label': t('mc_label'),
            'mc_flag': t('mc_flag'), 'mc_subtype': t('mc_subtype')}
    out = m(data)
    assert list(out) == ['cls_answer_logits', 'mc_answer_logits', 'gt_v_emb', 'pred_v_emb'] and out['gt_v_emb'] is None and out['pred_v_emb'] is None
    for key, name in (('cls_answer_logits', 'cls_logits'), ('mc_answer_logits', 'mc_logits')):
        e = rel_err(out[key], g[name])
        print(f'{name} vs the reference fixture: {e:.2e}')
        assert tuple(out[key].shape) == g[name].shape and e < cases.DEVICE_BAR
    # in place: the same videos out of the slots tensor through an index, no mc_video_emb copy -- the same bits
    inplace = dict(data, slots=slots, cls_video_index=torch.arange(3, device=dev), mc_video_index=t('mc_video'))
    del inplace['cls_video_emb'], inplace['mc_video_emb']
    out2 = m(inplace)
    assert torch.equal(out2['cls_answer_logits'], out['cls_answer_logits']) and torch.equal(out2['mc_answer_logits'], out['mc_answer_logits'])
    train = m.calc_train_loss(data, out)
    assert list(train) == ['cls_answer_loss', 'mc_answer_loss', 'cls_bs', 'mc_bs'] and (train['cls_bs'], train['mc_bs']) == (3, 3)
    assert abs(train['cls_answer_loss'].item() - float(g['cls_answer_loss'])) < 1e-3 * float(g['cls_answer_loss'])
    assert abs(train['mc_answer_loss'].item() - float(g['mc_answer_loss'])) < 1e-3 * float(g['mc_answer_loss'])
    ev = m.calc_eval_loss(data, out)
    assert list(ev) == json.loads(str(g['eval_keys']))
    assert np.allclose([float(v) for v in ev.values()], g['eval_values'], rtol=0, atol=1e-6)
    assert all(isinstance(ev[k], int) for k in ev if k.endswith('_bs')) and all(torch.is_tensor(ev[k]) and ev[k].is_cuda for k in ev if k.endswith('_acc'))
    # an empty kind: None logits, zero loss, zero counts, the keys stay
    none = dict(data, mc_q_tokens=t('mc_tokens')[:0], mc_q_pad_mask=t('mc_pad')[:0], mc_flag=t('mc_flag')[:0], mc_label=t('mc_label')[:0],
                mc_subtype=t('mc_subtype')[:0])
    out3 = m(none)
    assert out3['mc_answer_logits'] is None and torch.equal(out3['cls_answer_logits'], out['cls_answer_logits'])
    tr3, ev3 = m.calc_train_loss(none, out3), m.calc_eval_loss(none, out3)
    assert tr3['mc_answer_loss'].item() == 0 and tr3['mc_bs'] == 0 and tr3['cls_answer_loss'].item() == train['cls_answer_loss'].item()
    assert list(ev3) == list(ev) and ev3['multiple-choice_bs'] == 0 and ev3['multiple-choice_acc'].item() == 0 and ev3['descriptive_bs'] == 3
    assert ev3['descriptive_acc'].item() == ev['descriptive_acc'].item()


@torch.no_grad()
def test_out_of_range_entries_give_nan_and_leave_neighbours(dev):
    """A video index, a frame or the token of a live position outside its table: NaN logits for that entry, answer -1, never an access; the
    other entries keep their bits."""
    case = next(c for c in cases.FORWARD_CASES if c['name'] == 'video-index-shuffled')
    fc = cases.forward_case(case)
    m, clean, ans = run_case(dev, fc)
    V = fc['slots'].shape[0]
    tok = fc['tokens'].copy()
    tok[3, 0] = 37                                    # (the vocabulary has 37 words; position 0 is live)
    for over, bad in ((dict(video_index=[3, V, 0, 2, -1]), [1, 4]), (dict(start=[0, 0, 1, 0, -1]), [2, 4]), (dict(tokens=tok), [3])):
        _, got, a = run_case(dev, fc, m=m, **over)
        good = [b for b in range(case['B']) if b not in bad]
        assert torch.isnan(got[bad]).all() and (a[bad] == -1).all(), over
        assert torch.equal(got[good], clean[good]) and torch.equal(a[good], ans[good]), over


@torch.no_grad()
def test_score_bookkeeping_and_accumulation(dev):
    """Runs of 4, 4, 3, 1 choices: per-question all-correct, the subtype counts and batch sizes equal the numpy restatement; the counts ADD over two
    calls; descriptive cross-entropy, argmax with a tie (the first index wins), more rows than one pass of the workgroup."""
    from slotformer_amd import ops
    rng = np.random.default_rng(11)
    flag = np.repeat(np.arange(4), [4, 4, 3, 1])
    labels = np.array([1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1], np.float32)
    mc = np.where(labels > 0, 2.0, -2.0) * rng.uniform(0.5, 1.5, 12)
    mc[5], mc[11] = 0.7, 0.0                           # question 1 gets a choice wrong; logit 0 is 'wrong': question 3 fails
    subtype = np.array([1, 2, 3, 3])
    cls = rng.standard_normal((300, 9))
    cls[7, 2] = cls[7, 5] = cls[7].max() + 1.0         # a tie: index 2 is the answer
    cls_labels = rng.integers(0, 9, 300)
    cls_labels[7] = 2
    want, corr = cases.eval_reference(cls, cls_labels, mc, labels, flag, subtype)
    d = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dev, dt)  # noqa: E731
    args = (d(cls, torch.float32), d(cls_labels, torch.int64), d(mc, torch.float32), d(labels, torch.float32), d(flag, torch.int64), d(subtype, torch.int64))
    losses, ques, counts = ops.aloe_score(*args)
    assert ques.cpu().tolist() == corr.astype(int).tolist() == [1, 0, 1, 0]
    c = counts.cpu().tolist()
    for i, key in enumerate(ops.ALOE_COUNT_KEYS):
        assert c[2 * i + 1] == want[f'{key}_bs'] and c[2 * i] == round(want[f'{key}_acc'] * want[f'{key}_bs']), key
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)  # noqa: E731
    assert abs(losses[0].item() - cases.ce64(f32(cls), cls_labels)) < 1e-6 * cases.ce64(f32(cls), cls_labels)
    assert abs(losses[1].item() - cases.bce64(f32(mc), labels)) < 1e-6 * cases.bce64(f32(mc), labels)
    # the counts add across calls, the losses and bits repeat
    losses2, _, counts2 = ops.aloe_score(*args, counts=counts)
    assert counts2 is counts and counts.cpu().tolist() == [2 * v for v in c] and torch.equal(losses2, losses)
    # multiple choice alone; descriptive alone
    _, q3, c3 = ops.aloe_score(None, None, *args[2:])
    assert c3.cpu().tolist() == [0, 0] + c[2:] and q3.cpu().tolist() == [1, 0, 1, 0]
    l4, q4, c4 = ops.aloe_score(args[0], args[1])
    assert c4.cpu().tolist() == c[:2] + [0] * 8 and q4.numel() == 0 and l4[1].item() == 0 and l4[0].item() == losses[0].item()


@torch.no_grad()
def test_harness_against_the_module(dev):
    """harness.clevrer_answers on 5 videos and 9 questions (5 descriptive, 4 multiple choice with 3, 1, 4, 2 choices) in batches of 4, the last
    one ragged, against the module called batch by batch; frames start + t * 2 of longer videos."""
    from slotformer_amd import harness
    hc = cases.harness_case()
    cfg, sd, slots, q, T = hc
    cls_tok, cls_pad, mc_tok, mc_pad, flag = q['cls_q_tokens'], q['cls_q_pad_mask'], q['mc_q_tokens'], q['mc_q_pad_mask'], q['mc_flag']
    m = model_on(dev, cfg, sd)
    s = torch.from_numpy(slots).to(dev)
    cls_ans, mc_ans = harness.clevrer_answers(m, s, q, batch_size=4)
    assert cls_ans.is_pinned() and mc_ans.is_pinned() and cls_ans.dtype == torch.int32 and mc_ans.dtype == torch.bool
    assert tuple(cls_ans.shape) == (5, ) and tuple(mc_ans.shape) == (10, )
    # against float64, exactly: the case clears the answer bar (tests/test_clevrer_vqa.py) ...
    ref_cls, ref_mc = cases.harness64(hc)
    assert np.array_equal(cls_ans.numpy(), answers64(ref_cls, False)) and np.array_equal(mc_ans.numpy(), answers64(ref_mc, True) > 0)
    # ... and against the module, batch by batch
    d = lambda a, dt=torch.int64: torch.from_numpy(np.asarray(a)).to(dev, dt)  # noqa: E731
    got_cls, got_mc = [], []
    for a, b in ((0, 4), (4, 5)):
        out = m({'slots': s, 'frame_offset': 2, 'num_frames': T, 'cls_q_tokens': d(cls_tok[a:b]), 'cls_q_pad_mask': d(cls_pad[a:b], torch.bool),
                 'cls_video_index': d(q['cls_video_index'][a:b]), 'cls_start': d(q['cls_start'][a:b]), 'mc_q_tokens': d(mc_tok[:0])})
        assert out['mc_answer_logits'] is None
        got_cls.append(out['cls_answer_logits'].argmax(-1))
    for qa, qb in ((0, 2), (2, 4)):   # questions 0-1 (choices 0..3), 2-3 (choices 4..9): mc_flag restarts at 0 in every batch, as the dataset collates
        rows = (flag >= qa) & (flag < qb)
        out = m({'slots': s, 'frame_offset': 2, 'num_frames': T, 'cls_q_tokens': d(cls_tok[:0]), 'mc_q_tokens': d(mc_tok[rows]),
                 'mc_q_pad_mask': d(mc_pad[rows], torch.bool), 'mc_flag': d(flag[rows] - qa), 'mc_video_index': d(q['mc_video_index'][qa:qb]),
                 'mc_start': d(q['mc_start'][qa:qb])})
        assert out['cls_answer_logits'] is None
        got_mc.append(out['mc_answer_logits'] > 0)
    assert torch.equal(torch.cat(got_cls).cpu().int(), cls_ans) and torch.equal(torch.cat(got_mc).cpu(), mc_ans)
    on_dev = harness.clevrer_answers(m, s, q, batch_size=256, to_host=False)
    assert on_dev[0].is_cuda and torch.equal(on_dev[0].cpu(), cls_ans) and torch.equal(on_dev[1].cpu(), mc_ans)


@torch.no_grad()
def test_weight_changes_rebuild_the_plan(dev):
    """After an in-place weight change the plan is rebuilt: the text table is recomputed and the logits follow the new weights."""
    from slotformer_amd import engine
    case = next(c for c in cases.FORWARD_CASES if c['name'] == 'b4-one-row-tile')
    fc = cases.forward_case(case)
    m, before, _ = run_case(dev, fc)
    tm = m.transformer_model
    plan = engine.aloe_plan(tm)
    assert engine.aloe_plan(tm) is plan                      # cached while nothing changes
    table = plan.text_table.clone()
    tm.q_embedding.weight.mul_(1.5)
    tm.q_in_proj.bias.add_(0.25)
    _, after, _ = run_case(dev, fc, m=m)
    plan2 = engine.aloe_plan(tm)
    assert plan2 is not plan and not torch.equal(plan2.text_table, table)
    sd = dict(fc['sd'])
    sd['q_embedding.weight'] = fc['sd']['q_embedding.weight'] * 1.5
    sd['q_in_proj.bias'] = fc['sd']['q_in_proj.bias'] + 0.25
    ref = cases.forward64(sd, fc['cfg'], fc['slots'], fc['tokens'], fc['pad'], fc['mc'], fc['video_index'], fc['start'], fc['frame_offset'], fc['T'])
    assert rel_err(after, ref) < cases.DEVICE_BAR and rel_err(before, ref) > 10 * cases.DEVICE_BAR
    # the table itself: P[w] = Wq[:, :E] emb[w] + Wq[:, E + 2] + bq
    E = cases.dims(fc['cfg'])['E']
    W = sd['q_in_proj.weight'].double()
    want = sd['q_embedding.weight'].double() @ W[:, :E].T + W[:, E + 2] + sd['q_in_proj.bias'].double()
    assert rel_err(plan2.text_table, want.numpy()) < 1e-6
