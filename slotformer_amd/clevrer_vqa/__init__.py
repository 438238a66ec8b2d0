"""slotformer.clevrer_vqa counterpart: build_model, the two drivers around the reasoner -- `fit` (the reference's nerv training run of
aloe_clevrer_params.py through clevrer_vqa/method.py) and `evaluate` -- on a device-resident slots tensor, and the host assembly of the result
records test_clevrer_vqa.py writes.  The inference loop itself is `harness.clevrer_answers`."""
import numpy as np
import torch

from ..physion_vqa import batch_schedule, step_seed   # (one rule for the batches and the dropout seeds of every fit)

from .models import build_model, CLEVRERAloe, CLEVRERTransformerModel

FIRST_TEST_SCENE = 15000   # test_clevrer_vqa.py: results[scene_index - 15000]
NUM_TEST_SCENES = 5000


def build_dataset(params, *a, **k):
    raise NotImplementedError('datasets are host-side I/O outside the hot path (SURVEY.md 2.1 row 13)')


def build_method(*a, **k):
    raise NotImplementedError('the nerv trainer is outside the hot path (SURVEY.md 2.1 row 12); the training kernels of CLEVRERAloe are '
                              'reached through clevrer_vqa.fit / train.aloe_with_grad; a trainer object is not built')


def result_records(cls_answers, mc_answers, questions, label2answer, first_scene=FIRST_TEST_SCENE, num_scenes=NUM_TEST_SCENES):
    """The list test_clevrer_vqa.py dumps as CLEVRER.json, from the answers of `harness.clevrer_answers`.

    cls_answers [B1] answer ids and mc_answers [Bn] booleans; questions: the collated arrays `cls_scene_index`, `cls_question_id` [B1],
    `mc_scene_index`, `mc_question_id` [B2], `mc_flag`, `mc_choice_id` [Bn]; label2answer: id -> answer word.  Descriptive questions get
    {'question_id', 'answer'}; the choices of a multiple-choice question get {'choice_id', 'answer': 'correct' | 'wrong'} under one
    {'question_id', 'choices'} entry per question -- a question id already present in its scene is extended, as there."""
    results = [{'scene_index': i + first_scene, 'questions': []} for i in range(num_scenes)]
    cls_answers, mc_answers = np.asarray(cls_answers).reshape(-1), np.asarray(mc_answers).reshape(-1).astype(bool)
    for i in range(cls_answers.size):
        results[int(questions['cls_scene_index'][i]) - first_scene]['questions'].append(
            {'question_id': int(questions['cls_question_id'][i]), 'answer': str(label2answer[int(cls_answers[i])])})
    flag, choice_id = np.asarray(questions['mc_flag']).reshape(-1), np.asarray(questions['mc_choice_id']).reshape(-1)
    for i in range(len(questions['mc_question_id'])):
        q_id = int(questions['mc_question_id'][i])
        sel = flag == i
        choices = [{'choice_id': int(c), 'answer': 'correct' if a else 'wrong'} for c, a in zip(choice_id[sel], mc_answers[sel])]
        q_list = results[int(questions['mc_scene_index'][i]) - first_scene]['questions']
        for entry in q_list:
            if entry['question_id'] == q_id:
                entry['choices'] += choices
                break
        else:
            q_list.append({'question_id': q_id, 'choices': choices})
    return results


def question_schedule(questions, epochs, batch_size, seed):
    """The batches `fit` trains on, a function of its arguments alone: the Q1 descriptive and Q2 multiple-choice questions are numbered
    0 .. Q1 + Q2 - 1 and drawn by `physion_vqa.batch_schedule` (one permutation per epoch, `batch_size` QUESTIONS per batch, the last batch of an
    epoch ragged).  -> [epoch][batch] dicts of host int64 arrays: `cls` the descriptive questions of the batch in the order drawn; `mc` its
    multiple-choice questions in the order drawn; `mc_rows` the rows of the collated choice arrays those questions expand to -- every choice of
    a question, together and in order.  The sequences of a batch are the `cls` questions first, then `mc_rows`."""
    q1 = 0 if questions.get('cls_q_tokens') is None else len(questions['cls_q_tokens'])
    flag = np.zeros(0, np.int64) if questions.get('mc_flag') is None else np.asarray(questions['mc_flag']).reshape(-1).astype(np.int64)
    q2 = 0 if questions.get('mc_video_index') is None else len(questions['mc_video_index'])
    if flag.size and (np.any(np.diff(flag) < 0) or flag.min() < 0 or flag.max() >= q2):
        raise ValueError(f'slotformer_amd.clevrer_vqa: mc_flag holds non-decreasing question numbers in [0, {q2})')
    if q1 + q2 < 1:
        raise ValueError('slotformer_amd.clevrer_vqa: no question to train on')
    first, last = np.searchsorted(flag, np.arange(q2), 'left'), np.searchsorted(flag, np.arange(q2), 'right')
    out = []
    for epoch in batch_schedule(q1 + q2, epochs, batch_size, seed):
        batches = []
        for idx in epoch:
            idx = idx.numpy().astype(np.int64)
            mc = idx[idx >= q1] - q1
            rows = np.concatenate([np.arange(first[q], last[q]) for q in mc]) if mc.size else np.zeros(0, np.int64)
            batches.append(dict(cls=idx[idx < q1], mc=mc, mc_rows=rows.astype(np.int64)))
        out.append(batches)
    return out


def _collated(questions, dev):
    """The collated arrays of `harness.clevrer_answers` plus the labels, on the device: one sequence table over the descriptive questions and,
    behind them, the choices (video and start frame of a choice composed through mc_flag)."""
    def get(key, dtype, width=None):
        v = questions.get(key)
        if v is None:
            return torch.zeros((0, width) if width else (0, ), dtype=dtype, device=dev)
        return torch.as_tensor(v).to(dev, dtype)

    cls_tok, mc_tok = questions.get('cls_q_tokens'), questions.get('mc_q_tokens')
    width = (cls_tok if cls_tok is not None else mc_tok).shape[-1]
    flag = get('mc_flag', torch.int64)
    q1, qn = get('cls_q_tokens', torch.int32, width).shape[0], flag.numel()

    def rows(key, dtype, required):
        """one entry per sequence: the descriptive questions' own, the choices' through mc_flag; each kind on its own -- a kind with questions and
        no `video_index` is refused, one without `start` reads from frame 0"""
        out = []
        for kind, n, pick in (('cls', q1, None), ('mc', qn, flag)):
            v = questions.get(f'{kind}_{key}')
            if n and v is None:
                if required:
                    raise ValueError(f'slotformer_amd.clevrer_vqa: {kind}_{key} is missing: every question names its video')
                out.append(torch.zeros(n, dtype=dtype, device=dev))
            else:
                t = get(f'{kind}_{key}', dtype)
                out.append(t if pick is None else t[pick])
        return torch.cat(out)

    return dict(tokens=torch.cat([get('cls_q_tokens', torch.int32, width), get('mc_q_tokens', torch.int32, width)]),
                pad=torch.cat([get('cls_q_pad_mask', torch.uint8, width), get('mc_q_pad_mask', torch.uint8, width)]),
                video=rows('video_index', torch.int32, True), start=rows('start', torch.int32, False), cls_label=get('cls_label', torch.int32),
                mc_label=get('mc_label', torch.float32), q1=q1, qn=qn)


def _transformer(model):
    return getattr(model, 'transformer_model', model)


def fit(model, slots, questions, epochs, batch_size=128, lr=1e-3, seed=0, warmup_steps_pct=0.1, min_lr_ratio=0.01, cls_answer_loss_w=1.,
        mc_answer_loss_w=1.):
    """Train a CLEVRERAloe (or its CLEVRERTransformerModel) in place on slots [V, T_all, N, C] that live on the device and are read in place
    (aloe_clevrer_params.py through clevrer_vqa/method.py: Adam at 1e-3, 10 % linear warm-up then cosine decay to lr / 100, loss = cross-entropy on
    the descriptive questions + BCE-with-logits on the choices, no weight decay, no clipping; dropout 0.1 from nn.TransformerEncoderLayer).
    questions: the collated arrays `harness.clevrer_answers` takes plus `cls_label` [B1], `mc_label` [Bn] and `mc_subtype` [B2].  A batch is
    `batch_size` QUESTIONS of both kinds (`question_schedule` on `seed`), each multiple-choice question expanded to its choices; (B1, Bn) of every
    batch is known on the host, every index tensor goes up before the first step and the workspace is sized for the largest batch.  A step is
    the training forward, the score-gradient launch, the backward -- which writes every gradient straight into the optimiser's flat bucket -- and
    one `FlatAdam` launch; the dropout masks of step k come from `step_seed(seed, k)`.  Nothing is uploaded, downloaded or waited for inside an
    epoch, and everything is deterministic: one seed, one result, bit for bit.  Leaves the module in eval() with its cached plans dropped, so
    that `answer` sees the trained weights and a fresh text table.  Returns the mean (cross-entropy, BCE) of every epoch, [epochs, 2] on the
    device."""
    from .. import ops, plans
    from .._call import scratch
    from .._lib import lib
    from ..train import FlatAdam, warmup_cosine_lr, aloe_parameters, aloe_model
    import ctypes as C
    tm = _transformer(model)
    if not torch.is_tensor(slots) or slots.dim() != 4 or slots.shape[3] != tm.vision_in_proj.in_features - 2:
        raise ValueError(f'slotformer_amd.clevrer_vqa: slots are a [V, T, N, {tm.vision_in_proj.in_features - 2}] tensor, got '
                         f'{tuple(getattr(slots, "shape", ()))}')
    V, T_all, N = slots.shape[:3]
    T = int(questions.get('num_frames') or T_all)
    offset = int(questions.get('frame_offset', 1))
    sched = question_schedule(questions, epochs, batch_size, seed)
    for key in ('cls', 'mc'):
        vi = questions.get(f'{key}_video_index')
        if vi is None and questions.get(f'{key}_q_tokens') is not None and len(questions[f'{key}_q_tokens']):
            raise ValueError(f'slotformer_amd.clevrer_vqa: {key}_video_index is missing: every question names its video')
        if vi is not None and len(vi) and (np.asarray(vi).min() < 0 or np.asarray(vi).max() >= V):
            raise IndexError(f'slotformer_amd.clevrer_vqa: {key}_video_index outside the {V} videos')
        st = questions.get(f'{key}_start')
        if st is not None and len(st) and (np.asarray(st).min() < 0 or np.asarray(st).max() + (T - 1) * offset >= T_all):
            raise IndexError(f'slotformer_amd.clevrer_vqa: {key}_start + {T - 1} * {offset} outside the {T_all} frames')
    if not (slots.is_cuda and tm.CLS.is_cuda):   # (what the host can check comes first, so that it is checked without a device too)
        raise RuntimeError('slotformer_amd: CLEVRERAloe trains on a HIP device only; there is no CPU fallback')
    dev = slots.device
    col = _collated(questions, dev)
    q1 = col['q1']
    params = aloe_parameters(tm)
    for p in params:
        p.requires_grad_(True)
    opt = FlatAdam(params, lr=lr)
    desc, keep = aloe_model(tm, N, T, col['tokens'].shape[1])   # (after FlatAdam: the parameters now live in its bucket)
    p_drop = float(tm.transformer_encoder.layers[0].dropout.p)
    batches, biggest = [], 1
    for epoch in sched:   # every index tensor goes up, and every batch is picked, before the first step
        eb = []
        for b in epoch:
            seq = torch.as_tensor(np.concatenate([b['cls'], q1 + b['mc_rows']]), device=dev)
            eb.append(dict(tokens=col['tokens'][seq], pad_mask=col['pad'][seq], B1=len(b['cls']), video_index=col['video'][seq], start=col['start'][seq],
                           frame_offset=offset, cls_label=col['cls_label'][torch.as_tensor(b['cls'], device=dev)],
                           mc_label=col['mc_label'][torch.as_tensor(b['mc_rows'], device=dev)]))
            biggest = max(biggest, seq.numel())
        batches.append(eb)
    n_cls, n_mc = max(q1, 1), max(col['qn'], 1)
    for eb in batches:   # the share of each batch in its epoch's two means, uploaded with the index tensors
        for b in eb:
            b['loss_share'] = torch.tensor([b['B1'] / n_cls, (b['tokens'].shape[0] - b['B1']) / n_mc], dtype=torch.float32).to(dev)
    total = sum(len(e) for e in batches)
    warm = int(round(float(warmup_steps_pct) * total))
    ws = scratch(lib().sf_aloe_train_workspace_bytes, C.byref(desc), biggest, device=dev)
    step, losses = 0, []
    tm.train()
    with torch.no_grad():
        for eb in batches:
            epoch_loss = torch.zeros(2, dtype=torch.float32, device=dev)
            for b in eb:
                s = step_seed(seed, step)
                cls_logits, mc_logits, ws, _, _ = ops.aloe_train_fwd(desc, slots, b, p=p_drop, seed=s, ws=ws)
                loss, g_cls, g_mc = ops.aloe_score_grad(cls_logits, b['cls_label'], mc_logits, b['mc_label'], cls_answer_loss_w, mc_answer_loss_w)
                ops.aloe_train_bwd(desc, slots, b, g_cls, g_mc, ws, p=p_drop, seed=s, out=opt.grad)
                opt.lr = warmup_cosine_lr(step, total, warm, lr, lr * float(min_lr_ratio))
                opt.step(gathered=True)
                step += 1
                epoch_loss += loss * b['loss_share']
            losses.append(epoch_loss)
    del keep
    model.eval()
    plans.invalidate(tm)
    return torch.stack(losses) if losses else torch.zeros(0, 2, device=dev)


@torch.no_grad()
def evaluate(model, slots, questions, batch_size=256):
    """calc_eval_loss over a whole set -> its ten keys (`<kind>_acc` floats, `<kind>_bs` ints for descriptive, multiple-choice, explanatory,
    predictive, counterfactual).  The logits of every batch stay on the device; one score launch counts them (`CLEVRERAloe.eval_counts`) and the
    ten counts come back in ONE download."""
    from .. import harness, ops
    if int(batch_size) < 1:
        raise ValueError(f'slotformer_amd.clevrer_vqa: batch_size >= 1, got {batch_size!r}')
    tm = _transformer(model)
    if not (torch.is_tensor(slots) and slots.is_cuda and tm.CLS.is_cuda):
        raise RuntimeError('slotformer_amd: CLEVRERAloe runs on a HIP device only; there is no CPU fallback')
    dev = slots.device
    was_training = tm.training
    tm.eval()
    try:
        col = _collated(questions, dev)
        q1, n = col['q1'], col['tokens'].shape[0]
        T, offset = questions.get('num_frames'), int(questions.get('frame_offset', 1))
        cls_logits = torch.empty(q1, tm.num_answer_classes, dtype=torch.float32, device=dev)
        mc_logits = torch.empty(n - q1, dtype=torch.float32, device=dev)
        for lo, hi, mc, dst in ((0, q1, False, cls_logits), (q1, n, True, mc_logits)):
            for a, b in harness.render_chunks(hi - lo, int(batch_size)):
                a, b = lo + a, lo + b
                got, _ = tm.answer(slots, col['tokens'][a:b], col['pad'][a:b], mc, video_index=col['video'][a:b], start=col['start'][a:b],
                                   frame_offset=offset, num_frames=T)
                dst[a - lo:b - lo] = got.view(-1) if mc else got
    finally:
        tm.train(was_training)
    _, _, counts = ops.aloe_score(cls_logits if q1 else None, col['cls_label'], mc_logits if n > q1 else None, col['mc_label'], questions.get('mc_flag'),
                                  questions.get('mc_subtype'), device=dev)
    host = counts.cpu().tolist()
    out = {}
    for i, key in enumerate(ops.ALOE_COUNT_KEYS):
        right, bs = host[2 * i], host[2 * i + 1]
        out[f'{key}_acc'], out[f'{key}_bs'] = (right / bs if bs else 0.), bs
    return out
