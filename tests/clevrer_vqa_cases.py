"""What the tests of the CLEVRER VQA path share (no test in here): seeded weights and inputs, a float64 restatement of the Aloe reasoner written
from the model's definition (slotformer/clevrer_vqa/models/transformer.py: CLS, vision_in_proj([slot | 0 1]), q_in_proj([q_embedding | type
pair | 1 0]), a learnable position row on every row, a pre-LN nn.TransformerEncoder under a key-padding mask, an MLP on the CLS row) that DROPS
the padded rows outright instead of masking them, and numpy restatements of CLEVRERAloe.calc_eval_loss and of the record loop of
test_clevrer_vqa.py.

Assumed about the third-party encoder the reference builds (nerv, not in the reference tree): the id pair is appended AFTER the features, the
position table is added to every row (CLS included), the layers are torch's nn.TransformerEncoderLayer (relu, eps 1e-5)."""
import numpy as np
import torch
import torch.nn.functional as F

from phyre_readout_cases import DEVICE_BAR, layer64, seeded_slots  # noqa: F401  (the project's 1e-3 bar; one pre-LN layer in float64)

# aloe_clevrer_params-rollout.py
TRANSFORMER_DICT = dict(input_len=(6 + 1) * 25 + 20 + 12, input_dim=16, pos_enc='learnable', num_layers=12, num_heads=8, ffn_dim=512,
                        norm_first=True, cls_mlp_size=128)
LANG_DICT = dict(question_vocab_size=82, answer_vocab_size=22, question_len=20)
FIXTURE = dict(B=3, T=25, N=7, C=128, text_len=32, seed=20241019)
LAYER_LEAVES = ('self_attn.in_proj_weight', 'self_attn.in_proj_bias', 'self_attn.out_proj.weight', 'self_attn.out_proj.bias', 'linear1.weight',
                'linear1.bias', 'linear2.weight', 'linear2.bias', 'norm1.weight', 'norm1.bias', 'norm2.weight', 'norm2.bias')


def config(T=25, N=7, C=128, text_len=32, heads=8, input_dim=16, nl=12, ffn=512, question_len=20, q_vocab=82, a_vocab=22, mlp=128):
    """-> (transformer_dict, lang_dict, vision_dict, loss_dict) of a CLEVRERTransformerModel over 1 + T N + text_len tokens"""
    return (dict(TRANSFORMER_DICT, input_len=T * N + text_len, input_dim=input_dim, num_layers=nl, num_heads=heads, ffn_dim=ffn, cls_mlp_size=mlp),
            dict(question_vocab_size=q_vocab, answer_vocab_size=a_vocab, question_len=question_len), dict(vision_dim=C),
            dict(use_mask_obj_loss=False))


def dims(cfg):
    td, ld, vd, _ = cfg
    d = (td['input_dim'] + 2) * td['num_heads']
    return dict(d=d, E=td['input_dim'] - 2, L=td['input_len'] + 1, C=vd['vision_dim'], heads=td['num_heads'], ffn=td['ffn_dim'], nl=td['num_layers'],
                mlp=td['cls_mlp_size'], q_vocab=ld['question_vocab_size'], a_vocab=ld['answer_vocab_size'], question_len=ld['question_len'])


def owned_shapes(cfg):
    """[(key, shape)] of the parameters the REFERENCE's CLEVRERTransformerModel owns itself, in its state-dict order without the encoder's:
    the module's own parameters first, then the submodules in construction order."""
    m = dims(cfg)
    d, E, C, H, A = m['d'], m['E'], m['C'], m['mlp'], m['a_vocab']
    return [('text_token', (2, )), ('vision_token', (2, )), ('cls_token', (2, )), ('mc_question_token', (2, )), ('mc_choice_token', (2, )),
            ('CLS', (1, 1, d)), ('q_embedding.weight', (m['q_vocab'], E)), ('q_in_proj.weight', (d, E + 4)), ('q_in_proj.bias', (d, )),
            ('cls_answer_mlp.0.weight', (H, d)), ('cls_answer_mlp.0.bias', (H, )), ('cls_answer_mlp.2.weight', (A, H)), ('cls_answer_mlp.2.bias', (A, )),
            ('mc_answer_mlp.0.weight', (H, d)), ('mc_answer_mlp.0.bias', (H, )), ('mc_answer_mlp.2.weight', (1, H)), ('mc_answer_mlp.2.bias', (1, )),
            ('vision_in_proj.weight', (d, C + 2)), ('vision_in_proj.bias', (d, ))]


def encoder_shapes(cfg):
    """[(key, shape)] of this repository's AloeEncoder under `transformer_encoder.`"""
    m = dims(cfg)
    d, ffn = m['d'], m['ffn']
    shape = {'self_attn.in_proj_weight': (3 * d, d), 'self_attn.in_proj_bias': (3 * d, ), 'self_attn.out_proj.weight': (d, d),
             'self_attn.out_proj.bias': (d, ), 'linear1.weight': (ffn, d), 'linear1.bias': (ffn, ), 'linear2.weight': (d, ffn), 'linear2.bias': (d, ),
             'norm1.weight': (d, ), 'norm1.bias': (d, ), 'norm2.weight': (d, ), 'norm2.bias': (d, )}
    return [('transformer_encoder.pos_enc', (1, m['L'], d))] + [(f'transformer_encoder.layers.{i}.{leaf}', shape[leaf]) for i in range(m['nl'])
                                                                for leaf in LAYER_LEAVES]


def state_shapes(cfg):
    own = owned_shapes(cfg)
    return own[:6] + encoder_shapes(cfg) + own[6:]


_TOKENS = {'text_token': (1, 0), 'vision_token': (0, 1), 'cls_token': (0, 1), 'mc_question_token': (1, 0), 'mc_choice_token': (0, 1)}


def seeded_weights(cfg, seed):
    """{key: float32 tensor} for every entry of state_shapes(cfg) from one numpy generator: nn.Linear-sized matrices, biases and LayerNorm
    parameters away from 0 / 1 (a wrong index must show), O(1) CLS and position rows, unit-scale embeddings; the id pairs are the fixed ones."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in state_shapes(cfg):
        leaf = key.rsplit('.', 1)[-1]
        if key in _TOKENS:
            a = np.array(_TOKENS[key], np.float64)
        elif key == 'CLS' or key.endswith('pos_enc'):
            a = 0.5 * rng.standard_normal(shape)
        elif key == 'q_embedding.weight':
            a = rng.standard_normal(shape)
        elif len(shape) == 2:
            a = rng.uniform(-1, 1, shape) * (1.5 / np.sqrt(shape[1]))
        elif 'norm' in key and leaf == 'weight':
            a = 1.0 + 0.1 * rng.standard_normal(shape)
        else:
            a = 0.1 * rng.uniform(-1, 1, shape)
        sd[key] = torch.from_numpy(np.asarray(a, np.float32))
    return sd


def seeded_text(seed, B, text_len, vocab, lengths=None, question_len=None, choice_lengths=None):
    """-> (tokens [B, text_len] int64, pad_mask [B, text_len] bool).  lengths[b] live positions from 0 (default: random in [1, text_len]);
    with question_len / choice_lengths (multiple choice) the choice occupies [question_len, question_len + choice_lengths[b]) and the question
    [0, min(lengths[b], question_len)): padding stands in the middle AND at the end.  Padded positions hold token 0, as the dataset pads."""
    rng = np.random.default_rng(seed)
    tokens = rng.integers(1, vocab, size=(B, text_len))
    pad = np.ones((B, text_len), bool)
    lengths = rng.integers(1, (question_len or text_len) + 1, size=B) if lengths is None else np.asarray(lengths)
    for b in range(B):
        pad[b, :min(int(lengths[b]), question_len or text_len)] = False
        if question_len is not None:
            n = int(choice_lengths[b]) if choice_lengths is not None else int(rng.integers(1, text_len - question_len + 1))
            pad[b, question_len:question_len + n] = False
    tokens[pad] = 0
    return tokens.astype(np.int64), pad


def forward64(sd, cfg, slots, tokens, pad, mc, video_index=None, start=None, frame_offset=1, T=None):
    """logits in float64 (numpy): [B, answer_vocab] for descriptive questions, [B] for multiple choice.  slots [V, T_all, N, C]; batch entry b
    reads video video_index[b] (default b) at frames start[b] + t * frame_offset, t < T (default all frames from 0).  Every sequence is built
    WITHOUT its padded text rows -- position rows chosen by the original place -- and runs alone: nothing is masked."""
    m = dims(cfg)
    heads = m['heads']
    g = lambda k: sd[k].double()  # noqa: E731
    s = torch.as_tensor(np.asarray(slots)).double()
    tokens, pad = np.asarray(tokens), np.asarray(pad).astype(bool)
    B, text_len = tokens.shape
    T = s.shape[1] if T is None else T
    N = s.shape[2]
    pos = g('transformer_encoder.pos_enc')[0]
    mlp = 'mc_answer_mlp' if mc else 'cls_answer_mlp'
    out = []
    for b in range(B):
        vid = b if video_index is None else int(video_index[b])
        f0 = 0 if start is None else int(start[b])
        frames = s[vid, [f0 + t * frame_offset for t in range(T)]]                      # [T, N, C]
        v_in = torch.cat([frames.flatten(0, 1), g('vision_token').expand(T * N, 2)], -1)   # the id pair AFTER the features
        v_rows = F.linear(v_in, g('vision_in_proj.weight'), g('vision_in_proj.bias'))
        emb = g('q_embedding.weight')[torch.as_tensor(tokens[b])]
        if mc:
            ql = m['question_len']
            typ = torch.cat([g('mc_question_token').expand(ql, 2), g('mc_choice_token').expand(text_len - ql, 2)], 0)
        else:
            typ = g('cls_token').expand(text_len, 2)
        q_in = torch.cat([emb, typ, g('text_token').expand(text_len, 2)], -1)
        q_rows = F.linear(q_in, g('q_in_proj.weight'), g('q_in_proj.bias'))
        x = torch.cat([g('CLS')[0], v_rows, q_rows], 0) + pos
        keep = np.concatenate([np.ones(1 + T * N, bool), ~pad[b]])
        x = x[torch.as_tensor(keep)][None]                                              # the padded rows are gone
        for i in range(m['nl']):
            x = layer64(sd, f'transformer_encoder.layers.{i}.', x, heads)
        h = F.relu(F.linear(x[0, 0], g(mlp + '.0.weight'), g(mlp + '.0.bias')))
        out.append(F.linear(h, g(mlp + '.2.weight'), g(mlp + '.2.bias')).numpy())
    out = np.stack(out)
    return out[:, 0] if mc else out


def clearance(logits, mc):
    """(margin, bar): descriptive -- the smallest top-2 gap of a row against 2 DEVICE_BAR max|logit|; multiple choice -- the smallest |logit|
    against DEVICE_BAR max|logit|.  margin > bar makes the device's answers comparable exactly."""
    x = np.asarray(logits, np.float64)
    big = np.abs(x).max()
    if mc:
        return float(np.abs(x).min()), DEVICE_BAR * big
    top = np.sort(x, -1)
    return float((top[:, -1] - top[:, -2]).min()), 2 * DEVICE_BAR * big


def ce64(logits, labels):
    x = np.asarray(logits, np.float64)
    mx = x.max(-1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x - mx).sum(-1))
    return float(np.mean(lse - x[np.arange(len(x)), np.asarray(labels)]))


def bce64(logits, labels):
    x, y = np.asarray(logits, np.float64), np.asarray(labels, np.float64)
    return float(np.mean(np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))))


def eval_reference(cls_logits, cls_labels, mc_logits, mc_labels, mc_flag, mc_subtype):
    """CLEVRERAloe.calc_eval_loss restated in numpy: {key: value} with the reference's ten keys; a kind is absent when its logits are None."""
    ret = {}
    if cls_logits is None:
        ret['descriptive_acc'], ret['descriptive_bs'] = 0., 0
    else:
        ret['descriptive_acc'] = float((np.argmax(cls_logits, -1) == np.asarray(cls_labels)).mean())
        ret['descriptive_bs'] = len(cls_labels)
    if mc_logits is None:
        corr = None
        ret['multiple-choice_acc'], ret['multiple-choice_bs'] = 0., 0
    else:
        right = (np.asarray(mc_logits) > 0).astype(np.float64) == np.asarray(mc_labels, np.float64)
        flag = np.asarray(mc_flag)
        bs = int(flag.max()) + 1
        corr = np.array([right[flag == i].all() for i in range(bs)])
        ret['multiple-choice_acc'], ret['multiple-choice_bs'] = float(corr.sum() / bs), bs
    for name, sid in (('explanatory', 1), ('predictive', 2), ('counterfactual', 3)):
        sel = None if corr is None else np.asarray(mc_subtype) == sid
        if sel is None or not sel.any():
            ret[f'{name}_acc'], ret[f'{name}_bs'] = 0., 0
        else:
            ret[f'{name}_acc'], ret[f'{name}_bs'] = float(corr[sel].sum() / sel.sum()), int(sel.sum())
    return ret, corr


def records_reference(batches, label2answer):
    """The loop of test_clevrer_vqa.py (test) restated on numpy batches: each batch holds `scene_index`, `question_id` [B] (descriptive questions
    first, as the dataset collates them), `mc_choice_id`, `mc_flag` [Bn], `cls_answer` [B1] (argmax) or None, `mc_answer` [Bn] (logit > 0) or None."""
    results = [{'scene_index': i + 15000, 'questions': []} for i in range(5000)]
    for bt in batches:
        num_cls = 0 if bt['cls_answer'] is None else len(bt['cls_answer'])
        num_mc = 0 if bt['mc_answer'] is None else int(bt['mc_flag'].max()) + 1
        for i in range(num_cls):
            results[bt['scene_index'][i] - 15000]['questions'].append(
                {'question_id': int(bt['question_id'][i]), 'answer': str(label2answer[int(bt['cls_answer'][i])])})
        for i in range(num_mc):
            idx = i + num_cls
            q_id = bt['question_id'][idx]
            ans, cid = bt['mc_answer'][bt['mc_flag'] == i], bt['mc_choice_id'][bt['mc_flag'] == i]
            lst = [{'choice_id': int(cid[j]), 'answer': 'correct' if ans[j] else 'wrong'} for j in range(len(cid))]
            q_list = results[bt['scene_index'][idx] - 15000]['questions']
            hit = [j for j, e in enumerate(q_list) if e['question_id'] == q_id]
            if hit:
                q_list[hit[0]]['choices'] += lst
            else:
                q_list.append({'question_id': int(q_id), 'choices': lst})
    return results


def fixture_case():
    """The inputs of tests/golden/clevrer_aloe.npz (the reference shape: 3 videos of 25 frames, 7 slots of 128, 32 text positions, 12 layers):
    the tool that wrote the file and the tests build them alike."""
    cfg = config()
    f = FIXTURE
    sd = seeded_weights(cfg, f['seed'])
    slots = seeded_slots(f['seed'] + 1, f['B'], f['T'], f['N'], f['C'])
    cls_tokens, cls_pad = seeded_text(f['seed'] + 2, f['B'], f['text_len'], 82, lengths=[9, 20, 14])
    cls_label = np.array([6, 3, 6])            # (the reference answers 6, 14, 6: two of three right)
    # two multiple-choice questions on videos 0 and 2 with 2 + 1 choices
    mc_flag = np.array([0, 0, 1])
    mc_tokens, mc_pad = seeded_text(f['seed'] + 4, 3, f['text_len'], 82, lengths=[12, 12, 20], question_len=20, choice_lengths=[5, 12, 3])
    mc_label = np.array([0., 0., 1.], np.float32)   # (it says 'wrong' to every choice: question 0 all right, question 1 not)
    mc_subtype = np.array([1, 3])
    return dict(cfg=cfg, sd=sd, slots=slots, cls_tokens=cls_tokens, cls_pad=cls_pad, cls_label=cls_label, mc_video=np.array([0, 2]),
                mc_flag=mc_flag, mc_tokens=mc_tokens, mc_pad=mc_pad, mc_label=mc_label, mc_subtype=mc_subtype)


# ---- the seeded cases of the GPU forward test -----------------------------------------------------------------------------------------------------
# A sequence is one workgroup per head in the attention launch and one in the head launch; the embedding launch packs 48 vision rows of the
# flattened (b, t, n) space into a workgroup, so batches on both sides of a 48-row tile are: T N = 175 -> B 1 (4 tiles, the last partial),
# T N = 12 -> B 4 (one tile exactly) and B 5 (one row tile over); T N = 1 -> B 5 (a tile of 5 rows).  The GEMMs tile B L rows by 32 .. 128.
# lengths: live question positions (descriptive) -- L_live = 1 + T N + length.
def _case(name, B, T, N, C, text_len, heads=8, input_dim=16, nl=2, ffn=512, seed=0, **kw):
    return dict(name=name, B=B, T=T, N=N, C=C, text_len=text_len, heads=heads, input_dim=input_dim, nl=nl, ffn=ffn, seed=seed, **kw)


FORWARD_CASES = [
    _case('tiny-L6', 5, 1, 1, 32, 4, nl=1, seed=1, lengths=[1, 2, 3, 4, 4], ffn=64),
    _case('live-191-192-193', 3, 25, 7, 128, 32, seed=2, lengths=[15, 16, 17]),
    _case('live-177-and-no-padding', 2, 25, 7, 128, 32, seed=3, lengths=[1, 32]),
    _case('b1-partial-row-tile', 1, 25, 7, 128, 32, seed=4, lengths=[11]),
    _case('mc-padding-inside', 4, 25, 7, 128, 32, seed=5, mc=True, lengths=[7, 20, 1, 13], choice_lengths=[12, 1, 6, 3]),
    _case('heads10-d180', 3, 4, 6, 64, 8, heads=10, seed=6, lengths=[8, 3, 5]),
    _case('n16-c256', 2, 2, 16, 256, 6, seed=7, lengths=[6, 2]),
    _case('heads4-hd32', 3, 3, 5, 96, 7, heads=4, input_dim=30, seed=8, lengths=[7, 4, 1]),
    _case('heads2-hd6-ffn1024', 2, 2, 3, 32, 5, heads=2, input_dim=4, seed=9, lengths=[5, 2], ffn=1024),
    _case('b4-one-row-tile', 4, 3, 4, 64, 6, seed=10, lengths=[6, 1, 3, 5]),
    _case('b5-one-row-over', 5, 3, 4, 64, 6, seed=11, lengths=[2, 6, 4, 1, 5]),
    _case('L256-full', 2, 15, 16, 32, 15, seed=12, lengths=[15, 14]),
    _case('start-offset-strided', 3, 4, 7, 128, 8, seed=13, lengths=[8, 5, 2], T_all=12, start=[3, 0, 5], frame_offset=2, strided=True),
    _case('video-index-shuffled', 5, 3, 7, 128, 8, seed=14, lengths=[3, 8, 1, 6, 4], V=4, video_index=[3, 0, 0, 2, 1]),
]


def forward_case(case):
    """-> dict(cfg, sd, slots [V, T_all, N, C], tokens, pad, mc, video_index, start, frame_offset, T)"""
    mc = bool(case.get('mc'))
    ql = 20 if mc else case['text_len']
    cfg = config(case['T'], case['N'], case['C'], case['text_len'], case['heads'], case['input_dim'], case['nl'], case['ffn'], question_len=ql,
                 q_vocab=37, a_vocab=9, mlp=48)
    sd = seeded_weights(cfg, 7000 + case['seed'])
    slots = seeded_slots(8000 + case['seed'], case.get('V', case['B']), case.get('T_all', case['T']), case['N'], case['C'])
    tokens, pad = seeded_text(9000 + case['seed'], case['B'], case['text_len'], 37, lengths=case['lengths'], question_len=ql if mc else None,
                              choice_lengths=case.get('choice_lengths'))
    return dict(cfg=cfg, sd=sd, slots=slots, tokens=tokens, pad=pad, mc=mc, video_index=case.get('video_index'), start=case.get('start'),
                frame_offset=case.get('frame_offset', 1), T=case['T'])


def reference64(fc):
    return forward64(fc['sd'], fc['cfg'], fc['slots'], fc['tokens'], fc['pad'], fc['mc'], fc['video_index'], fc['start'], fc['frame_offset'], fc['T'])


def harness_case():
    """5 videos of 11 frames and 9 questions for harness.clevrer_answers: 5 descriptive, 4 multiple choice with 3, 1, 4, 2 choices; 4 frames per
    question at start + 2 t.  -> (cfg, sd, slots, questions: the collated arrays, T)"""
    T, N, C, text_len = 4, 7, 128, 32
    cfg = config(T, N, C, text_len, nl=2, q_vocab=37, a_vocab=9, mlp=48)
    sd = seeded_weights(cfg, 4242)
    slots = seeded_slots(4243, 5, 11, N, C)
    cls_tok, cls_pad = seeded_text(4244, 5, text_len, 37, lengths=[4, 20, 9, 1, 15])
    flag = np.repeat(np.arange(4), [3, 1, 4, 2])
    mc_tok, mc_pad = seeded_text(4245, 10, text_len, 37, lengths=np.repeat([6, 20, 11, 3], [3, 1, 4, 2]), question_len=20)
    q = dict(cls_q_tokens=cls_tok, cls_q_pad_mask=cls_pad, cls_video_index=np.array([4, 0, 2, 2, 1]), cls_start=np.array([0, 3, 1, 4, 2]),
             mc_q_tokens=mc_tok, mc_q_pad_mask=mc_pad, mc_flag=flag, mc_video_index=np.array([3, 3, 0, 1]), mc_start=np.array([2, 0, 4, 1]),
             frame_offset=2, num_frames=T)
    return cfg, sd, slots, q, T


def harness64(hc):
    """-> (descriptive logits [5, 9], multiple-choice logits [10]) of harness_case() in float64"""
    cfg, sd, slots, q, T = hc
    flag = q['mc_flag']
    return (forward64(sd, cfg, slots, q['cls_q_tokens'], q['cls_q_pad_mask'], False, q['cls_video_index'], q['cls_start'], 2, T),
            forward64(sd, cfg, slots, q['mc_q_tokens'], q['mc_q_pad_mask'], True, q['mc_video_index'][flag], q['mc_start'][flag], 2, T))
