"""What the tests of the PHYRE readout and of AUCCESS share (no test in here): seeded weights and inputs, a float64 restatement of the whole
readout written from the model's definition (slotformer/phyre_planning/models/readout.py: in_proj + temporal position row, CLS, pre-LN
nn.TransformerEncoder, cls_mlp on the CLS row) that also takes the planning driver's frame table (-1 = a frame of zeros), and a numpy
restatement of the AUCCESS loop of test_phyre_planning.py (collect_results)."""
import numpy as np
import torch
import torch.nn.functional as F

READOUT_DICT = dict(num_slots=8, slot_size=128, t_pe='sin', d_model=128, num_layers=4, num_heads=8, ffn_dim=512, norm_first=True, sel_slots=[0, 3])
FIXTURE = dict(B=6, T_all=4, seed=20240919)
EVAL_THRESHS = tuple(np.arange(0.1, 1, 0.2))
DEVICE_BAR = 1e-3       # the project's relative bar on the logits (of the largest |logit| of a case)
# |sigmoid(logit) - threshold| every seeded case keeps: sigmoid' <= 1/4, so the bar moves a confidence by at most DEVICE_BAR max|logit| / 4;
# four times that
THRESH_MARGIN = lambda logits: DEVICE_BAR * max(1.0, float(np.abs(logits).max()))  # noqa: E731

INVALID_INPUT, NOT_SOLVED = 0, -1


def readout_dict(N=8, C=128, sel=(0, 3), nl=4):
    return dict(READOUT_DICT, num_slots=N, slot_size=C, num_layers=nl, sel_slots=list(sel))


def state_shapes(rd):
    """[(key, shape)] of PHYREReadout(rd).state_dict(), in its order: the module's own parameters first, then the submodules."""
    d, C, ffn, T = rd['d_model'], rd['slot_size'], rd['ffn_dim'], len(rd['sel_slots'])
    out = [('CLS', (1, 1, d)), ('enc_t_pe', (1, T, d)), ('in_proj.weight', (d, C)), ('in_proj.bias', (d, ))]
    for i in range(rd['num_layers']):
        p = f'transformer_encoder.layers.{i}.'
        out += [(p + 'self_attn.in_proj_weight', (3 * d, d)), (p + 'self_attn.in_proj_bias', (3 * d, )), (p + 'self_attn.out_proj.weight', (d, d)),
                (p + 'self_attn.out_proj.bias', (d, )), (p + 'linear1.weight', (ffn, d)), (p + 'linear1.bias', (ffn, )), (p + 'linear2.weight', (d, ffn)),
                (p + 'linear2.bias', (d, )), (p + 'norm1.weight', (d, )), (p + 'norm1.bias', (d, )), (p + 'norm2.weight', (d, )), (p + 'norm2.bias', (d, ))]
    out += [('cls_mlp.0.weight', (d, d)), ('cls_mlp.0.bias', (d, )), ('cls_mlp.2.weight', (1, d)), ('cls_mlp.2.bias', (1, ))]
    return out


def sin_pos_enc(T, d):
    """enc_t_pe [1, T, d] in float64: the sinusoid table whose LAST row is position 0, sines then cosines (slotformer.py:10-16)."""
    inv_freq = 1.0 / (10000.0 ** (np.arange(0.0, d, 2.0) / d))
    phase = np.outer(np.arange(T - 1, -1, -1, dtype=np.float64), inv_freq)
    return np.concatenate([np.sin(phase), np.cos(phase)], -1)[None]


def seeded_weights(rd, seed):
    """{key: float32 tensor} for every entry of state_shapes(rd) from one numpy generator: nn.Linear-sized matrices, biases and LayerNorm
    parameters away from 0 / 1 (a wrong index must show), an O(1) CLS row; enc_t_pe is the closed form."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in state_shapes(rd):
        leaf = key.rsplit('.', 1)[-1]
        if key == 'enc_t_pe':
            a = sin_pos_enc(shape[1], shape[2])
        elif key == 'CLS':
            a = 0.5 * rng.standard_normal(shape)
        elif len(shape) == 2:
            a = rng.uniform(-1, 1, shape) * (1.5 / np.sqrt(shape[1]))
        elif 'norm' in key and leaf == 'weight':
            a = 1.0 + 0.1 * rng.standard_normal(shape)
        else:
            a = 0.1 * rng.uniform(-1, 1, shape)
        sd[key] = torch.from_numpy(np.asarray(a, np.float32))
    return sd


def seeded_slots(seed, V, T_all, N, C):
    return np.random.default_rng(seed).standard_normal((V, T_all, N, C)).astype(np.float32)


def layer64(sd, prefix, x, heads):
    """one pre-LN nn.TransformerEncoderLayer (relu, no dropout) on x [B, L, d] in float64"""
    g = lambda k: sd[prefix + k].double()  # noqa: E731
    B, L, d = x.shape
    hd = d // heads
    h = F.layer_norm(x, (d, ), g('norm1.weight'), g('norm1.bias'), 1e-5)
    q, k, v = F.linear(h, g('self_attn.in_proj_weight'), g('self_attn.in_proj_bias')).split(d, dim=-1)
    sp = lambda t: t.reshape(B, L, heads, hd).transpose(1, 2)  # noqa: E731
    a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / hd ** 0.5, dim=-1) @ sp(v)
    x2 = x + F.linear(a.transpose(1, 2).reshape(B, L, d), g('self_attn.out_proj.weight'), g('self_attn.out_proj.bias'))
    h2 = F.layer_norm(x2, (d, ), g('norm2.weight'), g('norm2.bias'), 1e-5)
    return x2 + F.linear(F.relu(F.linear(h2, g('linear1.weight'), g('linear1.bias'))), g('linear2.weight'), g('linear2.bias'))


def forward64(sd, rd, slots, table=None, video_index=None):
    """logits [B] in float64 (numpy).  slots [V, T_all, N, C]; table: the frame of every token group (default rd['sel_slots']; -1 = a frame of
    zeros; the position row is the PLACE in the table); video_index: the videos of the batch (default all, in order)."""
    s = torch.as_tensor(np.asarray(slots)).double()
    if video_index is not None:
        s = s[torch.as_tensor(np.asarray(video_index)).long()]
    table = list(rd['sel_slots'] if table is None else table)
    B, _, N, C = s.shape
    frames = torch.stack([torch.zeros(B, N, C, dtype=torch.float64) if f < 0 else s[:, f] for f in table], 1)   # [B, T, N, C]
    tok = F.linear(frames, sd['in_proj.weight'].double(), sd['in_proj.bias'].double()) + sd['enc_t_pe'].double()[0][None, :, None, :]
    x = torch.cat([sd['CLS'].double().expand(B, 1, -1), tok.flatten(1, 2)], 1)   # [B, 1 + T N, d]: t-major, slot-minor
    for i in range(rd['num_layers']):
        x = layer64(sd, f'transformer_encoder.layers.{i}.', x, rd['num_heads'])
    h = F.relu(F.linear(x[:, 0], sd['cls_mlp.0.weight'].double(), sd['cls_mlp.0.bias'].double()))
    return F.linear(h, sd['cls_mlp.2.weight'].double(), sd['cls_mlp.2.bias'].double())[:, 0].numpy()


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def loss64(logits, labels):
    x, y = np.asarray(logits, np.float64), np.asarray(labels, np.float64)
    return float(np.mean(np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))))


def hits64(logits, labels, thresh):
    """(sigmoid(logit) > thresh) == label, elementwise (the thresholds as the kernel holds them: float32)"""
    return (sigmoid64(logits) > float(np.float32(thresh))).astype(np.float64) == np.asarray(labels, np.float64)


def threshold_clearance(logits):
    """min over logits and the five thresholds of |sigmoid(logit) - threshold|"""
    p = sigmoid64(logits)
    return float(min(np.abs(p - float(np.float32(t))).min() for t in EVAL_THRESHS))


def fixture_case():
    """The inputs of tests/golden/phyre_readout.npz: the tool that wrote the file and the tests build them alike."""
    rd = readout_dict()
    sd = seeded_weights(rd, FIXTURE['seed'])
    slots = seeded_slots(FIXTURE['seed'] + 1, FIXTURE['B'], FIXTURE['T_all'], rd['num_slots'], rd['slot_size'])
    labels = (np.random.default_rng(FIXTURE['seed'] + 2).uniform(size=FIXTURE['B']) > 0.5).astype(np.float32)
    return rd, sd, slots, labels


# ---- the seeded cases of the GPU forward test ---------------------------------------------------------------------------------------------------
# B sequences of L = 1 + T N tokens; the layer launch puts 128 // L sequences in a workgroup: (7, 8) at L 17 are one workgroup exactly and one
# sequence over.  V: videos behind the batch (video_index picks B of them); strided: the slots are a view with larger video and frame strides.
def _case(name, B, N, T, C, sel, T_all, nl=4, seed=0, **kw):
    return dict(name=name, B=B, N=N, T=T, C=C, sel=list(sel), T_all=T_all, nl=nl, seed=seed, **kw)


FORWARD_CASES = [
    _case('b1', 1, 8, 2, 128, (0, 3), 4, seed=11),
    _case('b7-one-workgroup', 7, 8, 2, 128, (0, 3), 4, seed=32),
    _case('b8-one-over', 8, 8, 2, 128, (0, 3), 4, seed=13),
    _case('b23-n7-t3', 23, 7, 3, 128, (0, 2, 4), 5, seed=34),
    _case('n16-c256-L33', 3, 16, 2, 256, (1, 2), 3, seed=15),
    _case('n1-t1-c32-L2', 5, 1, 1, 32, (0, ), 2, seed=16),
    _case('n16-t5-c64-L81', 2, 16, 5, 64, (0, 1, 2, 3, 4), 5, seed=17),
    _case('sel-unsorted', 3, 8, 2, 128, (3, 0), 4, seed=18),
    _case('sel-repeated', 3, 8, 2, 128, (2, 2), 4, seed=19),
    _case('sel-zero-frame', 3, 8, 2, 128, (-1, 1), 4, seed=20),
    _case('strided-view', 3, 8, 2, 128, (0, 3), 4, seed=21, strided=True),
    _case('video-index', 5, 8, 2, 128, (0, 3), 4, seed=22, V=4, video_index=(3, 0, 0, 2, 1)),
    _case('one-layer', 9, 8, 2, 128, (0, 3), 4, nl=1, seed=23),
]


def forward_case(case):
    """-> (rd, sd, slots [V, T_all, N, C], table).  rd['sel_slots'] holds the table with its -1 entries replaced by 0 (a model's sel_slots are
    frame numbers); `table` is what the kernel and the restatement are given."""
    rd = readout_dict(case['N'], case['C'], [max(s, 0) for s in case['sel']], case['nl'])
    sd = seeded_weights(rd, 5000 + case['seed'])
    slots = seeded_slots(6000 + case['seed'], case.get('V', case['B']), case['T_all'], case['N'], case['C'])
    return rd, sd, slots, list(case['sel'])


# ---- AUCCESS ----------------------------------------------------------------------------------------------------------------------------------
def auccess_reference(conf, status):
    """What test_phyre_planning.py (collect_results) computes, restated: per task the valid actions sorted by falling confidence (argsort
    ascending, reversed, as there), "a solved action among the first k attempts" for k = 1..100, its mean over the tasks weighted by
    log(k + 1) - log(k) -> (auccess, success_rate [100], success table [tasks, 100], first_rank [tasks]: the place of the first solved action
    in that ranking, `actions` when there is none)."""
    conf, status = np.asarray(conf, np.float64), np.asarray(status)
    tasks, actions = conf.shape
    table = np.zeros((tasks, 100))
    first = np.full(tasks, actions, np.int64)
    for t in range(tasks):
        valid = status[t] != INVALID_INPUT
        ranked_solved = (status[t][valid] > 0)[np.argsort(conf[t][valid])[::-1]]
        hit = np.cumsum(ranked_solved) > 0            # hit[i]: a solved action among the first i + 1 attempts
        n = min(100, hit.size)
        table[t, :n] = hit[:n]
        table[t, n:] = hit[-1] if hit.size else 0     # fewer than 100 valid actions: the later attempts add nothing
        if ranked_solved.any():
            first[t] = int(np.argmax(ranked_solved))
    k = np.arange(1, 101, dtype=np.float64)
    w = np.log(k + 1) - np.log(k)
    rate = table.mean(0)
    return float(100.0 * (w * rate).sum() / w.sum()), rate, table, first


def _distinct_conf(rng, tasks, actions):
    """confidences without a tie inside a task: a permutation of (i + 0.5) / actions"""
    return np.stack([(rng.permutation(actions) + 0.5) / actions for _ in range(tasks)]).astype(np.float32)


def auccess_cases():
    """{name: (conf [tasks, actions] float32, status [tasks, actions] int32)}.  Every case but 'tie' has no two equal confidences in a task."""
    rng = np.random.default_rng(777)
    out = {}
    # three tasks x 257 actions (more than one pass of a 256-thread workgroup) with invalid actions; task 1 has no solved action; task 2 has
    # fewer than 100 valid actions
    conf = _distinct_conf(rng, 3, 257)
    status = rng.choice(np.array([INVALID_INPUT, NOT_SOLVED, NOT_SOLVED, NOT_SOLVED, 1, 2], np.int32), size=(3, 257))
    status[0, conf[0] > 0.97] = NOT_SOLVED   # (the first solved action of task 0 is not at the top)
    status[1][status[1] > 0] = NOT_SOLVED
    keep = rng.permutation(257)[:60]
    masked = np.full(257, INVALID_INPUT, np.int32)
    masked[keep] = np.where(rng.uniform(size=60) < 0.1, 1, NOT_SOLVED)
    masked[keep[np.argsort(conf[2][keep])[::-1][:3]]] = NOT_SOLVED   # (not at the top either)
    masked[keep[np.argsort(conf[2][keep])[::-1][5]]] = 1             # (but certainly one)
    status[2] = masked
    out['three-tasks'] = (conf, status.astype(np.int32))
    # a solved action first in the ranking; the only solved action last among the valid ones; invalid actions carry the highest confidences
    conf = _distinct_conf(rng, 2, 150)
    status = np.full((2, 150), NOT_SOLVED, np.int32)
    order0, order1 = np.argsort(conf[0])[::-1], np.argsort(conf[1])[::-1]
    status[0, order0[:4]] = INVALID_INPUT
    status[0, order0[4]] = 2
    status[0, order0[40]] = 1
    status[1, order1[:3]] = INVALID_INPUT
    status[1, order1[-1]] = 1
    out['first-and-last'] = (conf, status)
    # the tie rule: the best solved action shares its confidence with two failed ones; one failed action lies above
    conf = np.array([[0.9, 0.7, 0.7, 0.7, 0.2, 0.95, 0.1]], np.float32)
    status = np.array([[NOT_SOLVED, NOT_SOLVED, 1, NOT_SOLVED, 1, INVALID_INPUT, NOT_SOLVED]], np.int32)
    out['tie'] = (conf, status)
    return out


AUCCESS_EXPECTED_TIE_RANK = 1   # 0.9 lies above; the solved 0.7 wins against the two failed 0.7
