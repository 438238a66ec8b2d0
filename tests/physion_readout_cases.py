"""What the tests of the Physion readout share (no test in here): seeded inputs, float64 restatements of PhysionReadout's forward, loss, accuracy
and gradients written from the model's definition (slotformer/physion_vqa/models/readout.py) -- the gradient restatement TAKES the routing
(t_star, pair_star) as arguments, so that a kernel is compared at the route it took -- and a float32 emulation of the kernels' split-bf16
products, whose distance from float64 sets the forward tolerance (the rule of tests/test_dvae_tokens_gpu.py)."""
from itertools import combinations

import numpy as np
import torch

AGGS = ('max', 'sum', 'mean')
FIXTURE_SHAPE = dict(B=4, T=5, N=6, C=192, F=192)
FIXTURE_SEED = 20240607
EVAL_THRESHS = tuple(np.arange(0.1, 1, 0.2))


def seeded_case(seed, B, T, N, C, F, K=1):
    """slots [B,T,N,C], W1 [K,F,2C], b1 [K,F], w2 [K,F], b2 [K] (float32) from one numpy generator: unit-normal slots, nn.Linear-sized weights."""
    rng = np.random.default_rng(seed)
    slots = rng.standard_normal((B, T, N, C)).astype(np.float32)
    a1, a2 = 1.0 / np.sqrt(2 * C), 1.0 / np.sqrt(F)
    W1 = rng.uniform(-a1, a1, (K, F, 2 * C)).astype(np.float32)
    b1 = rng.uniform(-a1, a1, (K, F)).astype(np.float32)
    w2 = rng.uniform(-a2, a2, (K, F)).astype(np.float32)
    b2 = rng.uniform(-a2, a2, (K, )).astype(np.float32)
    return slots, W1, b1, w2, b2


def fixture_case(agg):
    """The inputs of tests/golden/physion_readout.npz for one aggregate: the tool that wrote the file and the tests build them alike."""
    s = FIXTURE_SHAPE
    slots, W1, b1, w2, b2 = seeded_case(FIXTURE_SEED + AGGS.index(agg), s['B'], s['T'], s['N'], s['C'], s['F'])
    labels = (np.random.default_rng(FIXTURE_SEED).uniform(size=s['B']) > 0.5).astype(np.float32)
    return slots, W1, b1, w2, b2, labels


def pairs_of(N):
    return list(combinations(range(N), 2))


def relation64(slots, W1, b1, N):
    """[B,T,pairs,F] float64: linear1 of every slot pair (one head)."""
    s = slots.astype(np.float64)
    C = s.shape[-1]
    W = W1.astype(np.float64)
    U = s @ W[:, :C].T + b1.astype(np.float64)
    V = s @ W[:, C:].T
    pi, pj = np.array(pairs_of(N)).T
    return U[:, :, pi] + V[:, :, pj]


def aggregate64(rel, agg):
    return rel.max(2) if agg == 'max' else rel.sum(2) if agg == 'sum' else rel.mean(2)


def forward64(slots, W1, b1, w2, b2, agg):
    """K heads -> dict(steps [K,B,T], logits [K,B], t_star [K,B] (first maximum), rel: list of [B,T,pairs,F]) in float64."""
    N = slots.shape[2]
    steps, rels = [], []
    for k in range(W1.shape[0]):
        rel = relation64(slots, W1[k], b1[k], N)
        rels.append(rel)
        steps.append(aggregate64(rel, agg) @ w2[k].astype(np.float64) + float(b2[k]))
    steps = np.stack(steps)
    return dict(steps=steps, logits=steps.max(2), t_star=steps.argmax(2), rel=rels)


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def loss64(logits, labels):
    """mean BCE-with-logits."""
    x, y = np.asarray(logits, np.float64), np.asarray(labels, np.float64)
    return float(np.mean(np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))))


def dloss64(logits, labels):
    return (sigmoid64(logits) - np.asarray(labels, np.float64)) / np.size(logits)


def hits64(logits, labels, thresh):
    """(sigmoid(logit) > thresh) == label, elementwise (the thresholds as the kernel holds them: float32)."""
    return (sigmoid64(logits) > float(np.float32(thresh))).astype(np.float64) == np.asarray(labels, np.float64)


def grads64(slots, W1, b1, w2, agg, g, t_star, pair_star=None):
    """Gradients of one head given g [B] = dL/dlogit and the ROUTE: t_star [B], and for max pair_star [B,F] (the pair each feature's maximum is
    taken at).  -> dW1 [F,2C], db1 [F], dw2 [F], db2 (float64)."""
    B, _, N, C = slots.shape
    F = W1.shape[0]
    pr = pairs_of(N)
    dW1, db1, dw2 = np.zeros((F, 2 * C)), np.zeros(F), np.zeros(F)
    W = W1.astype(np.float64)
    fs = np.arange(F)
    for b in range(B):
        s = slots[b, t_star[b]].astype(np.float64)   # [N,C]
        U, V = s @ W[:, :C].T + b1.astype(np.float64), s @ W[:, C:].T
        rel = np.stack([U[i] + V[j] for i, j in pr])   # [pairs,F]
        dR = g[b] * w2.astype(np.float64)
        if agg == 'max':
            R = rel[pair_star[b], fs]
            coef = np.zeros((len(pr), F))
            coef[pair_star[b], fs] = dR
        else:
            R = rel.sum(0) if agg == 'sum' else rel.mean(0)
            coef = np.tile(dR if agg == 'sum' else dR / len(pr), (len(pr), 1))
        dw2 += g[b] * R
        db1 += coef.sum(0)
        for p, (i, j) in enumerate(pr):
            dW1[:, :C] += np.outer(coef[p], s[i])
            dW1[:, C:] += np.outer(coef[p], s[j])
    return dW1, db1, dw2, float(np.sum(g))


def _split(x):
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def emulate_f32(slots, W1, b1, w2, b2, agg):
    """The kernels' arithmetic in float32 on the host: operands as bf16 hi + bf16 lo, the three products hi.lo + lo.hi + hi.hi accumulated in
    float32, pairs added, aggregated and dotted in float32.  -> steps [K,B,T] (float64 view of the float32 result)."""
    s = torch.from_numpy(slots)
    N, C = s.shape[2:]
    sh, sl = _split(s)
    pi, pj = torch.tensor(pairs_of(N)).T
    out = []
    for k in range(W1.shape[0]):
        wh, wl = _split(torch.from_numpy(W1[k]))

        def prod(cols):
            return sh @ wl[:, cols].T + sl @ wh[:, cols].T + sh @ wh[:, cols].T

        U = prod(slice(0, C)) + torch.from_numpy(b1[k])
        V = prod(slice(C, 2 * C))
        rel = U[:, :, pi] + V[:, :, pj]
        R = rel.max(2).values if agg == 'max' else rel.sum(2) if agg == 'sum' else rel.sum(2) * np.float32(1.0 / len(pi))
        out.append((R @ torch.from_numpy(w2[k]) + float(b2[k])).double().numpy())
    return np.stack(out)


def emulation_distance(case, agg):
    """max |emulated - float64| over the step logits, relative to the largest |logit| of the case."""
    ref = forward64(*case, agg)
    emu = emulate_f32(*case, agg)
    return float(np.abs(emu - ref['steps']).max() / np.abs(ref['logits']).max())


# ---- the seeded cases of the GPU tests: (B, T, N, C, F, K, agg) ------------------------------------------------------------------------------
# every value of an axis with N 6 / C 192 / F 192, and at least once with another value of every other axis
FORWARD_CASES = [
    (1, 1, 6, 192, 192, 1, 'max'), (3, 7, 6, 192, 192, 1, 'sum'), (3, 8, 6, 192, 192, 3, 'mean'), (3, 75, 6, 192, 192, 1, 'max'),
    (1, 75, 6, 192, 192, 3, 'sum'), (3, 7, 2, 192, 192, 1, 'max'), (3, 8, 7, 192, 192, 1, 'mean'), (1, 7, 16, 192, 192, 1, 'max'),
    (3, 8, 6, 64, 32, 1, 'max'), (1, 7, 6, 256, 256, 3, 'max'), (3, 1, 2, 64, 32, 3, 'sum'), (1, 8, 7, 256, 256, 1, 'sum'),
    (3, 7, 16, 64, 32, 3, 'mean'), (1, 75, 7, 64, 32, 1, 'mean'), (3, 1, 16, 256, 256, 1, 'sum'), (1, 8, 2, 256, 256, 3, 'mean'),
    (3, 75, 2, 64, 32, 1, 'sum'), (1, 1, 7, 192, 192, 3, 'max'),
]
BACKWARD_CASES = [
    (1, 1, 6, 192, 192, 'max'), (5, 7, 6, 192, 192, 'max'), (64, 7, 6, 192, 192, 'max'), (5, 7, 6, 192, 192, 'sum'), (5, 1, 6, 192, 192, 'mean'),
    (5, 7, 2, 192, 192, 'sum'), (1, 7, 7, 192, 192, 'mean'), (64, 1, 2, 64, 32, 'max'), (5, 1, 7, 64, 32, 'max'), (1, 7, 2, 64, 32, 'mean'),
    (64, 7, 7, 64, 32, 'sum'),
]

# the other seeded inputs of the GPU tests (ties and planted maxima; repeated video_index entries): (seeded_case arguments, aggregate)
OTHER_GPU_CASES = [((77, 3, 12, 6, 192, 192, 1), 'max'), ((8, 3, 9, 6, 192, 192, 3), 'sum')]


def case_seed(shape):
    return 1000 + sum((i + 1) * 7919 * int(v if not isinstance(v, str) else AGGS.index(v)) for i, v in enumerate(shape)) % 100000


def forward_case(shape):
    B, T, N, C, F, K, _ = shape
    return seeded_case(case_seed(shape), B, T, N, C, F, K)


def backward_case(shape):
    B, T, N, C, F, _ = shape
    return seeded_case(case_seed(shape), B, T, N, C, F, 1)
