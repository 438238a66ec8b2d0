"""What tests/test_base_fit.py (CPU) and tests/test_base_fit_gpu.py share: the smallest shapes `base_slots.fit` takes -- 4 videos of 6 frames at
64 x 64, batches of 2 clips x 2 frames -- the three seeded models and a seeded frame table."""
import numpy as np
import torch

import golden_util as gu

V, T, RES, N_FRAMES, BATCH = 4, 6, 64, 2, 2
SEED = 11


def savi(kld='var-0.01'):
    cfg = dict(gu.TRAIN_SAVI)
    cfg['loss_dict'] = dict(cfg['loss_dict'], kld_method=kld)
    return _seeded(gu.ParamsView(cfg), 21)


def steve(fused=False, img_loss=False):
    cfg = gu.steve_tokens_cfg()
    cfg['loss_dict'] = dict(use_img_recon_loss=img_loss)
    m = _seeded(gu.ParamsView(cfg), 22)
    m.fused_token_loss = fused
    return m


def dvae():
    return _seeded(gu.ParamsView(dict(model='dVAE', vocab_size=64)), 23)


def _seeded(params, seed):
    """The model with its state drawn from gu.seeded_state_dict (closed-form entries keep their constructed values)."""
    from slotformer_amd.base_slots import build_model
    m = build_model(params)
    sd = m.state_dict()
    m.load_state_dict(gu.seeded_state_dict([(k, tuple(v.shape)) for k, v in sd.items()], seed, keep=sd))
    return m


def smooth_frames(seed=5):
    """uint8 [V, T, RES, RES, 3]: a few low-frequency waves per video, drifting from frame to frame -- something a dVAE can learn in a few steps."""
    rs = np.random.RandomState(seed)
    y, x = np.meshgrid(np.linspace(0, 1, RES), np.linspace(0, 1, RES), indexing='ij')
    out = np.zeros((V, T, RES, RES, 3), np.float64)
    for v in range(V):
        for c in range(3):
            fy, fx, ph = rs.uniform(0.5, 3., 3)
            for t in range(T):
                out[v, t, :, :, c] = 0.5 + 0.45 * np.sin(2 * np.pi * (fy * y + fx * x) + ph + 0.3 * t)
    return torch.from_numpy(np.round(out * 255).astype(np.uint8))


def random_frames(seed=6):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (V, T, RES, RES, 3)).astype(np.uint8))
