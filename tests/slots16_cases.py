"""The 9 .. 16-slot cases shared by tools/gen_golden_slots16.py (which writes their fixtures) and the tests that read them:
name -> (configuration, arguments of the tools/gen_golden.py case function)."""
import golden_util as gu

SAVI_N9 = gu.savi_cfg(64, 9, iters=3, kernel_mlp=True, pred='transformer', rnn=True, kld='none')        # Transformer + LSTM predictor, 3 iterations
SAVI_N11 = gu.savi_cfg(64, 11, iters=2, kernel_mlp=False, pred='mlp', rnn=False, kld='var-0.01')          # the C2 form (stochastic, MLP predictor)
SAVI_N16 = gu.savi_cfg(64, 16, iters=2, kernel_mlp=True, pred='transformer', rnn=True, kld='none')       # the C1 form
ROLL_N11 = gu.rollout_cfg(11, 128, 6, 256, 4, 8, 1024, rollout_len=4)

SAVI_CASES = {
    'savi_n9': (SAVI_N9, dict(B=1, T=2, seed=109)),
    'savi_n11': (SAVI_N11, dict(B=2, T=3, seed=111, noise_seed=7)),
    'savi_n16': (SAVI_N16, dict(B=2, T=3, seed=116)),
}
ROLL_CASES = {'roll_n11': (ROLL_N11, dict(B=2, pred_len=4, seed=211))}
SAVI_TRAIN_CASES = {'savi_train_n11': (SAVI_N11, dict(B=1, T=2, seed=311, noise_seed=9))}


def register(cfg):
    """The tests reused from the 8-slot suite look a configuration up by NAME on golden_util: give this one a name there, and return it."""
    name = 'SLOTS16_SAVI_N%d' % cfg['slot_dict']['num_slots']
    setattr(gu, name, cfg)
    return name
