"""The float64 reference of every case of tests/decode_cases.py, held to the conditions without which the segmentation checks of
tests/test_decode_gpu.py would compare all-background frames: both sides of the threshold are populated, several labels occur, and almost
no pixel sits on a decision of the rule."""
import pytest
import torch

import decode_cases as dc


@pytest.mark.parametrize('name', dc.NAMES)
def test_reference_exercises_the_segmentation_rule(name):
    res, N, D, ch, r, ks, F_ = dc.CASES[name]
    ref = dc.reference(name)
    assert ref['masks'].dtype == torch.float64 and ref['masks'].shape == (F_, N, 1, res, res)
    assert ref['logits'].shape == ref['masks'].shape and ref['recons'].shape == (F_, N, 3, res, res)
    assert torch.equal(torch.softmax(ref['logits'], 1), ref['masks'])
    total = ref['best'].numel()
    below = ref['below'].sum().item() / total
    labels = [len(torch.unique(s)) for s in ref['seg']]
    tie, edge = ref['tie'].sum().item() / total, ref['edge'].sum().item() / total
    excluded = ref['excluded'].sum().item() / total
    print(f'{name}: below the threshold {below:.4f}, labels per frame {labels}, top-2 ties {tie:.5f}, at the threshold {edge:.5f}, '
          f'ambiguous frames {int(ref["ambiguous"].sum())}, excluded {excluded:.5f}')
    assert below >= 0.20 and 1. - below >= 0.15
    assert min(labels) >= 3
    assert excluded <= 0.01
    # a below-threshold pixel really goes to a slot that is not its argmax somewhere: the two rules differ on this case
    assert (ref['seg'] != ref['masks'].squeeze(2).argmax(1)).any()
