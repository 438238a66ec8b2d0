"""CPU: the LPIPS parameter container (names, shapes, loading), the host twin of the weight packing, the float64 restatement on cases with a
closed form, and the argument errors / workspace query of the C entry points (all raised before any device work)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_cases as lc


def test_state_dict_names_and_shapes():
    from slotformer_amd.lpips import LPIPS
    sd = LPIPS().state_dict()
    want = lc.expected_keys()
    assert set(sd) == set(want), set(sd) ^ set(want)
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
        assert sd[k].dtype == torch.float32
    assert torch.equal(sd['scaling_layer.shift'].flatten(), torch.tensor(lc.SHIFT))
    assert torch.equal(sd['scaling_layer.scale'].flatten(), torch.tensor(lc.SCALE))
    # the explicit names of the issue, not only the table of lpips_cases
    for k in ('net.slice1.0.weight', 'net.slice1.2.bias', 'net.slice2.5.weight', 'net.slice2.7.weight', 'net.slice3.10.weight', 'net.slice3.12.bias',
              'net.slice3.14.weight', 'net.slice4.17.weight', 'net.slice4.19.weight', 'net.slice4.21.bias', 'net.slice5.24.weight',
              'net.slice5.26.weight', 'net.slice5.28.bias', 'lin0.model.1.weight', 'lin4.model.1.weight'):
        assert k in sd
    assert len(sd) == 13 * 2 + 5 + 2


def test_loads_package_state_dict_with_duplicate_lins_keys():
    from slotformer_amd.lpips import LPIPS
    sd = lc.seeded_weights(3)
    extra = dict(sd)
    for i in range(5):
        extra[f'lins.{i}.model.1.weight'] = sd[f'lin{i}.model.1.weight'].clone()
    m = LPIPS()
    m.load_state_dict(extra)
    got = m.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'net.slice3.12.bias'})   # still strict about its own names


def test_torchvision_and_linear_files_fill_the_same_tensors():
    from slotformer_amd.lpips import LPIPS, load_vgg_and_linear
    sd = lc.seeded_weights(4)
    vgg = {}
    for name, _, _ in lc.CONVS:
        n = name.split('.')[-1]
        vgg[f'features.{n}.weight'], vgg[f'features.{n}.bias'] = sd[name + '.weight'], sd[name + '.bias']
    vgg['classifier.0.weight'] = torch.zeros(4, 4)   # the rest of a torchvision VGG16 is ignored
    lin = {f'lin{i}.model.1.weight': sd[f'lin{i}.model.1.weight'] for i in range(5)}
    lin.update({f'lins.{i}.model.1.weight': sd[f'lin{i}.model.1.weight'] for i in range(5)})
    a, b = load_vgg_and_linear(LPIPS(), vgg, lin).state_dict(), LPIPS()
    b.load_state_dict(sd)
    b = b.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_unsupported_options_raise():
    from slotformer_amd.lpips import LPIPS
    for kw in ({'net': 'alex'}, {'net': 'squeeze'}, {'spatial': True}, {'lpips': False}):
        with pytest.raises(NotImplementedError):
            LPIPS(**kw)
    m = LPIPS()
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError):
        m(x, x, retPerLayer=True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):   # CPU tensors: an error, not another path
        m(x, x)


def _bf16_to_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize('cin,cout', [(64, 64), (64, 128), (256, 512)])
def test_host_pack_layout_and_remainder(cin, cout):
    """sf_lpips_pack_conv_weights_host, then the unpack the header's layout describes: hi + lo is the weight to 2^-16 relative"""
    from slotformer_amd import _lib
    lib = _lib.lib()
    w = lc.seeded_weights(5)[{(64, 64): 'net.slice1.2', (64, 128): 'net.slice2.5', (256, 512): 'net.slice4.17'}[(cin, cout)] + '.weight'].numpy()
    n = cout * cin * 9
    buf = np.zeros(2 * n, dtype=np.uint16)
    assert lib.sf_lpips_pack_conv_weights_host(w.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), cout, cin) == 0
    KC = cin // 16
    co, ci, tap = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(9), indexing='ij')
    ct, r, cc, h, j = co // 32, co % 32, ci // 16, (ci % 16) // 8, ci % 8
    idx = (((ct * 9 * KC + tap * KC + cc) * 64) + h * 32 + r) * 8 + j
    assert len(np.unique(idx)) == n and idx.max() == n - 1          # a permutation of the plane
    hi, lo = _bf16_to_f32(buf[:n])[idx], _bf16_to_f32(buf[n:])[idx]
    wf = w.reshape(cout, cin, 9)
    assert np.array_equal(hi, torch.from_numpy(wf).bfloat16().float().numpy())   # hi is the round-to-nearest-even bf16
    rem = np.abs((hi.astype(np.float64) + lo.astype(np.float64)) - wf.astype(np.float64))
    assert (rem <= 2. ** -16 * np.abs(wf)).all(), (rem / np.abs(wf)).max()


def test_host_pack_first_layer_is_k_major_f32():
    from slotformer_amd import _lib
    w = lc.seeded_weights(5)['net.slice1.0.weight'].numpy()
    out = np.zeros((27, 64), dtype=np.float32)
    assert _lib.lib().sf_lpips_pack_conv_weights_host(w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 64, 3) == 0
    assert np.array_equal(out, w.reshape(64, 27).T)


def test_restatement_identical_inputs_give_zero():
    sd = lc.seeded_weights(0)
    x, _ = lc.frames(2, 16, 16)
    assert torch.equal(lc.restate64(sd, x, x.clone()), torch.zeros(2, dtype=torch.float64))
    assert torch.equal(lc.emulate32(sd, x, x.clone()), torch.zeros(2))


def test_restatement_single_tap_weight_gives_that_taps_term():
    """all tap weights zero except one channel of the first tap: the score is the mean over the pixels of that weight times the squared
    difference of that channel of the normalised relu1_2 features, written out here without the restatement's helpers"""
    sd = lc.seeded_weights(0)
    x, y = lc.frames(1, 16, 16)
    for i in range(5):
        sd[f'lin{i}.model.1.weight'] = torch.zeros_like(sd[f'lin{i}.model.1.weight'])
    sd['lin0.model.1.weight'][0, 7, 0, 0] = 0.25

    def relu1_2(v):
        v = (v.double() - torch.tensor(lc.SHIFT).double().view(1, 3, 1, 1)) / torch.tensor(lc.SCALE).double().view(1, 3, 1, 1)
        v = F.relu(F.conv2d(v, sd['net.slice1.0.weight'].double(), sd['net.slice1.0.bias'].double(), padding=1))
        return F.relu(F.conv2d(v, sd['net.slice1.2.weight'].double(), sd['net.slice1.2.bias'].double(), padding=1))[0]

    fx, fy = relu1_2(x), relu1_2(y)
    want = 0.
    for py in range(16):
        for px in range(16):
            a, b = fx[:, py, px], fy[:, py, px]
            want += 0.25 * (a[7] / (a.norm() + 1e-10) - b[7] / (b.norm() + 1e-10)) ** 2
    want = want / 256
    got = lc.restate64(sd, x, y)
    assert got.shape == (1, ) and abs(got[0].item() - want.item()) <= 1e-12 * abs(want.item())
    per_tap = lc.restate64(sd, x, y, per_tap=True)
    assert torch.equal(per_tap[1:], torch.zeros(4, 1, dtype=torch.float64)) and per_tap[0, 0] == got[0]


def test_restatement_reaches_one_pixel_at_20x28():
    """20 x 28 -> 10 x 14 -> 5 x 7 -> 2 x 3 -> 1 x 1 under the floor of the pool: the last tap is one pixel, its term needs no mean"""
    sd = lc.seeded_weights(0)
    x, y = lc.frames(1, 20, 28)
    a = torch.cat([x, y]).double()
    a = (a - sd['scaling_layer.shift'].double()) / sd['scaling_layer.scale'].double()
    shapes = []
    for s, (l0, l1) in enumerate(lc.SLICES):
        if s:
            a = F.max_pool2d(a, 2, 2)
        for name, _, _ in lc.CONVS[l0:l1]:
            a = F.relu(F.conv2d(a, sd[name + '.weight'].double(), sd[name + '.bias'].double(), padding=1))
        shapes.append(tuple(a.shape[2:]))
    assert shapes == [(20, 28), (10, 14), (5, 7), (2, 3), (1, 1)]
    fx, fy = a[0, :, 0, 0], a[1, :, 0, 0]
    w = sd['lin4.model.1.weight'].double().flatten()
    last = (w * (fx / (fx.norm() + 1e-10) - fy / (fy.norm() + 1e-10)) ** 2).sum()
    per_tap = lc.restate64(sd, x, y, per_tap=True)
    assert abs(per_tap[4, 0].item() - last.item()) <= 1e-12 * abs(last.item()) and last.item() > 0


def test_emulation_is_close_to_float64():
    """the arithmetic the kernels use costs a few 1e-6 relative on the test inputs (what the GPU tests' bound is made of)"""
    _, _, _, ref, emu = lc.case(2, 16, 16)
    assert 1e-4 < ref.min().item() and ref.max().item() < 1e-1      # distances of the expected size: no relative bound on a cancelled value
    assert 0. < lc.rel(emu, ref) < 5e-5


def test_workspace_query():
    from slotformer_amd import _lib
    lib = _lib.lib()
    a, b, c = (lib.sf_lpips_workspace_bytes(32, 32, k) for k in (1, 2, 5))
    assert 0 < a < b < c
    assert a >= 2 * (2 * 32 * 32 * 64 * 4)            # two activation buffers of both images at the first stage
    assert lib.sf_lpips_workspace_bytes(15, 32, 2) == 0 and lib.sf_lpips_workspace_bytes(32, 15, 2) == 0
    assert lib.sf_lpips_workspace_bytes(16, 16, 1) > 0
    assert lib.sf_lpips_workspace_bytes(32, 32, 0) == 0 and lib.sf_lpips_workspace_bytes(4096, 4096, 64) == 0


def test_argument_errors_without_gpu():
    from slotformer_amd import _lib
    lib = _lib.lib()

    def err():
        return lib.sf_last_error_string().decode()

    one = C.c_void_p(16)   # a non-null dummy pointer: every case below is rejected before it is dereferenced
    m = _lib.sf_lpips_model()
    big = 1 << 40
    assert lib.sf_lpips_f32(None, one, one, one, 2, 32, 32, 2, 0, one, big, None) < 0 and 'null pointer' in err()
    assert lib.sf_lpips_f32(C.byref(m), one, None, one, 2, 32, 32, 2, 0, one, big, None) < 0 and 'null pointer' in err()
    assert lib.sf_lpips_f32(C.byref(m), one, one, one, 2, 32, 32, 2, 0, None, big, None) < 0 and 'null pointer' in err()
    assert lib.sf_lpips_f32(C.byref(m), one, one, one, 2, 15, 32, 2, 0, one, big, None) < 0 and 'at least 16' in err()
    assert lib.sf_lpips_f32(C.byref(m), one, one, one, 2, 32, 8, 2, 0, one, big, None) < 0 and 'at least 16' in err()
    assert lib.sf_lpips_f32(C.byref(m), one, one, one, 2, 32, 32, 0, 0, one, big, None) < 0 and 'chunk' in err()
    need = lib.sf_lpips_workspace_bytes(32, 32, 2)
    assert lib.sf_lpips_f32(C.byref(m), one, one, one, 2, 32, 32, 2, 0, one, need - 1, None) < 0 and 'workspace too small' in err()
    # a model with null members is rejected too (here: all of them), before any launch
    assert lib.sf_lpips_f32(C.byref(m), one, one, one, 2, 32, 32, 2, 0, one, need, None) < 0 and 'null pointer in the model' in err()
    assert lib.sf_lpips_pack_conv_weights(None, one, 64, 64, None) < 0 and 'null pointer' in err()
    assert lib.sf_lpips_pack_conv_weights(one, one, 64, 96, None) < 0 and 'channel counts' in err()
    assert lib.sf_lpips_pack_conv_weights_host(one, None, 64, 64) < 0 and 'null pointer' in err()
    assert lib.sf_lpips_pack_conv_weights_host(one, one, 32, 3) < 0 and 'channel counts' in err()
    assert lib.sf_lpips_mean_over_videos_f32(None, one, one, 2, 3, None) < 0 and 'null pointer' in err()
    assert lib.sf_lpips_mean_over_videos_f32(one, None, None, 2, 3, None) < 0 and 'null pointer' in err()
    assert lib.sf_lpips_mean_over_videos_f32(one, one, one, 0, 3, None) < 0 and 'bad shape' in err()
