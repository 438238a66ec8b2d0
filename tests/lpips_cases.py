"""Weights, inputs and two independent restatements of LPIPS (VGG16) shared by tests/test_lpips.py (CPU) and tests/test_lpips_gpu.py:

  restate64   the definition in float64 torch CPU operations (F.conv2d, F.max_pool2d, the tap formulas);
  emulate32   the same network in float32 with the arithmetic of csrc/lpips.hip: the first layer in f32, every later convolution on bf16 hi | lo
              operands with the three products x_lo.w_hi + x_hi.w_lo + x_hi.w_hi (bf16 x bf16 is exact in f32, so an f32 F.conv2d on bf16-valued
              tensors is that product up to the order of the sum), and every layer's output stored as hi + lo.

The distance of emulate32 from restate64 is what the arithmetic costs; the GPU tests allow the device four times that (it sums a 9 * Cin long
chain in another order than F.conv2d does)."""
import functools

import torch
import torch.nn.functional as F

# (state-dict prefix, Cin, Cout) of the thirteen convolutions; a pool precedes the first convolution of slices 2-5; a tap follows every slice
CONVS = (('net.slice1.0', 3, 64), ('net.slice1.2', 64, 64),
         ('net.slice2.5', 64, 128), ('net.slice2.7', 128, 128),
         ('net.slice3.10', 128, 256), ('net.slice3.12', 256, 256), ('net.slice3.14', 256, 256),
         ('net.slice4.17', 256, 512), ('net.slice4.19', 512, 512), ('net.slice4.21', 512, 512),
         ('net.slice5.24', 512, 512), ('net.slice5.26', 512, 512), ('net.slice5.28', 512, 512))
SLICES = ((0, 2), (2, 4), (4, 7), (7, 10), (10, 13))
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def expected_keys():
    """name -> shape of LPIPS(net='vgg').state_dict() as the public package saves it"""
    out = {}
    for name, cin, cout in CONVS:
        out[name + '.weight'] = (cout, cin, 3, 3)
        out[name + '.bias'] = (cout, )
    for i, c in enumerate(TAP_CHANNELS):
        out[f'lin{i}.model.1.weight'] = (1, c, 1, 1)
    out['scaling_layer.shift'] = (1, 3, 1, 1)
    out['scaling_layer.scale'] = (1, 3, 1, 1)
    return out


def seeded_weights(seed=0):
    """He-scaled convolution weights, small biases, non-negative tap weights (float32, CPU), under the package's names"""
    g = torch.Generator().manual_seed(1000 + seed)
    sd = {}
    for name, cin, cout in CONVS:
        sd[name + '.weight'] = torch.randn(cout, cin, 3, 3, generator=g) * (2. / (9 * cin)) ** 0.5
        sd[name + '.bias'] = torch.randn(cout, generator=g) * 0.05
    for i, c in enumerate(TAP_CHANNELS):
        sd[f'lin{i}.model.1.weight'] = torch.rand(1, c, 1, 1, generator=g) * (2. / c)
    sd['scaling_layer.shift'] = torch.tensor(SHIFT)[None, :, None, None]
    sd['scaling_layer.scale'] = torch.tensor(SCALE)[None, :, None, None]
    return sd


def frames(n, H, W, seed=0, sigma=0.1):
    """x uniform in [-1, 1], y = x + N(0, sigma) clamped: [n,3,H,W] float32 each"""
    g = torch.Generator().manual_seed(77 + seed + 1000 * H + W)
    x = torch.rand(n, 3, H, W, generator=g) * 2 - 1
    y = (x + sigma * torch.randn(n, 3, H, W, generator=g)).clamp(-1, 1)
    return x, y


def _tap(fx, fy, w):
    nx = fx / (fx.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    ny = fy / (fy.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return (w.view(1, -1, 1, 1) * (nx - ny) ** 2).sum(1).mean((1, 2))


def restate64(sd, x, y, normalize=False, per_tap=False):
    """[n,3,H,W] x 2 -> [n] float64 (per_tap: [5,n])"""
    n = x.shape[0]
    a = torch.cat([x, y]).double()
    if normalize:
        a = 2 * a - 1
    a = (a - sd['scaling_layer.shift'].double()) / sd['scaling_layer.scale'].double()
    taps = []
    for s, (l0, l1) in enumerate(SLICES):
        if s:
            a = F.max_pool2d(a, 2, 2)
        for name, _, _ in CONVS[l0:l1]:
            a = F.relu(F.conv2d(a, sd[name + '.weight'].double(), sd[name + '.bias'].double(), padding=1))
        taps.append(_tap(a[:n], a[n:], sd[f'lin{s}.model.1.weight'].double().reshape(-1)))
    taps = torch.stack(taps)
    return taps if per_tap else taps.sum(0)


def split(a):
    hi = a.bfloat16().float()
    return hi, (a - hi).bfloat16().float()


def emulate32(sd, x, y, normalize=False):
    """[n,3,H,W] x 2 -> [n] float32 with the kernel's arithmetic"""
    n = x.shape[0]
    a = torch.cat([x, y]).float()
    if normalize:
        a = 2 * a - 1
    a = (a - sd['scaling_layer.shift']) / sd['scaling_layer.scale']
    total = 0.
    layer = 0
    for s, (l0, l1) in enumerate(SLICES):
        if s:
            a = F.max_pool2d(a, 2, 2)
        for name, _, _ in CONVS[l0:l1]:
            w, b = sd[name + '.weight'], sd[name + '.bias']
            if layer == 0:
                a = F.conv2d(a, w, b, padding=1)
            else:
                xh, xl = split(a)
                wh, wl = split(w)
                a = F.conv2d(xl, wh, None, padding=1) + F.conv2d(xh, wl, None, padding=1) + F.conv2d(xh, wh, None, padding=1) + b.view(1, -1, 1, 1)
            hi, lo = split(F.relu(a))
            a = hi + lo
            layer += 1
        total = total + _tap(a[:n], a[n:], sd[f'lin{s}.model.1.weight'].reshape(-1))
    return total


@functools.lru_cache(maxsize=None)
def case(n, H, W, seed=0, wseed=0):
    """(sd, x, y, float64 reference [n], emulation [n]) of a seeded case, computed once per process and shared; treat as read-only"""
    with torch.no_grad():
        sd = seeded_weights(wseed)
        x, y = frames(n, H, W, seed)
        return sd, x, y, restate64(sd, x, y), emulate32(sd, x, y).double()


def rel(a, b):
    """max relative distance of a from the reference b, per pair"""
    return ((a.double() - b.double()).abs() / b.double().abs()).max().item()
