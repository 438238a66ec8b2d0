"""LPIPS with the VGG16 backbone on the HIP library (csrc/lpips.hip): what the reference's evaluation takes as `lpips.LPIPS(net='vgg')`
(test_vp.py:21-23) and calls through `perceptual_dist` (vp_utils.py:109-111).

`LPIPS` is a parameter container with the state-dict names of the public `lpips` package, so `load_state_dict` takes what that package saves;
`load_vgg_and_linear` fills it from a torchvision VGG16 state dict and the package's linear-layer file instead.  No weights are shipped."""
import ctypes as C

import torch
from torch import nn

from . import engine, plans
from ._call import stream
from ._lib import lib, check, sf_lpips_model

# (slice, index inside torchvision's vgg16().features, Cin, Cout) of the thirteen convolutions, in order: THE table of state-dict names --
# `net.<slice>.<index>.{weight,bias}` here, `features.<index>.{weight,bias}` in torchvision
CONVS = (('slice1', 0, 3, 64), ('slice1', 2, 64, 64),
         ('slice2', 5, 64, 128), ('slice2', 7, 128, 128),
         ('slice3', 10, 128, 256), ('slice3', 12, 256, 256), ('slice3', 14, 256, 256),
         ('slice4', 17, 256, 512), ('slice4', 19, 512, 512), ('slice4', 21, 512, 512),
         ('slice5', 24, 512, 512), ('slice5', 26, 512, 512), ('slice5', 28, 512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)          # lin0 .. lin4: `lin<N>.model.1.weight` [1,C,1,1]
SHIFT = (-.030, -.088, -.188)                    # `scaling_layer.shift` / `.scale` [1,3,1,1]
SCALE = (.458, .448, .450)
IGNORED_PREFIXES = ('lins.', )                   # newer releases of the package save the linear layers a second time under `lins.N.model.1.weight`
DEFAULT_CHUNK = 32                               # pairs per pass: 2 * 32 images of 128 x 128 hold 0.5 GB of workspace


def conv_key(i):
    s, n, _, _ = CONVS[i]
    return f'net.{s}.{n}'


def lin_key(i):
    return f'lin{i}.model.1.weight'


class _Leaf(nn.Module):
    pass


class LPIPS(nn.Module):
    """lpips.LPIPS(net='vgg'): forward(in0, in1, normalize=False) -> [N,1,1,1], the perceptual distance of every pair of [N,3,H,W] images in
    [-1, 1] (normalize=True: in [0, 1]).  Inputs must be float32 on a HIP device with H, W >= 16; there is no CPU path.

    A fresh module holds SEEDED RANDOM weights: its scores mean nothing until a state dict is loaded (`load_state_dict` with the package's own,
    or `load_vgg_and_linear`).  The arithmetic is split-bf16 on MFMA whatever `sf_set_precision` says (csrc/lpips.hip)."""

    def __init__(self, pretrained=True, net='vgg', version='0.1', lpips=True, spatial=False, pnet_rand=False, pnet_tune=False, use_dropout=True,
                 model_path=None, eval_mode=True, verbose=False, chunk=DEFAULT_CHUNK):
        super().__init__()
        if net not in ('vgg', 'vgg16'):
            raise NotImplementedError(f"LPIPS(net={net!r}): only the VGG16 backbone runs on the HIP library")
        if spatial:
            raise NotImplementedError('LPIPS(spatial=True) is not implemented')
        if not lpips:
            raise NotImplementedError('LPIPS(lpips=False) is not implemented')
        self.chunk = int(chunk)
        g = torch.Generator().manual_seed(0)
        self.scaling_layer = _Leaf()
        self.scaling_layer.register_buffer('shift', torch.tensor(SHIFT)[None, :, None, None])
        self.scaling_layer.register_buffer('scale', torch.tensor(SCALE)[None, :, None, None])
        self.net = _Leaf()
        for s, n, cin, cout in CONVS:
            if not hasattr(self.net, s):
                self.net.add_module(s, _Leaf())
            leaf = _Leaf()
            leaf.weight = nn.Parameter(torch.randn(cout, cin, 3, 3, generator=g) * (2. / (9 * cin)) ** 0.5, requires_grad=False)
            leaf.bias = nn.Parameter(torch.randn(cout, generator=g) * 0.01, requires_grad=False)
            getattr(self.net, s).add_module(str(n), leaf)
        for i, c in enumerate(TAP_CHANNELS):
            lin, leaf = _Leaf(), _Leaf()
            leaf.weight = nn.Parameter(torch.rand(1, c, 1, 1, generator=g) / c, requires_grad=False)
            lin.model = _Leaf()
            lin.model.add_module('1', leaf)
            self.add_module(f'lin{i}', lin)
        if eval_mode:
            self.eval()

    def load_state_dict(self, state_dict, *args, **kwargs):
        kept = {k: v for k, v in state_dict.items() if not k.startswith(IGNORED_PREFIXES)}
        return super().load_state_dict(kept, *args, **kwargs)

    # ---- the plan: packed weights + the C descriptor, rebuilt when a parameter changes --------------------------------------------------------
    def _plan(self):
        return plans.cached(self, 'lpips', plans.signature(self), self._build_plan)

    def _build_plan(self):
        sd = dict(self.named_parameters())
        dev = sd[conv_key(0) + '.weight'].device
        if dev.type != 'cuda':
            raise RuntimeError('slotformer_amd.lpips: the module must live on a HIP device; there is no CPU fallback')
        plan = plans.Plan()
        m = sf_lpips_model()
        st = torch.cuda.current_stream(dev).cuda_stream
        for i, (_, _, cin, cout) in enumerate(CONVS):
            packed = torch.empty(cout * cin * 9 * 4, dtype=torch.uint8, device=dev)
            check(lib().sf_lpips_pack_conv_weights(plan.dp(sd[conv_key(i) + '.weight']), packed.data_ptr(), cout, cin, st))
            plan.keep.append(packed)
            m.conv_w[i] = packed.data_ptr()
            m.conv_b[i] = plan.dp(sd[conv_key(i) + '.bias'])
        for i in range(len(TAP_CHANNELS)):
            m.lin_w[i] = plan.dp(sd[lin_key(i)].reshape(-1))
        m.shift = plan.dp(self.scaling_layer.shift.reshape(-1))
        m.scale = plan.dp(self.scaling_layer.scale.reshape(-1))
        plan.struct = m
        return plan

    @torch.no_grad()
    def distances(self, in0, in1, normalize=False, out=None, chunk=None):
        """in0, in1 [F,3,H,W] device float32 -> [F] float32 (into `out` when given).  The frames go through the network `chunk` pairs at a time;
        the workspace (engine.workspace) holds one chunk.  Asynchronous on torch's current stream."""
        for t in (in0, in1):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
                raise RuntimeError('slotformer_amd.lpips: inputs must be float32 tensors on a HIP device; there is no CPU fallback')
        if in0.shape != in1.shape or in0.dim() != 4 or in0.shape[1] != 3:
            raise ValueError(f'LPIPS: two [N,3,H,W] batches of one shape are required, got {tuple(in0.shape)} and {tuple(in1.shape)}')
        F, _, H, W = in0.shape
        if min(H, W) < 16:
            raise ValueError('LPIPS: H and W must be at least 16 (five stages of VGG16)')
        plan = self._plan()
        dev = in0.device
        if out is None:
            out = torch.empty(F, dtype=torch.float32, device=dev)
        assert out.is_cuda and out.dtype == torch.float32 and out.numel() == F and out.is_contiguous()
        if F == 0:
            return out
        chunk = max(1, min(int(chunk or self.chunk), F))
        need = lib().sf_lpips_workspace_bytes(H, W, chunk)
        if need == 0:
            raise ValueError(f'LPIPS: {H} x {W} frames in chunks of {chunk} are not supported (sf_lpips_workspace_bytes)')
        ws = engine.workspace(dev, need, ('lpips', ))
        x, y = in0.contiguous(), in1.contiguous()
        check(lib().sf_lpips_f32(C.byref(plan.struct), x.data_ptr(), y.data_ptr(), out.data_ptr(), F, H, W, chunk, int(bool(normalize)),
                                 ws.data_ptr(), ws.numel(), stream(x)))
        return out

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        if retPerLayer:
            raise NotImplementedError('LPIPS(retPerLayer=True) is not implemented')
        return self.distances(in0, in1, normalize=normalize).view(-1, 1, 1, 1)


def load_vgg_and_linear(module, vgg_state_dict, linear_state_dict):
    """Fill `module` from a torchvision VGG16 state dict (`features.N.weight` / `.bias`; the classifier is ignored) and the `lpips` package's
    linear-layer file for VGG (`lin0.model.1.weight` .. `lin4.model.1.weight`, [1,C,1,1]; `lins.*` duplicates ignored).  Returns `module`."""
    sd = {}
    for i, (_, n, _, _) in enumerate(CONVS):
        for leaf in ('weight', 'bias'):
            sd[f'{conv_key(i)}.{leaf}'] = vgg_state_dict[f'features.{n}.{leaf}']
    for i in range(len(TAP_CHANNELS)):
        sd[lin_key(i)] = linear_state_dict[lin_key(i)]
    sd['scaling_layer.shift'] = module.scaling_layer.shift
    sd['scaling_layer.scale'] = module.scaling_layer.scale
    module.load_state_dict(sd)
    return module
