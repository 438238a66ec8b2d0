"""Training of the rollout Transformer on the HIP library.

`SlotRollouter.forward` lands here when autograd is recording: the whole autoregressive rollout is ONE autograd node.
Its forward is `sf_rollout_train_fwd_f32` (activations of all steps kept in a workspace owned by the node), its backward
`sf_rollout_train_bwd_f32`, which writes every parameter gradient into one flat fp32 bucket -- the unit the data-parallel
all-reduce works on (parallel.allreduce_flat_bucket's layout, without the pack / unpack copies).  This replaces
torch autograd over the reference's per-step nn.TransformerEncoder calls (slotformer.py:110-124) and nerv's DDP wrap.

Dropout follows nn.TransformerEncoderLayer: active iff the module is in train() mode, p read from the layer.

Data-parallel training: SlotFormer's parameters all belong to ONE node, so `rollouter.ddp_flat_bucket = True` lets that node
all-reduce its bucket inside backward().  StoSAVi's step is a chain of nodes (image encoder, one Slot-Attention node per
frame, predictor layers, decoder) whose gradients autograd accumulates into `.grad`; there the step ends with one
`parallel.allreduce_flat_bucket(model.parameters())` -- still a single RCCL call (4.8 MB).
"""
import ctypes as C

import torch
import torch.nn.functional as tnf

from ._call import ptr, require_device, scratch, stream
from ._lib import sf_savi_features, sf_savi_features_grads, sf_savi_decoder_grads
from ._lib import sf_adam_group
from ._lib import lib, check, sf_rollouter_grads, sf_tfm_layer_grads, sf_slot_attention, sf_slot_attention_grads, _SA_LEAVES
from . import engine, parallel

_LAYER_LEAVES = ('norm1.weight', 'norm1.bias', 'self_attn.in_proj_weight', 'self_attn.in_proj_bias',
                 'self_attn.out_proj.weight', 'self_attn.out_proj.bias', 'norm2.weight', 'norm2.bias', 'linear1.weight',
                 'linear1.bias', 'linear2.weight', 'linear2.bias')
_LAYER_FIELDS = ('norm1_g', 'norm1_b', 'in_proj_w', 'in_proj_b', 'out_proj_w', 'out_proj_b', 'norm2_g', 'norm2_b', 'lin1_w',
                 'lin1_b', 'lin2_w', 'lin2_b')


def _leaf(module, dotted):
    for part in dotted.split('.'):
        module = getattr(module, part)
    return module


def rollouter_parameters(r):
    """The trainable leaves of a SlotRollouter in bucket order: in_proj, out_proj, then every layer's leaves."""
    ps = [r.in_proj.weight, r.in_proj.bias, r.out_proj.weight, r.out_proj.bias]
    for layer in r.transformer_encoder.layers:
        ps += [_leaf(layer, n) for n in _LAYER_LEAVES]
    return ps


def learnable_tables(r):
    """The position tables of a rollouter that are trained (t_pe / slots_pe = 'learnable', slotformer.py:19-29 build_pos_enc)."""
    return [p for p in (getattr(r, 'enc_t_pe', None), getattr(r, 'enc_slots_pe', None)) if isinstance(p, torch.nn.Parameter) and p.requires_grad]


def _grad_descriptor(flat, params, num_layers, pe_off=None):
    """sf_rollouter_grads whose pointers are consecutive slices of `flat` (same order as rollouter_parameters); pe_off: where the
    gradient of the folded position table goes (floats into `flat`), None = tables fixed."""
    ptrs, off = [], 0
    for p in params:
        ptrs.append(flat.data_ptr() + 4 * off)
        off += p.numel()
    g = sf_rollouter_grads()
    g.pe_tok = None if pe_off is None else flat.data_ptr() + 4 * pe_off
    g.in_proj_w, g.in_proj_b, g.out_proj_w, g.out_proj_b = ptrs[:4]
    arr = (sf_tfm_layer_grads * num_layers)()
    for i in range(num_layers):
        for j, f in enumerate(_LAYER_FIELDS):
            setattr(arr[i], f, ptrs[4 + i * len(_LAYER_FIELDS) + j])
    g.layers = C.cast(arr, C.POINTER(sf_tfm_layer_grads))
    return g, arr


def _split(flat, params):
    out, off = [], 0
    for p in params:
        out.append(flat[off:off + p.numel()].view_as(p))
        off += p.numel()
    return out


class _Rollout(torch.autograd.Function):
    """pred = rollouter(x, pred_len) as a single autograd node."""

    @staticmethod
    def forward(ctx, r, x, pred_len, p_drop, seed, *params):
        x = x.detach().float().contiguous()
        require_device(x)
        plan = engine.rollouter_plan(r, packed=False)
        B = x.shape[0]
        ws = scratch(lib().sf_rollout_train_workspace_bytes, C.byref(plan.struct), B, pred_len, device=x.device)
        pred = torch.empty(B, pred_len, *x.shape[2:], dtype=torch.float32, device=x.device)
        check(lib().sf_rollout_train_fwd_f32(C.byref(plan.struct), x.data_ptr(), pred.data_ptr(), B, pred_len, float(p_drop),
                                             int(seed), ws.data_ptr(), ws.numel(), stream()))
        ctx.r, ctx.plan, ctx.ws, ctx.args = r, plan, ws, (B, pred_len, float(p_drop), int(seed), tuple(x.shape))
        ctx.params = params
        return pred

    @staticmethod
    def backward(ctx, d_pred):
        d_x, grads = _rollout_backward(ctx, d_pred, ctx.args[4] if ctx.needs_input_grad[1] else None)
        return (None, d_x, None, None, None) + tuple(g_ if ctx.needs_input_grad[5 + i] else None for i, g_ in enumerate(grads))


def _rollout_backward(ctx, d_pred, xshape=None, grad_out=None):
    """sf_rollout_train_bwd_f32 on the workspace a rollout forward node kept (ctx.r, plan, ws, args, params).  Returns (d_x or None, the
    gradients of ctx.params).  grad_out None: the gradients are views of one fresh flat buffer (`r.last_grad_bucket`).  grad_out: a caller's flat
    fp32 buffer laid out as a FlatAdam bucket over ctx.params (the weights, then the learnable tables) -- the kernels write the weights' gradients
    straight into it, nothing is allocated for them, and the returned gradients are views of it."""
    B, pred_len, p_drop, seed = ctx.args[:4]
    r, plan, params = ctx.r, ctx.plan, ctx.params
    d_pred = d_pred.float().contiguous()
    # the weights' gradients, then (learnable tables only) the gradient of the folded table pe_tok [window tokens, d_model]
    tables = learnable_tables(r)
    params = params[:len(params) - len(tables)]
    nw = sum(p.numel() for p in params)
    W, N, d = plan.struct.window_len, plan.struct.num_slots, plan.struct.d_model
    if grad_out is None:
        flat = torch.empty(nw + (W * N * d if tables else 0), dtype=torch.float32, device=d_pred.device)
        pe = flat[nw:]
    else:
        if grad_out.dtype != torch.float32 or not grad_out.is_contiguous() or grad_out.numel() != nw + sum(p.numel() for p in tables):
            raise ValueError('slotformer_amd: grad_out must be a contiguous float32 bucket over the rollouter parameters and its learnable tables')
        flat = grad_out
        pe = torch.empty(W * N * d, dtype=torch.float32, device=d_pred.device) if tables else None
    g, keep = _grad_descriptor(flat, params, len(r.transformer_encoder.layers), None)
    g.pe_tok = pe.data_ptr() if tables else None
    d_x = torch.empty(xshape, dtype=torch.float32, device=d_pred.device) if xshape is not None else None
    check(lib().sf_rollout_train_bwd_f32(C.byref(plan.struct), d_pred.data_ptr(), ptr(d_x),
                                         C.byref(g), B, pred_len, p_drop, seed, ctx.ws.data_ptr(), ctx.ws.numel(),
                                         stream()))
    del keep
    ctx.ws = None
    if grad_out is None:
        if getattr(r, 'ddp_flat_bucket', False):
            # data-parallel training (config C3): ONE all-reduce of the whole bucket over RCCL / xGMI, averaged
            parallel.allreduce_flat(flat)
        r.last_grad_bucket = flat
    grads = _split(flat, params)
    if tables:
        # pe_tok[t * N + n] = enc_t_pe[t] + enc_slots_pe[n]  (slotformer.py:103-109): sum the folded gradient over slots / frames
        dpe = pe.view(W, N, d)
        off = nw
        for p in tables:
            dim = 1 if p is getattr(r, 'enc_t_pe', None) else 0
            if grad_out is None:
                grads.append(dpe.sum(dim).view_as(p))
            else:
                view = flat[off:off + p.numel()]
                torch.sum(dpe, dim, out=view.view(dpe.shape[1 - dim], d))
                grads.append(view.view_as(p))
                off += p.numel()
    return d_x, grads


def rollout_with_grad(r, x, pred_len):
    """SlotRollouter.forward under autograd (slotformer.py:85-126).  x [B, history_len, N, C] -> [B, pred_len, N, C]."""
    layer0 = r.transformer_encoder.layers[0]
    p_drop = float(layer0.dropout.p) if r.training else 0.0
    seed = int(torch.randint(0, 2**62, (1, )).item()) if p_drop > 0 else 0
    seed = getattr(r, 'dropout_seed_override', None) or seed
    # (learnable position tables ride along as extra leaves: the kernels read them folded into pe_tok, engine.rollouter_plan, and
    # sf_rollout_train_bwd_f32 returns the folded table's gradient)
    return _Rollout.apply(r, x, pred_len, p_drop, seed, *rollouter_parameters(r), *learnable_tables(r))


# ---------------------------------------------------------------------------------------------------------------------
# Training on clips of a device-resident table (video_prediction.fit): csrc/clip_train.hip
# ---------------------------------------------------------------------------------------------------------------------
def burnin_len(r):
    """Frames a rollouter reads before it predicts: history_len, ONE for the single-step rollouter (whose window grows to cond_len)."""
    return 1 if hasattr(r, 'cond_len') else r.history_len


def _index_i32(t, n, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f'slotformer_amd: {name} must live on a HIP device; there is no CPU fallback')
    if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f'slotformer_amd: {name} must be a contiguous int32 [{n}] tensor, got {t.dtype} {tuple(t.shape)}')
    return t


def _check_table(table, tail, name='table'):
    if not (torch.is_tensor(table) and table.is_cuda):
        raise RuntimeError(f'slotformer_amd: the {name} must live on a HIP device; there is no CPU fallback')
    if table.dtype != torch.float32 or table.dim() < 3 or not table.is_contiguous() or (tail is not None and tuple(table.shape[2:]) != tuple(tail)):
        raise ValueError(f'slotformer_amd: the {name} must be a contiguous float32 [V, T{"".join(", %d" % k for k in (tail or ()))}] tensor, got '
                         f'{table.dtype} {tuple(table.shape)}')
    return table


def _clips_forward(r, table, clip_video, clip_start, frame_offset, pred_len, p_drop, seed, ws=None):
    """sf_rollout_train_clips_fwd_f32 -> (pred [B, pred_len, N, C], plan, workspace).  The index tensors are trusted (never read back); what the
    host knows is checked by the library: a clip of burn-in + pred_len frames at this offset must fit the table's T."""
    plan = engine.rollouter_plan(r, packed=False)
    N, Cs = plan.struct.num_slots, plan.struct.slot_size
    _check_table(table, (N, Cs))
    B = clip_video.numel() if torch.is_tensor(clip_video) else 0
    _index_i32(clip_video, B, 'clip_video')
    _index_i32(clip_start, B, 'clip_start')
    ws = scratch(lib().sf_rollout_train_workspace_bytes, C.byref(plan.struct), B, pred_len, device=table.device, reuse=ws)
    pred = torch.empty(B, pred_len, N, Cs, dtype=torch.float32, device=table.device)
    check(lib().sf_rollout_train_clips_fwd_f32(C.byref(plan.struct), table.data_ptr(), table.shape[1], clip_video.data_ptr(), clip_start.data_ptr(),
                                               int(frame_offset), pred.data_ptr(), B, pred_len, float(p_drop), int(seed), ws.data_ptr(), ws.numel(),
                                               stream()))
    return pred, plan, ws


class _RolloutClips(torch.autograd.Function):
    """pred = rollouter(burn-in frames of B clips of a slot table, pred_len) as a single autograd node; the table is data (no gradient)."""

    @staticmethod
    def forward(ctx, r, table, clip_video, clip_start, frame_offset, pred_len, p_drop, seed, grad_out, *params):
        pred, plan, ws = _clips_forward(r, table, clip_video, clip_start, frame_offset, pred_len, p_drop, seed)
        ctx.r, ctx.plan, ctx.ws, ctx.args = r, plan, ws, (pred.shape[0], pred_len, float(p_drop), int(seed))
        ctx.params, ctx.grad_out = params, grad_out
        return pred

    @staticmethod
    def backward(ctx, d_pred):
        _, grads = _rollout_backward(ctx, d_pred, None, ctx.grad_out)
        if ctx.grad_out is not None:   # the caller's bucket holds them: nothing for autograd to accumulate
            grads = [None] * len(grads)
        return (None, ) * 9 + tuple(g_ if (g_ is not None and ctx.needs_input_grad[9 + i]) else None for i, g_ in enumerate(grads))


def rollout_clips_with_grad(r, table, clip_video, clip_start, frame_offset, pred_len, seed=None, grad_out=None):
    """`rollout_with_grad` on clips that stay where they lie: table [V, T, N, C] float32 and int32 [B] clip_video / clip_start on the device; burn-in
    frame j of clip b is table[clip_video[b], clip_start[b] + j * frame_offset] (burnin_len(r) frames).  -> pred [B, pred_len, N, C], bit for bit
    what `rollout_with_grad` returns on a gathered copy.  Dropout as there (active iff r.training, p of the first layer); seed: the dropout seed
    (default: r.dropout_seed_override, else a fresh one from torch's CPU generator).
    grad_out: a flat fp32 buffer laid out as FlatAdam's bucket over rollouter_parameters(r) + learnable_tables(r) (`FlatAdam.grad`): the backward
    writes the gradients there -- then step with `FlatAdam.step(gathered=True)` -- and the parameters' `.grad` are left alone."""
    require_device(table, what='the slot table')
    layer0 = r.transformer_encoder.layers[0]
    p_drop = float(layer0.dropout.p) if r.training else 0.0
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1, )).item()) if p_drop > 0 else 0
        seed = getattr(r, 'dropout_seed_override', None) or seed
    return _RolloutClips.apply(r, table, clip_video, clip_start, int(frame_offset), int(pred_len), p_drop, int(seed), grad_out,
                               *rollouter_parameters(r), *learnable_tables(r))


_CLIP_MSE_WS = {}


def _clip_mse_ws(device, B, S, E):
    """The loss launch's workspace, one per device: zero-filled once; every launch leaves its arrival counter at zero.  Launches that share it must
    be ordered (one stream at a time), as everything in this module is."""
    old = _CLIP_MSE_WS.get(device)
    ws = scratch(lib().sf_clip_mse_workspace_bytes, B, S, E, device=device, reuse=old, at_least=1 << 16)
    if ws is not old:
        _CLIP_MSE_WS[device] = ws.zero_()
    return ws


def clip_mse_launch(pred, target, clip_video, clip_start, frame_offset, hist, step_w, clip_len, scale, d_pred, stats):
    """sf_clip_mse_f32.  pred [B, S, ...] float32.  clip_video None: `target` is dense, of pred's shape.  Otherwise `target` is a table [V, T, ...] and
    step s of clip b is compared with target[clip_video[b], clip_start[b] + (hist + s) * frame_offset].  step_w [S] float32 on the device or None;
    clip_len int32 [B] or None (step s counts iff hist + s < clip_len[b]).  d_pred (pred's shape, or None) receives scale * w_s * 2 * (pred - target) /
    count; stats float64 [1 + 2 S] has the loss, the per-step sums of squares and the per-step counts ADDED to it."""
    if not (torch.is_tensor(pred) and pred.is_cuda and torch.is_tensor(target) and target.is_cuda):
        raise RuntimeError('slotformer_amd: clip_mse needs tensors on a HIP device; there is no CPU fallback')
    B, S = pred.shape[:2]
    E = pred[0, 0].numel()
    if pred.dtype != torch.float32 or not pred.is_contiguous():
        raise ValueError('slotformer_amd: clip_mse takes a contiguous float32 prediction')
    if clip_video is None:
        if clip_start is not None or tuple(target.shape) != tuple(pred.shape) or target.dtype != torch.float32 or not target.is_contiguous():
            raise ValueError(f'slotformer_amd: a dense target is contiguous float32 of the shape of pred {tuple(pred.shape)}, got {tuple(target.shape)}')
        T_total, first, fstep = S, 0, 1
    else:
        _check_table(target, tuple(pred.shape[2:]), 'target table')
        _index_i32(clip_video, B, 'clip_video')
        _index_i32(clip_start, B, 'clip_start')
        T_total, first, fstep = target.shape[1], int(hist) * int(frame_offset), int(frame_offset)
    if step_w is not None and (step_w.dtype != torch.float32 or step_w.numel() != S or not step_w.is_cuda or not step_w.is_contiguous()):
        raise ValueError(f'slotformer_amd: step_w is a contiguous float32 [{S}] device tensor')
    if clip_len is not None:
        _index_i32(clip_len, B, 'clip_len')
    if stats.dtype != torch.float64 or stats.numel() != 1 + 2 * S or not stats.is_contiguous():
        raise ValueError(f'slotformer_amd: stats is a contiguous float64 [{1 + 2 * S}] device tensor')
    if lib().sf_clip_mse_workspace_bytes(B, S, E) == 0:
        raise NotImplementedError(f'slotformer_amd: clip_mse takes 1 to 64 steps and rows of a multiple of 4 elements, got S {S}, E {E}')
    ws = _clip_mse_ws(pred.device, B, S, E)
    check(lib().sf_clip_mse_f32(pred.data_ptr(), target.data_ptr(), ptr(clip_video), ptr(clip_start), T_total, first, fstep, ptr(step_w),
                                ptr(clip_len), int(hist), float(scale), ptr(d_pred), stats.data_ptr(), B, S, E, ws.data_ptr(), ws.numel(), stream()))


class _ClipMse(torch.autograd.Function):
    """(loss, stats) of sf_clip_mse_f32; the gradient w.r.t. pred was written by the forward launch."""

    @staticmethod
    def forward(ctx, pred, target, clip_video, clip_start, frame_offset, hist, step_w, clip_len, scale):
        pred = pred.detach().float().contiguous()
        S = pred.shape[1]
        d_pred = torch.empty_like(pred)
        stats = torch.zeros(1 + 2 * S, dtype=torch.float64, device=pred.device)
        clip_mse_launch(pred, target, clip_video, clip_start, frame_offset, hist, step_w, clip_len, scale, d_pred, stats)
        ctx.save_for_backward(d_pred)
        ctx.mark_non_differentiable(stats)
        return stats[0].float(), stats

    @staticmethod
    def backward(ctx, d_loss, _d_stats):
        d_pred, = ctx.saved_tensors
        return (d_pred * d_loss, ) + (None, ) * 8


def clip_mse(pred, target, clip_video=None, clip_start=None, frame_offset=1, hist=0, step_w=None, clip_len=None, scale=1.):
    """The rollout loss of slotformer.py:289-318 under autograd, one launch (see `clip_mse_launch` for the operands): -> (loss, stats).
    loss = scale * sum_s w_s * sum (pred - target)^2 / count over the counted steps, a float32 scalar; stats float64 [1 + 2 S] = (loss, the
    UNWEIGHTED per-step sums of squares, the per-step counts), not differentiable: stats[1 + k] / stats[1 + S + k] is `slot_recon_loss_{k+1}`."""
    return _ClipMse.apply(pred, target, clip_video, clip_start, int(frame_offset), int(hist), step_w, clip_len, float(scale))


def clip_frames(frames, clip_video, clip_start, frame_offset, hist, S, mean=0.5, std=0.5):
    """sf_clip_frames_f32: the S target frames of every clip from a uint8 table [V, T, H, W, 3] (already at the model's resolution) ->
    float32 [B, S, 3, H, W] = (x / 255 - mean) / std, the bits `FrameIngest` gives at equal source and output size.  mean / std: a float or three."""
    require_device(frames, what='the frame table')
    if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError(f'slotformer_amd: the frame table is a contiguous uint8 [V, T, H, W, 3] tensor, got {frames.dtype} {tuple(frames.shape)}')
    B = clip_video.numel() if torch.is_tensor(clip_video) else 0
    _index_i32(clip_video, B, 'clip_video')
    _index_i32(clip_start, B, 'clip_start')
    three = lambda v: (C.c_float * 3)(*([float(v)] * 3 if not hasattr(v, '__len__') else [float(x) for x in v]))  # noqa: E731
    H, W = frames.shape[2:4]
    out = torch.empty(B, int(S), 3, H, W, dtype=torch.float32, device=frames.device)
    check(lib().sf_clip_frames_f32(frames.data_ptr(), frames.shape[1], clip_video.data_ptr(), clip_start.data_ptr(), int(hist) * int(frame_offset),
                                   int(frame_offset), three(mean), three(std), out.data_ptr(), B, int(S), H, W,
                                   stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Slot Attention (savi.py:36-102) under autograd
# ---------------------------------------------------------------------------------------------------------------------
def slot_attention_parameters(sa):
    """Leaves of a SlotAttention container in the order of sf_slot_attention's pointer fields."""
    return [sa.norm_inputs.weight, sa.norm_inputs.bias, sa.project_k.weight, sa.project_v.weight, sa.project_q[0].weight,
            sa.project_q[0].bias, sa.project_q[1].weight, sa.gru.weight_ih, sa.gru.weight_hh, sa.gru.bias_ih, sa.gru.bias_hh,
            sa.mlp[0].weight, sa.mlp[0].bias, sa.mlp[1].weight, sa.mlp[1].bias, sa.mlp[3].weight, sa.mlp[3].bias]


class _SlotAttention(torch.autograd.Function):
    """slots_out = SlotAttention(inputs, slots) as a single autograd node."""

    @staticmethod
    def forward(ctx, sa, inputs, slots, *params):
        inputs, slots = inputs.detach().float().contiguous(), slots.detach().float().contiguous()
        require_device(inputs)
        keep = [p.detach().float().contiguous() for p in params]
        m = sf_slot_attention()
        m.in_features, m.slot_size, m.mlp_hidden, m.num_slots = sa.in_features, sa.slot_size, sa.mlp_hidden_size, slots.shape[1]
        m.eps = float(sa.eps)
        for name, t in zip(_SA_LEAVES, keep):
            setattr(m, name, t.data_ptr())
        B, HW = inputs.shape[:2]
        ws = scratch(lib().sf_slot_attention_train_workspace_bytes, C.byref(m), B, HW, sa.num_iterations, device=inputs.device)
        out = torch.empty_like(slots)
        check(lib().sf_slot_attention_train_fwd_f32(C.byref(m), inputs.data_ptr(), slots.data_ptr(), B, HW, sa.num_iterations,
                                                    out.data_ptr(), ws.data_ptr(), ws.numel(), stream()))
        ctx.sa, ctx.m, ctx.keep, ctx.ws, ctx.inputs, ctx.params = sa, m, keep, ws, inputs, params
        return out

    @staticmethod
    def backward(ctx, d_out):
        sa, m, params, inputs = ctx.sa, ctx.m, ctx.params, ctx.inputs
        d_out = d_out.float().contiguous()
        B, HW = inputs.shape[:2]
        flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=d_out.device)
        g, off = sf_slot_attention_grads(), 0
        for name, p in zip(_SA_LEAVES, params):
            setattr(g, name, flat.data_ptr() + 4 * off)
            off += p.numel()
        d_in = torch.empty_like(inputs) if ctx.needs_input_grad[1] else None
        d_slots = torch.empty_like(d_out)
        check(lib().sf_slot_attention_train_bwd_f32(C.byref(m), inputs.data_ptr(), d_out.data_ptr(),
                                                    ptr(d_in), d_slots.data_ptr(), C.byref(g), B, HW,
                                                    sa.num_iterations, ctx.ws.data_ptr(), ctx.ws.numel(),
                                                    stream()))
        ctx.ws = None
        grads = _split(flat, params)
        return (None, d_in, d_slots if ctx.needs_input_grad[2] else None) + tuple(
            g_ if ctx.needs_input_grad[3 + i] else None for i, g_ in enumerate(grads))


def slot_attention_with_grad(sa, inputs, slots):
    """SlotAttention.forward under autograd (savi.py:56-102): inputs [B,HW,C], slots [B,N,D] -> slots [B,N,D]."""
    return _SlotAttention.apply(sa, inputs, slots, *slot_attention_parameters(sa))


# ---------------------------------------------------------------------------------------------------------------------
# SAVi decoder under autograd (data gradient only: the image term of SlotFormer's loss; the decoder is frozen there)
# ---------------------------------------------------------------------------------------------------------------------
def decoder_parameters(m):
    """Leaves of the spatial-broadcast decoder in bucket order: (weight, bias) per transposed conv, the 1x1 head, the
    position-embedding Linear."""
    n = len(m.dec_channels) - 1
    ps = []
    for i in range(n):
        ps += [m.decoder[i][0].weight, m.decoder[i][0].bias]
    return ps + [m.decoder[n].weight, m.decoder[n].bias, m.decoder_pos_embedding.dense.weight, m.decoder_pos_embedding.dense.bias]


class _Decode(torch.autograd.Function):
    """(recon_combined, recons, masks) = decode(slots); only recon_combined carries a gradient (savi.py:527-538,
    slotformer.py:313-326).  Parameter gradients are produced iff the decoder is not frozen."""

    @staticmethod
    def forward(ctx, m, slots, *params):
        from . import ops
        slots = slots.detach().float().contiguous()
        require_device(slots)
        plan = engine.decoder_plan(m, inference=False)
        if not hasattr(plan, 'bwd_w'):
            n = plan.struct.dec_layers
            plan.bwd_keep = [ops.pack_conv_weight(m.decoder[i][0].weight.detach().float().contiguous()) for i in range(n)]
            plan.bwd_w = (C.c_void_p * n)(*[t.data_ptr() for t in plan.bwd_keep])
        F_, N, D = slots.shape
        H = plan.struct.resolution
        ws = scratch(lib().sf_savi_decode_train_workspace_bytes, C.byref(plan.struct), F_, device=slots.device)
        recon = torch.empty(F_, 3, H, H, device=slots.device, dtype=torch.float32)
        recons = torch.empty(F_, N, 3, H, H, device=slots.device, dtype=torch.float32)
        masks = torch.empty(F_, N, 1, H, H, device=slots.device, dtype=torch.float32)
        check(lib().sf_savi_decode_train_fwd_f32(C.byref(plan.struct), slots.data_ptr(), recon.data_ptr(), recons.data_ptr(),
                                                 masks.data_ptr(), F_, ws.data_ptr(), ws.numel(), stream()))
        ctx.m, ctx.plan, ctx.ws, ctx.shape, ctx.params = m, plan, ws, (F_, N, D), params
        ctx.mark_non_differentiable(recons, masks)
        return recon, recons, masks

    @staticmethod
    def backward(ctx, d_recon, _d_recons, _d_masks):
        F_, N, D = ctx.shape
        params, m = ctx.params, ctx.m
        d_recon = d_recon.float().contiguous()
        d_slots = torch.empty(F_, N, D, device=d_recon.device, dtype=torch.float32)
        g, grid, flat = None, None, None
        if params:
            flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=d_recon.device)
            ptrs, off = [], 0
            for p in params:
                ptrs.append(flat.data_ptr() + 4 * off)
                off += p.numel()
            g = sf_savi_decoder_grads()
            n = ctx.plan.struct.dec_layers
            for i in range(n):
                g.deconv_w[i], g.deconv_b[i] = ptrs[2 * i], ptrs[2 * i + 1]
            g.out_w, g.out_b, g.pos_w, g.pos_b = ptrs[2 * n:2 * n + 4]
            grid = m.decoder_pos_embedding.grid.detach().float().reshape(-1, 4).contiguous()
        check(lib().sf_savi_decode_train_bwd_f32(C.byref(ctx.plan.struct), ctx.plan.bwd_w, d_recon.data_ptr(), d_slots.data_ptr(),
                                                 ptr(grid), C.byref(g) if g is not None else None,
                                                 F_, ctx.ws.data_ptr(), ctx.ws.numel(), stream()))
        ctx.ws = None
        grads = ()
        if params:
            grads = tuple(g_ if ctx.needs_input_grad[2 + i] else None for i, g_ in enumerate(_split(flat, params)))
        return (None, d_slots if ctx.needs_input_grad[1] else None) + grads


def decode_with_grad(m, slots):
    """StoSAVi.decode (savi.py:504-525) under autograd: d(recon_combined)/d(slots), plus the decoder's own parameter
    gradients unless it is frozen (as in SlotFormer, slotformer.py:203-210)."""
    params = decoder_parameters(m)
    if not any(p.requires_grad for p in params):
        params = []
    return _Decode.apply(m, slots, *params)


# ---------------------------------------------------------------------------------------------------------------------
# SAVi image encoder (conv stack + position embedding + per-pixel MLP, savi.py:220-250,367-377) under autograd
# ---------------------------------------------------------------------------------------------------------------------
def features_parameters(m):
    """Leaves of a StoSAVi / STEVE container that the encoder node differentiates, in bucket order."""
    ps = []
    for i in range(len(m.enc_channels) - 1):
        ps += [m.encoder[i][0].weight, m.encoder[i][0].bias]
    pe, eo = m.encoder_pos_embedding, m.encoder_out_layer
    return ps + [pe.dense.weight, pe.dense.bias, eo[0].weight, eo[0].bias, eo[1].weight, eo[1].bias, eo[3].weight, eo[3].bias]


class _Features(torch.autograd.Function):
    """encoder_out [F, 64*64, C_out] = encoder_out_layer(flatten(encoder(img) + pos)) as one node (no image gradient)."""

    @staticmethod
    def forward(ctx, m, img, *params):
        img = img.detach().float().contiguous()
        require_device(img)
        keep = [p.detach().float().contiguous() for p in params]
        n = len(m.enc_channels) - 1
        s = sf_savi_features()
        s.resolution, s.layers, s.channels, s.ks = m.resolution[0], n, m.enc_channels[1], m.enc_ks
        s.hidden, s.out_channels = m.encoder_out_layer[1].out_features, m.encoder_out_layer[3].out_features
        if any(c != s.channels for c in m.enc_channels[1:]):
            raise NotImplementedError('slotformer_amd: encoder training needs equal conv widths (the reference uses 64 everywhere)')
        for i in range(n):
            s.conv_w[i], s.conv_b[i] = keep[2 * i].data_ptr(), keep[2 * i + 1].data_ptr()
        grid = m.encoder_pos_embedding.grid.detach().float().reshape(-1, 4).contiguous()
        keep.append(grid)
        s.pos_grid = grid.data_ptr()
        for name, t in zip(('pos_w', 'pos_b', 'ln_g', 'ln_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b'), keep[2 * n:2 * n + 8]):
            setattr(s, name, t.data_ptr())
        F_ = img.shape[0]
        ws = scratch(lib().sf_savi_features_train_workspace_bytes, C.byref(s), F_, device=img.device)
        out = torch.empty(F_, 64 * 64, s.out_channels, dtype=torch.float32, device=img.device)
        check(lib().sf_savi_features_train_fwd_f32(C.byref(s), img.data_ptr(), img[0].numel(), F_, out.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), stream()))
        ctx.m, ctx.s, ctx.keep, ctx.ws, ctx.img, ctx.params = m, s, keep, ws, img, params
        return out

    @staticmethod
    def backward(ctx, d_out):
        s, params, img = ctx.s, ctx.params, ctx.img
        d_out = d_out.float().contiguous()
        flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=d_out.device)
        ptrs, off = [], 0
        for p in params:
            ptrs.append(flat.data_ptr() + 4 * off)
            off += p.numel()
        g = sf_savi_features_grads()
        n = s.layers
        for i in range(n):
            g.conv_w[i], g.conv_b[i] = ptrs[2 * i], ptrs[2 * i + 1]
        for name, at in zip(('pos_w', 'pos_b', 'ln_g', 'ln_b', 'fc1_w', 'fc1_b', 'fc2_w', 'fc2_b'), ptrs[2 * n:]):
            setattr(g, name, at)
        check(lib().sf_savi_features_train_bwd_f32(C.byref(s), img.data_ptr(), img[0].numel(), d_out.data_ptr(), C.byref(g), img.shape[0],
                                                   ctx.ws.data_ptr(), ctx.ws.numel(), stream()))
        ctx.ws = None
        grads = _split(flat, params)
        return (None, None) + tuple(g_ if ctx.needs_input_grad[2 + i] else None for i, g_ in enumerate(grads))


def features_with_grad(m, img):
    """img [F, 3, H, W] -> encoder_out [F, 64*64, enc_out_channels] under autograd (savi.py:367-377)."""
    return _Features.apply(m, img, *features_parameters(m))


# ---------------------------------------------------------------------------------------------------------------------
# differentiable nn.Linear / nn.LayerNorm on the HIP library, for the slot-level layers (predictor, kernel distribution)
# ---------------------------------------------------------------------------------------------------------------------
class _Linear(torch.autograd.Function):
    """y = act(x W^T + b) with sf_linear_f32 / sf_linear_bwd_f32."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        from . import ops
        xd, wd = x.detach().float().contiguous(), weight.detach().float().contiguous()
        y = ops.linear(xd, wd, bias.detach().float().contiguous() if bias is not None else None, relu=relu)
        ctx.save_for_backward(xd, wd, y if relu else None)
        ctx.relu, ctx.has_bias = bool(relu), bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = dy.float().contiguous().clone() if ctx.relu else dy.float().contiguous()
        N, K = w.shape
        M = x.numel() // K
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        db = torch.empty(N, dtype=torch.float32, device=w.device) if ctx.has_bias else None
        ws = scratch(lib().sf_linear_bwd_workspace_bytes, M, N, K, device=w.device)
        check(lib().sf_linear_bwd_f32(ptr(x), ptr(w), ptr(y), ptr(dy), ptr(dx), ptr(dw), ptr(db), M, N, K, int(ctx.relu), ws.data_ptr(), ws.numel(),
                                      stream()))
        return dx, dw, db, None


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        from . import ops
        xd, g = x.detach().float().contiguous(), gamma.detach().float().contiguous()
        ctx.save_for_backward(xd, g)
        ctx.eps = float(eps)
        return ops.layernorm(xd, g, beta.detach().float().contiguous(), eps)

    @staticmethod
    def backward(ctx, dy):
        x, g = ctx.saved_tensors
        dy = dy.float().contiguous()
        D = x.shape[-1]
        dx, dg, db = torch.empty_like(x), torch.empty_like(g), torch.empty_like(g)
        ws = scratch(lib().sf_layernorm_bwd_workspace_bytes, D, device=x.device)
        check(lib().sf_layernorm_bwd_f32(x.data_ptr(), dy.data_ptr(), g.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                         x.numel() // D, D, ctx.eps, ws.data_ptr(), ws.numel(), stream()))
        return dx, dg, db, None


class _MHA(torch.autograd.Function):
    """Attention core of nn.MultiheadAttention (batch_first self-attention) on packed q|k|v rows."""

    @staticmethod
    def forward(ctx, qkv, B, L, d, heads, p, seed):
        qkv = qkv.detach().float().contiguous()
        out = torch.empty(B * L, d, dtype=torch.float32, device=qkv.device)
        check(lib().sf_mha_train_fwd_f32(qkv.data_ptr(), out.data_ptr(), B, L, d, heads, float(p), int(seed),
                                         stream()))
        ctx.save_for_backward(qkv)
        ctx.args = (B, L, d, heads, float(p), int(seed))
        return out

    @staticmethod
    def backward(ctx, d_out):
        qkv, = ctx.saved_tensors
        B, L, d, heads, p, seed = ctx.args
        d_out = d_out.float().contiguous()
        dqkv = torch.empty_like(qkv)
        check(lib().sf_mha_train_bwd_f32(qkv.data_ptr(), d_out.data_ptr(), dqkv.data_ptr(), B, L, d, heads, p, seed,
                                         stream()))
        return dqkv, None, None, None, None, None, None


class _Dropout(torch.autograd.Function):
    """nn.Dropout in train mode with the library's hashed masks (regenerated in the backward pass)."""

    @staticmethod
    def forward(ctx, x, p, seed):
        x = x.detach().float().contiguous()
        y = torch.empty_like(x)
        check(lib().sf_dropout_f32(x.data_ptr(), None, y.data_ptr(), x.numel(), float(p), int(seed), stream()))
        ctx.args = (float(p), int(seed))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.float().contiguous()
        dx = torch.empty_like(dy)
        check(lib().sf_dropout_f32(dy.data_ptr(), None, dx.data_ptr(), dy.numel(), ctx.args[0], ctx.args[1], stream()))
        return dx, None, None


def _new_seed():
    return int(torch.randint(0, 2**62, (1, )).item())


def dropout(x, p, training):
    return _Dropout.apply(x, p, _new_seed()) if (training and p > 0) else x


def transformer_encoder_layer(x, layer):
    """nn.TransformerEncoderLayer (pre-LN, relu, batch_first; predictor.py:33-38) on x [B, L, d] as a chain of HIP-backed
    autograd nodes, dropout included when the layer is in train() mode."""
    if not layer.norm_first:
        raise NotImplementedError('slotformer_amd: training needs norm_first Transformer layers (all reference configurations)')
    B, L, d = x.shape
    tr, att = layer.training, layer.self_attn
    h = layer_norm(x, layer.norm1)
    qkv = _Linear.apply(h, att.in_proj_weight, att.in_proj_bias, False)
    p_att = float(att.dropout) if tr else 0.0
    ctx = _MHA.apply(qkv.reshape(B * L, 3 * d), B, L, d, att.num_heads, p_att, _new_seed() if p_att > 0 else 0).view(B, L, d)
    x = x + dropout(linear(ctx, att.out_proj), layer.dropout1.p, tr)
    h = layer_norm(x, layer.norm2)
    h = dropout(linear(h, layer.linear1, relu=True), layer.dropout.p, tr)
    return x + dropout(linear(h, layer.linear2), layer.dropout2.p, tr)


def lstm_step(x, state, rnn):
    """One step of a 1-layer nn.LSTM on x [R, C] with state (h, c) [R, H] or None (predictor.py:116-117); the two gate
    projections are HIP-backed nodes, the gate nonlinearities are elementwise glue."""
    R = x.shape[0]
    H = rnn.hidden_size
    if state is None:
        h = torch.zeros(R, H, dtype=torch.float32, device=x.device)
        c = torch.zeros_like(h)
    else:
        h, c = state
    gates = _Linear.apply(x, rnn.weight_ih_l0, rnn.bias_ih_l0, False) + _Linear.apply(h, rnn.weight_hh_l0, rnn.bias_hh_l0, False)
    i, f, g, o = gates.chunk(4, -1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    return h2, (h2, c2)


class _SlateAttention(torch.autograd.Function):
    """softmax(q k^T / sqrt(hd) [causal]) v of the STEVE decoder (steve_transformer.py:12-55) on contiguous q [B,Lq,d],
    k, v [B,Lk,d], with optional dropout on the attention weights (p > 0: the training forward, which also keeps the row
    log-sum-exp; p == 0: the inference kernel).  Backward: the flash-style sf_slate_attention_train_bwd_f32."""

    @staticmethod
    def forward(ctx, q, k, v, heads, causal, p, seed):
        from . import ops
        q, k, v = (t.detach().float().contiguous() for t in (q, k, v))
        B, Lq, d = q.shape
        Lk = k.shape[1]
        lse = None
        if p > 0:
            out = torch.empty_like(q)
            lse = torch.empty(B, heads, Lq, dtype=torch.float32, device=q.device)
            check(lib().sf_slate_attention_train_fwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), d, d, d, d,
                                                         Lq * d, Lk * d, Lk * d, Lq * d, B, Lq, Lk, heads, d // heads, int(causal), float(p),
                                                         int(seed), stream()))
        else:
            out = ops.slate_attention(q, k, v, heads, causal)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.args = (heads, bool(causal), float(p), int(seed))
        return out

    @staticmethod
    def backward(ctx, d_out):
        q, k, v, out, lse = ctx.saved_tensors
        heads, causal, p, seed = ctx.args
        B, Lq, d = q.shape
        Lk = k.shape[1]
        d_out = d_out.float().contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ws = scratch(lib().sf_slate_attention_bwd_workspace_bytes, B, Lq, heads, device=q.device)
        check(lib().sf_slate_attention_train_bwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), d_out.data_ptr(), ptr(lse),
                                                     dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), d, d, d, d, Lq * d, Lk * d, Lk * d, Lq * d,
                                                     B, Lq, Lk, heads, d // heads, int(causal), p, seed, ws.data_ptr(), ws.numel(), stream()))
        return dq, dk, dv, None, None, None, None


class _SelfAttention(torch.autograd.Function):
    """Self-attention of a STEVE decoder block from its input: q|k|v = x [Wq;Wk;Wv]^T in ONE GEMM into a packed [B,L,3d]
    buffer that the attention kernels read in place (column offsets 0, d, 2d), and whose gradient the attention backward
    writes in place -- no per-projection GEMMs, no copies of q, k, v or of their gradients."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, heads, causal, p, seed):
        from . import ops
        x = x.detach().float().contiguous()
        B, L, d = x.shape
        wcat = torch.cat([w.detach().float() for w in (wq, wk, wv)], 0).contiguous()
        qkv = ops.linear(x, wcat)                                   # [B, L, 3d]
        lse = None
        if p > 0:
            out = torch.empty(B, L, d, dtype=torch.float32, device=x.device)
            lse = torch.empty(B, heads, L, dtype=torch.float32, device=x.device)
            base = qkv.data_ptr()
            check(lib().sf_slate_attention_train_fwd_f32(base, base + 4 * d, base + 8 * d, out.data_ptr(), lse.data_ptr(), 3 * d, 3 * d,
                                                         3 * d, d, L * 3 * d, L * 3 * d, L * 3 * d, L * d, B, L, L, heads, d // heads,
                                                         int(causal), float(p), int(seed), stream()))
        else:
            out = ops.slate_attention(qkv, qkv, qkv, heads, causal, 0, d, 2 * d, d_model=d)
        ctx.save_for_backward(x, wcat, qkv, out, lse)
        ctx.args = (heads, bool(causal), float(p), int(seed))
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, wcat, qkv, out, lse = ctx.saved_tensors
        heads, causal, p, seed = ctx.args
        B, L, d = x.shape
        d_out = d_out.float().contiguous()
        dqkv = torch.empty_like(qkv)
        st = stream()
        ws = scratch(lib().sf_slate_attention_bwd_workspace_bytes, B, L, heads, device=x.device)
        b0, g0 = qkv.data_ptr(), dqkv.data_ptr()
        check(lib().sf_slate_attention_train_bwd_f32(b0, b0 + 4 * d, b0 + 8 * d, out.data_ptr(), d_out.data_ptr(), ptr(lse), g0, g0 + 4 * d,
                                                     g0 + 8 * d, 3 * d, 3 * d, 3 * d, d, L * 3 * d, L * 3 * d, L * 3 * d, L * d, B, L, L, heads,
                                                     d // heads, int(causal), p, seed, ws.data_ptr(), ws.numel(), st))
        dx = torch.empty_like(x)
        dw = torch.empty_like(wcat)
        M = B * L
        ws = scratch(lib().sf_linear_bwd_workspace_bytes, M, 3 * d, d, device=x.device)
        check(lib().sf_linear_bwd_f32(x.data_ptr(), wcat.data_ptr(), None, dqkv.data_ptr(), dx.data_ptr(), dw.data_ptr(), None, M, 3 * d, d,
                                      0, ws.data_ptr(), ws.numel(), st))
        return (dx, ) + tuple(dw.split(d, 0)) + (None, None, None, None)


class _Embed(torch.autograd.Function):
    """tok_emb[idx] + pos[:L] (steve_transformer.py:58-74,286-289): HIP gather forward; the backward scatters the row
    gradients back (index_add on the [V+1, d] table, batch sum for the position table)."""

    @staticmethod
    def forward(ctx, idx, tok_emb, pos):
        from . import ops
        ctx.save_for_backward(idx)
        ctx.shapes = (tuple(tok_emb.shape), tuple(pos.shape))
        return ops.embed_tokens(idx, tok_emb.detach().float().contiguous(), pos.detach().float().contiguous())

    @staticmethod
    def backward(ctx, dx):
        idx, = ctx.saved_tensors
        (V, d), pshape = ctx.shapes
        dx = dx.float().contiguous()
        d_tok = torch.zeros(V, d, dtype=torch.float32, device=dx.device).index_add_(0, idx.reshape(-1), dx.reshape(-1, d))
        d_pos = torch.zeros(pshape, dtype=torch.float32, device=dx.device)
        d_pos[:dx.shape[1]] = dx.sum(0)
        return None, d_tok, d_pos


class _TokenCrossEntropy(torch.autograd.Function):
    """mean cross-entropy of logits [R,V] against int64 targets [R] (steve.py:341-344): sf_cross_entropy_f32 forward,
    (softmax - onehot) / R backward on sf_softmax_rows_f32."""

    @staticmethod
    def forward(ctx, logits, target):
        from . import ops
        logits = logits.detach().float().contiguous()
        ctx.save_for_backward(logits, target)
        return ops.cross_entropy(logits, target)

    @staticmethod
    def backward(ctx, g):
        from . import ops
        logits, target = ctx.saved_tensors
        R, V = logits.shape
        if V > 16384:
            p = ops.softmax_rows(logits)
            p.scatter_add_(1, target.view(-1, 1), torch.full((target.numel(), 1), -1.0, device=p.device))
            return p * (g / R), None
        dx = torch.empty_like(logits)
        gs = g.detach().float().reshape(1).contiguous()
        check(lib().sf_cross_entropy_bwd_f32(logits.data_ptr(), target.data_ptr(), gs.data_ptr(), dx.data_ptr(), R, V,
                                             stream()))
        return dx, None


def slate_decoder_forward(dec, slots, idx):
    """STEVETransformerDecoder.forward (steve_transformer.py:275-303) under autograd: slots [B,N,d], idx int64 [B,t] ->
    logits [B,1+t,V], as a chain of HIP-backed nodes; every dropout of the reference modules (embedding, attention weights,
    attention output, FFN) is active iff the decoder is in train() mode."""
    return linear(slate_decoder_hidden(dec, slots, idx), dec.head)


def slate_decoder_hidden(dec, slots, idx):
    """`slate_decoder_forward` up to and including the final LayerNorm -> [B,1+t,d]: the rows the vocabulary head is applied to, for
    `head_cross_entropy`, which takes them to the token loss without the logits."""
    tr = dec.training
    B, T = idx.shape
    H = dec.n_head

    def attend(q, k, v, mha, causal):
        p = float(mha.attn_dropout.p) if tr else 0.0
        return _SlateAttention.apply(q, k, v, H, causal, p, _new_seed() if p > 0 else 0)
    mem = linear(slots.float().contiguous(), dec.in_proj)
    bos = torch.full((B, 1), dec.vocab_size, dtype=torch.int64, device=idx.device)
    tokens = torch.cat([bos, idx.to(torch.int64)], 1).contiguous()
    x = dropout(_Embed.apply(tokens, dec.tok_emb.weight, dec.pos_emb.pe[0]), dec.pos_emb.dropout.p, tr)
    for blk in dec.tf_dec.blocks:
        sa, ca = blk.self_attn, blk.encoder_decoder_attn
        y = layer_norm(x, blk.self_attn_layer_norm)
        if blk.is_first:   # the first block normalises its input in place (steve_transformer.py:186-190)
            x = y
        p_sa = float(sa.attn_dropout.p) if tr else 0.0
        att = _SelfAttention.apply(y, sa.proj_q.weight, sa.proj_k.weight, sa.proj_v.weight, H, True, p_sa, _new_seed() if p_sa > 0 else 0)
        x = x + dropout(linear(att, sa.proj_o), sa.output_dropout.p, tr)
        y = layer_norm(x, blk.encoder_decoder_attn_layer_norm)
        att = attend(linear(y, ca.proj_q), *linear_cat(mem, ca.proj_k, ca.proj_v), ca, False)
        x = x + dropout(linear(att, ca.proj_o), ca.output_dropout.p, tr)
        y = layer_norm(x, blk.ffn_layer_norm)
        x = x + dropout(linear(linear(y, blk.ffn[0], relu=True), blk.ffn[2]), blk.ffn[3].p, tr)
    return layer_norm(x, dec.tf_dec.layer_norm)


def token_cross_entropy(logits, target):
    return _TokenCrossEntropy.apply(logits, target.to(torch.int64).contiguous())


class _HeadCrossEntropy(torch.autograd.Function):
    """(weighted mean loss, stats) of sf_head_ce_fwd_f32 / sf_head_ce_bwd_f32: the head's product and the cross-entropy in one pass each way.
    Saved for the backward: x, lse [R] and the targets -- nothing of R * V elements exists at any time.  `weight` is the head's [V, K] parameter
    when it is trained (its gradient: one sf_head_ce_wgrad_f32 call) and None for a frozen head; the products read `w_packed` either way."""

    @staticmethod
    def forward(ctx, x, weight, w_packed, target, group_w, group, V):
        from . import ops
        K = x.shape[-1]
        xd = x.detach().float().reshape(-1, K)
        if xd.stride(1) != 1 or xd.stride(0) < K or xd.stride(0) % 4 or xd.data_ptr() % 16:
            xd = xd.contiguous()
        stats = torch.zeros(2, dtype=torch.float64, device=xd.device)
        lse, _ = ops.head_ce_forward(xd, w_packed, target, V, group_w, group, stats, want_rows=False)
        ctx.save_for_backward(xd, w_packed, target, group_w, lse, stats)
        ctx.group, ctx.V, ctx.xshape = group, V, tuple(x.shape)
        ctx.mark_non_differentiable(stats)
        n = stats[1]
        return torch.where(n > 0, stats[0] / n, torch.zeros_like(n)).float(), stats

    @staticmethod
    def backward(ctx, g, _d_stats):
        from . import ops
        xd, w_packed, target, group_w, lse, stats = ctx.saved_tensors
        n = stats[1]
        gd = torch.where(n > 0, g.double() / n, torch.zeros_like(n)).float().reshape(1)   # stays on the device
        dx = ops.head_ce_backward(xd, w_packed, target, ctx.V, lse, gd, group_w, ctx.group).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        dw = ops.head_ce_wgrad(xd, w_packed, target, ctx.V, lse, gd, group_w, ctx.group) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None, None, None, None


def head_cross_entropy(x, weight, target, group_w=None, group=1, weight_grad=False):
    """The token loss of a vocabulary head without its logits: x [..., K] (the rows behind the decoder's final LayerNorm,
    `slate_decoder_hidden`), weight = the head, an nn.Linear without bias or its [V, K] weight, target int64 / int16 ids of x's leading shape ->
    (loss, stats).  loss: the mean over the rows of logsumexp(W x[r]) - W[target[r]] . x[r], weighted by group_w [R / group] float32 (the weight of
    each run of `group` consecutive rows -- a frame's tokens; 0 drops the frame), a float32 device scalar; stats float64 [2] = (sum w loss, sum w),
    not differentiable.  By default the gradient reaches x only and a head that requires grad is refused.  weight_grad=True takes such a head: the
    backward then also returns its gradient [V, K] float32 (`ops.head_ce_wgrad`, again without the logits; its workspace is at most eight [V, K]
    blocks), and skips dx when x needs none; with a frozen head the keyword changes nothing.  The packed copy of the weight is cached on its owner
    and rebuilt when the weight's version changes -- after every optimiser step of a trained head."""
    from . import ops, plans
    w = weight.weight if isinstance(weight, torch.nn.Module) else weight
    if isinstance(weight, torch.nn.Module) and getattr(weight, 'bias', None) is not None:
        raise NotImplementedError('slotformer_amd: head_cross_entropy takes a head without bias')
    if not (torch.is_tensor(w) and w.is_cuda and w.dim() == 2):
        raise RuntimeError('slotformer_amd: head_cross_entropy needs a [V, K] weight on a HIP device; there is no CPU fallback')
    if w.requires_grad and not weight_grad:
        raise NotImplementedError('slotformer_amd: head_cross_entropy gives no gradient to the head weight unless asked (the weight gradient of the '
                                  'fused head is opt-in): pass weight_grad=True, freeze the head, or use train.linear + train.token_cross_entropy')
    V, K = w.shape
    if x.shape[-1] != K or not lib().sf_head_ce_ok(V, K):
        raise NotImplementedError(f'slotformer_amd: head_cross_entropy takes K a multiple of 32 in [32, 256] and V a multiple of 32 in [32, 2^20], '
                                  f'got x [..., {x.shape[-1]}] and a [{V}, {K}] head')
    if target.dtype not in (torch.int64, torch.int16) or target.numel() != x.numel() // K:
        raise ValueError(f'slotformer_amd: head_cross_entropy targets are int64 or int16 ids, one per row of x, got {target.dtype} {tuple(target.shape)}')
    if group_w is not None:
        group_w = group_w.detach().float().contiguous()
    packed = plans.cached(weight, 'head_ce', plans.signature(w), lambda: ops.pack_head_ce_weight(w.detach().float().contiguous()))
    return _HeadCrossEntropy.apply(x, w if w.requires_grad else None, packed, target.contiguous().reshape(-1), group_w, int(group), V)


class _LinearCat(torch.autograd.Function):
    """[x W1^T | x W2^T | ...] for bias-free projections that share their input (q|k|v of the STEVE decoder's attention,
    steve_transformer.py:30-40): ONE GEMM on the concatenated weight, one weight-gradient contraction, one data-gradient GEMM,
    instead of one of each per projection."""

    @staticmethod
    def forward(ctx, x, *weights):
        from . import ops
        xd = x.detach().float().contiguous()
        wcat = torch.cat([w.detach().float() for w in weights], 0).contiguous()
        ctx.save_for_backward(xd, wcat)
        ctx.sizes = [w.shape[0] for w in weights]
        return ops.linear(xd, wcat)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.float().contiguous()
        N, K = w.shape
        M = x.numel() // K
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w)
        ws = scratch(lib().sf_linear_bwd_workspace_bytes, M, N, K, device=w.device)
        check(lib().sf_linear_bwd_f32(x.data_ptr(), w.data_ptr(), None, dy.data_ptr(), ptr(dx), dw.data_ptr(), None, M, N, K, 0, ws.data_ptr(),
                                      ws.numel(), stream()))
        return (dx, ) + tuple(dw.split(ctx.sizes, 0))


def linear_cat(x, *layers):
    """x projected by several bias-free nn.Linear layers at once; returns the tuple of outputs (column slices)."""
    out = _LinearCat.apply(x, *[l_.weight for l_ in layers])
    return out.split([l_.weight.shape[0] for l_ in layers], -1)


def linear(x, layer, relu=False):
    """nn.Linear `layer` applied to x under autograd, on the HIP kernels."""
    return _Linear.apply(x, layer.weight, layer.bias, relu)


def layer_norm(x, layer):
    return _LayerNorm.apply(x, layer.weight, layer.bias, layer.eps)


# ---- dVAE nodes (dVAE.py:113-139, steve_utils.py:26-41, 100-126) ------------------------------------------------------
class _GroupNorm1(torch.autograd.Function):
    """Conv2dBlock's GroupNorm(1 group) + ReLU (+ the PixelShuffle(2) that follows it) on NHWC maps:
    sf_groupnorm1_nhwc_f32 / sf_groupnorm1_nhwc_bwd_f32 (statistics and ReLU gate recomputed from the saved input)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, relu, pixel_shuffle):
        from . import ops
        xd, g, b = x.detach().float().contiguous(), gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        ctx.save_for_backward(xd, g, b)
        ctx.cfg = (float(eps), int(bool(relu)), int(pixel_shuffle))
        return ops.groupnorm1_nhwc(xd, g, b, eps=eps, relu=relu, pixel_shuffle=pixel_shuffle)

    @staticmethod
    def backward(ctx, dy):
        x, g, b = ctx.saved_tensors
        eps, relu, r = ctx.cfg
        dy = dy.float().contiguous()
        F_, H, W, C_ = x.shape
        dx, dg, db = torch.empty_like(x), torch.empty_like(g), torch.empty_like(b)
        ws = scratch(lib().sf_groupnorm1_bwd_workspace_bytes, F_, H, W, C_, device=x.device)
        check(lib().sf_groupnorm1_nhwc_bwd_f32(x.data_ptr(), g.data_ptr(), b.data_ptr(), dy.data_ptr(), dx.data_ptr(), dg.data_ptr(),
                                               db.data_ptr(), F_, H, W, C_, eps, relu, r, ws.data_ptr(), ws.numel(), stream()))
        return dx, dg, db, None, None, None


def groupnorm1(x, gamma, beta, eps=1e-5, relu=True, pixel_shuffle=1):
    return _GroupNorm1.apply(x, gamma, beta, eps, relu, pixel_shuffle)


class _SoftmaxRows(torch.autograd.Function):
    """softmax((x + noise) * scale) over the last dim; with Gumbel noise and scale = 1/tau the relaxed one-hot sample of
    steve_utils.py:26-41 (the log-partition shift of log_softmax cancels in the softmax).  The noise is either the tensor
    `add` or, with `seed`, generated inside the kernel (sf_gumbel_softmax_rows_f32) and never stored: the backward only
    needs the output."""

    @staticmethod
    def forward(ctx, x, add, scale, seed):
        from . import ops
        xd = x.detach().float().contiguous()
        if seed is not None and add is None:
            y = ops.gumbel_softmax_rows(xd, seed, scale)
        else:
            y = ops.softmax_rows(xd, None if add is None else add.detach().float().contiguous(), scale)
        ctx.save_for_backward(y)
        ctx.scale = float(scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        dy = dy.float().contiguous()
        V = y.shape[-1]
        dx = torch.empty_like(y)
        check(lib().sf_softmax_rows_bwd_f32(y.data_ptr(), dy.data_ptr(), ctx.scale, dx.data_ptr(), y.numel() // V, V,
                                            stream()))
        return dx, None, None, None


def gumbel_softmax(logits, gumbels=None, tau=1., hard=False, seed=None):
    """steve_utils.py:26-41 on the last dim: relaxed sample, or the straight-through one-hot.  The Gumbel noise is `gumbels`
    when given, else drawn inside the kernel from `seed` (default: a fresh seed from torch's CPU generator)."""
    from . import ops
    if gumbels is None and seed is None:
        seed = _new_seed()
    y_soft = _SoftmaxRows.apply(logits, gumbels, 1. / tau, seed)
    if not hard:
        return y_soft
    idx = ops.argmax_rows(y_soft.detach())
    y_hard = torch.zeros_like(y_soft).scatter_(-1, idx.unsqueeze(-1), 1.)
    return y_hard - y_soft.detach() + y_soft


def gumbel_noise(seed, numel, start=0):
    """Host restatement of the in-kernel Gumbel noise (csrc/gumbel_noise.h: sf_gumbel) for tests: float32 [numel], the elements
    [start, start + numel) of the stream of `seed` (indices are uint32)."""
    import numpy as np

    def mix(h):
        h = h.astype(np.uint32)
        h ^= h >> np.uint32(16)
        h = (h * np.uint32(0x7feb352d)).astype(np.uint32)
        h ^= h >> np.uint32(15)
        h = (h * np.uint32(0x846ca68b)).astype(np.uint32)
        h ^= h >> np.uint32(16)
        return h

    with np.errstate(over='ignore'):
        inner = mix(np.array([np.uint32((seed >> 32) & 0xffffffff) + np.uint32(0x9e3779b9)], dtype=np.uint32))
        sseed = mix(np.array([np.uint32(seed & 0xffffffff)], dtype=np.uint32) ^ inner)[0]
        h = mix(np.arange(int(start), int(start) + int(numel), dtype=np.uint64).astype(np.uint32) ^ sseed)
    u = ((h >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(1.1920929e-7)
    return torch.from_numpy(-np.log(-np.log(u)))


def _mix32_np(h):
    """sf_mix32 (csrc/sf_common.h) on a NumPy uint32 array."""
    import numpy as np
    with np.errstate(over='ignore'):
        h = h.astype(np.uint32)
        h ^= h >> np.uint32(16)
        h = (h * np.uint32(0x7feb352d)).astype(np.uint32)
        h ^= h >> np.uint32(15)
        h = (h * np.uint32(0x846ca68b)).astype(np.uint32)
        h ^= h >> np.uint32(16)
    return h


def normal_noise(seed, tag, numel):
    """Host restatement of the in-kernel normal noise (csrc/normal_noise.h: sf_normal_seed / sf_normal; ops.normal_noise) for tests: the same
    hashed uniforms, Box-Muller evaluated in float64, returned as float32 [numel]."""
    import numpy as np
    seed, tag = int(seed) & 0xffffffffffffffff, int(tag) & 0xffffffff
    inner = _mix32_np(np.array([((seed >> 32) + 0x9e3779b9 * (tag + 1)) & 0xffffffff], dtype=np.uint32))
    sseed = _mix32_np(np.array([seed & 0xffffffff], dtype=np.uint32) ^ inner)[0]
    i2 = np.arange(int(numel), dtype=np.uint32) * np.uint32(2)
    u1 = ((_mix32_np(i2 ^ sseed) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.**-23
    u2 = ((_mix32_np((i2 + np.uint32(1)) ^ sseed) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.**-23
    eps = np.sqrt(-2. * np.log(u1)) * np.cos(np.float64(np.float32(6.2831855)) * u2)
    return torch.from_numpy(eps.astype(np.float32))


class _KernelSample(torch.autograd.Function):
    """(kernels, kld) of sf_kernel_sample_fwd_f32 / _bwd_f32: the sampling of StoSAVi's stochastic kernels and their KL term in one launch each
    way.  Saves `dist` (and the noise tensor when one was given): a seeded draw is regenerated in the backward."""

    @staticmethod
    def forward(ctx, dist, slot_size, prior_log_var, noise, seed, tag):
        from . import ops
        dist = dist.detach().float().contiguous()
        noise = None if noise is None else noise.detach().float().contiguous()
        kld_sum = torch.zeros(1, dtype=torch.float64, device=dist.device)
        kernels = ops.kernel_sample_fwd(dist, slot_size, prior_log_var, kld_sum, noise, seed, tag)
        rows = dist.numel() // (2 * slot_size)
        ctx.save_for_backward(dist, noise)
        ctx.args = (slot_size, prior_log_var, seed, tag, rows)
        return kernels, (kld_sum[0] / rows).float()

    @staticmethod
    def backward(ctx, d_kernels, d_kld):
        from . import ops
        dist, noise = ctx.saved_tensors
        slot_size, prior_log_var, seed, tag, rows = ctx.args
        d_dist = ops.kernel_sample_bwd(dist, slot_size, prior_log_var, d_kernels.float().contiguous(), d_kld.float().reshape(1).contiguous(),
                                       1. / rows, noise, seed, tag)
        return d_dist, None, None, None, None, None


def kernel_sample(dist, slot_size, prior_log_var, noise=None, seed=None, tag=0):
    """StoSAVi's stochastic kernels under autograd (savi.py:337-365): dist [..., 2 * slot_size] = (mu | log_var) -> (kernels [..., slot_size] =
    mu + eps * exp(log_var / 2), kld), kld = the KL divergence from the prior N(mu, exp(prior_log_var)) summed over channels and averaged over rows
    (`host.losses.kernel_kld`), a differentiable float32 scalar on the device.  eps is `noise` (kernels' shape) when given, else
    `ops.normal_noise(seed, tag, kernels.shape)` generated inside the kernel and regenerated in the backward.  No synchronisation."""
    if noise is None and seed is None:
        raise ValueError('slotformer_amd: kernel_sample needs noise= or seed=')
    return _KernelSample.apply(dist, int(slot_size), float(prior_log_var), noise, None if noise is not None or seed is None else int(seed), int(tag))


def linear_weight(x, weight, bias=None, relu=False):
    """act(x W^T + b) for a bare [N, K] weight under autograd.  The backward contractions work on multiples of 64, so other
    widths (the dVAE's 48-wide patch vectors, its 3-channel output) are zero-padded up and the result sliced back."""
    N, K = weight.shape
    Np, Kp = -(-N // 64) * 64, -(-K // 64) * 64
    if Kp != K:
        x, weight = tnf.pad(x, (0, Kp - K)), tnf.pad(weight, (0, Kp - K))
    if Np != N:
        weight = tnf.pad(weight, (0, 0, 0, Np - N))
        bias = tnf.pad(bias, (0, Np - N)) if bias is not None else None
    y = _Linear.apply(x, weight, bias, relu)
    return y[..., :N] if Np != N else y


def conv3x3_nhwc(x, weight):
    """Bias-free 3x3 / stride-1 / pad-1 convolution of an NHWC map under autograd (the two 3x3 Conv2dBlocks of the dVAE decoder,
    dVAE.py:39,45) as ONE GEMM over the nine shifted copies of the map: the copies and their adjoint (shift-and-add) are data
    movement, the contraction and both of its gradients run on the HIP GEMM kernels."""
    F_, H, W, C_ = x.shape
    xp = tnf.pad(x, (0, 0, 1, 1, 1, 1))
    cols = torch.cat([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], -1)   # [F,H,W,9C], (ky, kx, c) order
    w2 = weight.permute(0, 2, 3, 1).reshape(weight.shape[0], 9 * C_)
    return linear_weight(cols, w2)


def flat_bucket_layout(param_groups):
    """Where the parameter groups of a FlatAdam sit in its bucket.  param_groups: a list of dicts with 'params' (as
    torch.optim takes them).  Each group's parameters that require a gradient lie contiguously, in group order: returns
    (params, begins) -- the flat parameter list and the element offset at which each group begins (ascending, begins[0] == 0)."""
    params, begins, off = [], [], 0
    for g in param_groups:
        begins.append(off)
        for p in g['params']:
            if p.requires_grad:
                params.append(p)
                off += p.numel()
    return params, begins


def grad_norm_grid(n):
    """Workgroups of the sf_grad_clip_coef_f32 launch over a bucket of n elements (its workspace holds a 16-byte counter and 16
    bytes per workgroup)."""
    return (int(lib().sf_grad_norm_workspace_bytes(n)) - 16) // 16


class FlatAdam:
    """Adam (torch.optim.Adam defaults: betas (0.9, 0.999), eps 1e-8, no weight decay -- the reference's optimiser) over ONE
    flat bucket.  The parameters are re-pointed at views of a single fp32 tensor (their values are kept), gradients are
    gathered into a matching flat tensor, and a step is one `sf_adam_flat_f32` launch -- plus, under data parallelism
    (`allreduce=True`), one RCCL all-reduce of that gradient bucket first.  `lr` may be changed between steps (schedules:
    `warmup_cosine_lr`).

    params: an iterable of tensors, or a list of dicts {'params': [...], 'lr': optional} as torch.optim.Adam takes them (STEVE's
    two rates: `steve_param_groups`).  Each group is contiguous in the bucket, in group order (`flat_bucket_layout`), and
    `param_groups` is the list of dicts with 'params' and a mutable 'lr' that a schedule written for torch.optim assigns to;
    `lr` is group 0's rate.  With more than one group the step is one `sf_adam_flat_groups_f32` launch.

    clip_grad: clip the gradient's global L2 norm to this value, torch.nn.utils.clip_grad_norm_'s rule (the reference's
    `clip_grad`, base_slots/method.py), applied to the all-reduced gradient as under DDP.  It adds ONE launch
    (`sf_grad_clip_coef_f32`) whose coefficient the update reads from device memory: no pass over the gradients, no host round
    trip, nothing allocated per step.  `p.grad` is left UNCLIPPED (clip_grad_norm_ rescales it in place; here the scale is
    applied inside the update).  `grad_norm` is a one-element device view of the norm before clipping (what the reference
    logs), `grad_nonfinite` one of a flag that is 1.0 when some gradient element was NaN or +-Inf.  As with torch a non-finite
    gradient propagates into the parameters; the flag is there for the caller to look at when it chooses."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, allreduce=False, clip_grad=None):
        params = list(params)
        if params and isinstance(params[0], dict):
            groups = [{'params': list(g['params']), 'lr': float(g.get('lr', lr))} for g in params]
        else:
            groups = [{'params': params, 'lr': float(lr)}]
        if not 1 <= len(groups) <= 8:
            raise ValueError('slotformer_amd: FlatAdam takes 1 to 8 parameter groups')
        self.params, begins = flat_bucket_layout(groups)
        for g in groups:
            g['params'] = [p for p in g['params'] if p.requires_grad]
        self.param_groups = groups
        if not self.params or not self.params[0].is_cuda:
            raise RuntimeError('slotformer_amd: FlatAdam needs parameters on a HIP device; there is no CPU fallback')
        self.betas, self.eps, self.allreduce, self.steps = betas, float(eps), allreduce, 0
        self.clip_grad = float(clip_grad) if clip_grad else None
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat = torch.empty(n, dtype=torch.float32, device=dev)
        off = 0
        for p in self.params:
            k = p.numel()
            self.flat[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.flat[off:off + k].view_as(p)   # same values, now a view of the bucket
            off += k
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        self._groups = (sf_adam_group * len(groups))()
        for g, b in zip(self._groups, begins):
            g.begin = b
        self.grad_norm = self.grad_nonfinite = None
        if self.clip_grad:
            # norm, coefficient, non-finite flag; the workspace's arrival counter starts at zero and every call leaves it there
            self._clip_out = torch.zeros(3, dtype=torch.float32, device=dev)
            self._clip_ws = scratch(lib().sf_grad_norm_workspace_bytes, n, device=dev).zero_()
            self.grad_norm, self.grad_nonfinite = self._clip_out[0:1], self._clip_out[2:3]

    @property
    def lr(self):
        return self.param_groups[0]['lr']

    @lr.setter
    def lr(self, value):
        self.param_groups[0]['lr'] = float(value)

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    def step(self, gathered=False):
        """One update.  gathered=True: the gradients already sit in `self.grad` (a backward that wrote into the bucket:
        `rollout_clips_with_grad(..., grad_out=opt.grad)`), so the per-parameter copies out of `p.grad` are skipped."""
        off = 0
        for p in (() if gathered else self.params):
            k = p.numel()
            if p.grad is None:
                self.grad[off:off + k].zero_()
            else:
                self.grad[off:off + k].copy_(p.grad.reshape(-1))
            off += k
        if self.allreduce:
            parallel.allreduce_flat(self.grad)
        self.steps += 1
        st = stream()
        scale = None
        if self.clip_grad:
            check(lib().sf_grad_clip_coef_f32(self.grad.data_ptr(), self.grad.numel(), self.clip_grad, self._clip_out.data_ptr(),
                                              self._clip_ws.data_ptr(), self._clip_ws.numel(), st))
            scale = self._clip_out.data_ptr() + 4
        if scale is None and len(self.param_groups) == 1:
            check(lib().sf_adam_flat_f32(self.flat.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                         self.flat.numel(), self.steps, float(self.lr), float(self.betas[0]), float(self.betas[1]), self.eps, st))
        else:
            for g, d in zip(self._groups, self.param_groups):
                g.lr = float(d['lr'])
            check(lib().sf_adam_flat_groups_f32(self.flat.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(),
                                                self.exp_avg_sq.data_ptr(), self.flat.numel(), self.steps, self._groups, len(self._groups),
                                                float(self.betas[0]), float(self.betas[1]), self.eps, scale, st))
        # The kernel wrote the parameters through a raw pointer: tell torch (and, through `_version`, the plan cache
        # of plans.py, which is keyed on (data_ptr, _version)) that their contents changed -- otherwise derived / packed
        # weight copies built before this step would keep being served.
        try:
            torch._C._increment_version(self.params)   # (one call for the list: a call per tensor costs the host ~80 us each)
        except TypeError:   # a torch whose _increment_version takes one tensor
            for p in self.params:
                torch._C._increment_version(p)


    def state_dict(self):
        """torch.optim.Adam's state dict: per parameter (ids in bucket order) `step`, `exp_avg`, `exp_avg_sq` -- the moments are VIEWS of the
        flat buffers, clone them to keep a snapshot -- and `param_groups` with torch's keys (weight_decay 0, amsgrad False).  What a
        torch.optim.Adam over the same parameters in the same order loads, and what the reference's checkpoints hold under 'optimizer'."""
        state, groups, off, i = {}, [], 0, 0
        for g in self.param_groups:
            ids = []
            for p in g['params']:
                k = p.numel()
                if self.steps > 0:   # (torch has no state before the first step)
                    state[i] = {'step': torch.tensor(float(self.steps)), 'exp_avg': self.exp_avg[off:off + k].view_as(p),
                                'exp_avg_sq': self.exp_avg_sq[off:off + k].view_as(p)}
                ids.append(i)
                off += k
                i += 1
            groups.append({'lr': g['lr'], 'betas': tuple(self.betas), 'eps': self.eps, 'weight_decay': 0, 'amsgrad': False, 'maximize': False,
                           'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None, 'decoupled_weight_decay': False,
                           'params': ids})
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, sd):
        """Resume from `state_dict()`'s layout -- FlatAdam's own or torch.optim.Adam's over the same parameters in the same order.  The moments are
        copied into the flat buffers; lr, betas and eps are taken from the groups.  Raises ValueError for what the flat update cannot express:
        other group sizes, weight decay, amsgrad, maximize, or parameters at different step counts."""
        groups = sd['param_groups']
        if len(groups) != len(self.param_groups) or any(len(a['params']) != len(b['params']) for a, b in zip(groups, self.param_groups)):
            raise ValueError('slotformer_amd: FlatAdam.load_state_dict: the parameter groups do not match')
        for a in groups:
            if a.get('weight_decay', 0) or a.get('amsgrad', False) or a.get('maximize', False):
                raise ValueError('slotformer_amd: FlatAdam has no weight decay, amsgrad or maximize')
        betas, eps = tuple(groups[0].get('betas', self.betas)), float(groups[0].get('eps', self.eps))
        if any(tuple(a.get('betas', betas)) != betas or float(a.get('eps', eps)) != eps for a in groups):
            raise ValueError('slotformer_amd: FlatAdam has one betas / eps for all groups')
        ids = [i for a in groups for i in a['params']]
        state = sd['state']
        steps = {int(float(state[i]['step'])) for i in ids if i in state}
        if len(steps) > 1 or (state and any(i not in state for i in ids)):
            raise ValueError('slotformer_amd: FlatAdam keeps ONE step count: every parameter must have the same')
        off = 0
        for i, p in zip(ids, self.params):
            k = p.numel()
            for buf, key in ((self.exp_avg, 'exp_avg'), (self.exp_avg_sq, 'exp_avg_sq')):
                if i in state:
                    if state[i][key].numel() != k:
                        raise ValueError(f'slotformer_amd: FlatAdam.load_state_dict: parameter {i} has {k} elements, its {key} {state[i][key].numel()}')
                    buf[off:off + k].copy_(state[i][key].reshape(-1))
                else:
                    buf[off:off + k].zero_()
            off += k
        self.steps = steps.pop() if steps else 0
        self.betas, self.eps = betas, eps
        for g, a in zip(self.param_groups, groups):
            g['lr'] = float(a['lr'])


def warmup_cosine_lr(step, total_steps, warmup_steps, max_lr, min_lr=0.):
    """Learning rate at `step` of the schedule every reference configuration names: linear warm-up, then cosine
    (base_slots/method.py: min_lr = lr / 100 for the slot models, 0 for STEVE; once per group for STEVE's two rates).
    Linear from min_lr to max_lr over the first `warmup_steps` steps, then
    min_lr + (max_lr - min_lr) * (1 + cos(pi * (step - warmup_steps) / (total_steps - warmup_steps))) / 2.
    A plain host function: assign its value to `FlatAdam.param_groups[k]['lr']` before the step.  The reference takes
    nerv's CosineAnnealingWarmupRestarts, which is not available here: this is the common single-cycle form and is NOT
    pinned against nerv."""
    import math
    if step < warmup_steps:
        return min_lr + (max_lr - min_lr) * step / warmup_steps
    if total_steps <= warmup_steps:
        return max_lr
    t = min(max((step - warmup_steps) / (total_steps - warmup_steps), 0.), 1.)
    return min_lr + (max_lr - min_lr) * (1. + math.cos(math.pi * t)) / 2.


def steve_param_groups(model, lr, dec_lr):
    """The two Adam groups STEVE trains with (base_slots/method.py:245-261): every trainable parameter whose name does not
    contain 'trans_decoder' at `lr`, the Transformer decoder's at `dec_lr`.  The frozen dVAE is in neither, nor are the decoder's
    fixed attention masks (parameters without a gradient, which torch.optim.Adam would carry along and never touch)."""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    return [{'params': [p for n, p in named if 'trans_decoder' not in n], 'lr': lr},
            {'params': [p for n, p in named if 'trans_decoder' in n], 'lr': dec_lr}]


class amp_bf16:
    """Context manager for the AMP-bf16 policy of the training path: inside it the GEMM / convolution / weight-gradient
    cores contract single-pass bf16 operands with f32 accumulation (library precision mode 2); parameters, activations,
    gradients and the optimizer state stay fp32.  The counterpart of the reference's `--fp16` autocast (train.py:84)."""

    def __enter__(self):
        self.old = lib().sf_get_precision()
        check(lib().sf_set_precision(2))
        return self

    def __exit__(self, *exc):
        check(lib().sf_set_precision(self.old))
        return False


def dropout_keep_mask(seed, step, layer, site, numel, p):
    """Host restatement of the library's dropout mask (csrc/dropout_mask.h: sf_keep / site_seed) for tests and tools:
    bool [numel], True = kept.  site: 0 attention weights, 1 attention output, 2 FFN hidden, 3 FFN output."""
    import numpy as np

    def mix(h):
        h = h.astype(np.uint32)
        h ^= h >> np.uint32(16)
        h = (h * np.uint32(0x7feb352d)).astype(np.uint32)
        h ^= h >> np.uint32(15)
        h = (h * np.uint32(0x846ca68b)).astype(np.uint32)
        h ^= h >> np.uint32(16)
        return h

    with np.errstate(over='ignore'):
        tag = np.uint32((step * 64 + layer) * 4 + site)
        inner = mix(np.array([np.uint32((seed >> 32) & 0xffffffff) + np.uint32(0x9e3779b9) * (tag + np.uint32(1))], dtype=np.uint32))
        sseed = mix(np.array([np.uint32(seed & 0xffffffff)], dtype=np.uint32) ^ inner)[0]
        idx = np.arange(numel, dtype=np.uint32)
        u = mix(idx ^ sseed) >> np.uint32(8)
    return u >= np.uint32(int(float(np.float32(p)) * 16777216.0))


# ---------------------------------------------------------------------------------------------------------------------
# Physion VQA readout (physion_vqa/models/readout.py) under autograd: two nodes over the kernels of csrc/physion_readout.hip
# ---------------------------------------------------------------------------------------------------------------------
class _Readout(torch.autograd.Function):
    """logits [B] (and the per-step logits [B,T], not differentiable) of one head; the slots are frozen inputs, as in the reference."""

    @staticmethod
    def forward(ctx, slots, video_index, video_len, agg, want_steps, W1, b1, w2, b2):
        from . import ops
        logits, t_star, steps, pairs = ops.physion_readout_fwd(slots, W1, b1, w2, b2, agg, video_index=video_index, video_len=video_len,
                                                               want_steps=want_steps, want_pairs=agg == 'max')
        ctx.keep = (slots, video_index, video_len, agg, t_star, pairs)
        ctx.save_for_backward(W1, b1, w2, b2)
        steps = steps[0] if want_steps else logits.new_empty(0)
        ctx.mark_non_differentiable(steps)
        return logits[0], steps

    @staticmethod
    def backward(ctx, g, _d_steps):
        from . import ops
        slots, video_index, video_len, agg, t_star, pairs = ctx.keep
        W1, b1, w2, b2 = ctx.saved_tensors
        dW1, db1, dw2, db2 = ops.physion_readout_bwd(slots, W1, b1, w2, g, t_star, agg, pair_star=pairs, video_index=video_index,
                                                     video_len=video_len)
        return None, None, None, None, None, dW1.view_as(W1), db1.view_as(b1), dw2.view_as(w2), db2.view_as(b2)


class _ReadoutLoss(torch.autograd.Function):
    """Mean BCE-with-logits of logits [B] against labels: one score launch; its backward is the g that launch wrote."""

    @staticmethod
    def forward(ctx, logits, labels):
        from . import ops
        loss, g, _, _ = ops.physion_readout_score(logits, labels)
        ctx.save_for_backward(g)
        ctx.shape = logits.shape
        return loss[0]

    @staticmethod
    def backward(ctx, d_loss):
        g, = ctx.saved_tensors
        return (g[0] * d_loss).view(ctx.shape), None


def readout_with_grad(readout, slots, video_index=None, video_len=None, return_steps=False):
    """PhysionReadout.forward under autograd (readout.py:56-79): slots [V,T,N,C] -> logits [B] (with return_steps also the per-step logits [B,T]).
    Forward and backward are `sf_physion_readout_fwd_f32` / `sf_physion_readout_bwd_f32`; the gradient reaches each video's winning frame only."""
    logits, steps = _Readout.apply(slots, video_index, video_len, readout.agg_func, bool(return_steps), readout.linear1.weight, readout.linear1.bias,
                                   readout.linear2.weight, readout.linear2.bias)
    return (logits, steps) if return_steps else logits


def readout_loss(logits, labels):
    """F.binary_cross_entropy_with_logits(logits, labels) (readout.py:81-87) on the score kernel, differentiable in `logits`."""
    return _ReadoutLoss.apply(logits, labels)


# ---------------------------------------------------------------------------------------------------------------------
# PHYRE task-success readout (phyre_planning/models/readout.py) under autograd: ONE node over the two calls of
# csrc/phyre_readout_train.hip -- a layer is one launch forward and one launch backward
# ---------------------------------------------------------------------------------------------------------------------
def phyre_learnable_pe(readout):
    return bool(isinstance(readout.enc_t_pe, torch.nn.Parameter) and readout.enc_t_pe.requires_grad)


def phyre_readout_parameters(readout):
    """The trainable leaves of a PHYREReadout in bucket order -- the order `ops.phyre_grad_layout` lays the gradients out in: in_proj, CLS, enc_t_pe
    (when learnable), every layer's leaves, cls_mlp.  (cls_mlp.2.bias, the one leaf of odd size, comes last: every other leaf of a flat bucket
    over this list starts 16-byte aligned.)"""
    ps = [readout.in_proj.weight, readout.in_proj.bias, readout.CLS]
    if phyre_learnable_pe(readout):
        ps.append(readout.enc_t_pe)
    for layer in readout.transformer_encoder.layers:
        ps += [_leaf(layer, n) for n in _LAYER_LEAVES]
    return ps + [readout.cls_mlp[0].weight, readout.cls_mlp[0].bias, readout.cls_mlp[2].weight, readout.cls_mlp[2].bias]


def phyre_readout_model(readout):
    """The `sf_phyre_readout_model` descriptor of a PHYREReadout on the device: raw pointers to its float32 parameters in their torch layouts (no
    packed copy: the training calls split what they need every step).  -> (struct, keep): hold `keep` while the struct is in use.  The pointers
    follow the parameters' storage, so build it after a FlatAdam has re-pointed them at its bucket."""
    from ._lib import sf_phyre_readout_model, sf_tfm_layer
    if not readout.shape_ok():
        from . import ops
        raise NotImplementedError(f'PHYREReadout({readout.readout_dict!r}) has no training kernel: {ops.PHYRE_LIMITS}')
    keep = []

    def dp(t):
        t = t.detach()
        if not t.is_cuda:
            raise RuntimeError('slotformer_amd: PHYREReadout trains on a HIP device only; there is no CPU fallback')
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('slotformer_amd: PHYREReadout trains on contiguous float32 parameters')
        keep.append(t)
        return t.data_ptr()

    rd = readout.readout_dict
    m = sf_phyre_readout_model()
    m.num_slots, m.slot_size, m.d_model, m.num_heads, m.ffn_dim, m.num_layers = (readout.num_slots, readout.slot_size, rd['d_model'], rd['num_heads'],
                                                                                 rd['ffn_dim'], rd['num_layers'])
    m.in_proj_w, m.in_proj_b, m.enc_t_pe, m.cls = dp(readout.in_proj.weight), dp(readout.in_proj.bias), dp(readout.enc_t_pe), dp(readout.CLS)
    arr = (sf_tfm_layer * rd['num_layers'])()
    for i, layer in enumerate(readout.transformer_encoder.layers):
        for leaf, field in zip(_LAYER_LEAVES, _LAYER_FIELDS):
            setattr(arr[i], field, dp(_leaf(layer, leaf)))
    m.layers = C.cast(arr, C.POINTER(sf_tfm_layer))
    m.mlp_w1, m.mlp_b1 = dp(readout.cls_mlp[0].weight), dp(readout.cls_mlp[0].bias)
    m.mlp_w2, m.mlp_b2 = dp(readout.cls_mlp[2].weight), dp(readout.cls_mlp[2].bias)
    keep.append(arr)
    return m, keep


class _PhyreReadout(torch.autograd.Function):
    """logits [B] = PHYREReadout(slots) as a single autograd node; the slots are frozen inputs, as in the reference."""

    @staticmethod
    def forward(ctx, readout, slots, sel, video_index, p, seed, grad_out, *params):
        from . import ops
        model, keep = phyre_readout_model(readout)
        logits, ws, _, _ = ops.phyre_readout_train_fwd(model, slots, sel, video_index=video_index, p=p, seed=seed)
        ctx.keep = (readout, model, keep, slots, sel, video_index, p, seed, grad_out, ws, params)
        return logits

    @staticmethod
    def backward(ctx, g):
        from . import ops
        readout, model, keep, slots, sel, video_index, p, seed, grad_out, ws, params = ctx.keep
        flat = ops.phyre_readout_train_bwd(model, slots, sel, g, ws, video_index=video_index, p=p, seed=seed, learnable_pe=phyre_learnable_pe(readout),
                                           out=grad_out)
        ctx.keep = None
        if grad_out is not None:   # the caller's bucket holds them: nothing for autograd to accumulate
            return (None, ) * (7 + len(params))
        readout.last_grad_bucket = flat
        return (None, ) * 7 + tuple(g_ if ctx.needs_input_grad[7 + i] else None for i, g_ in enumerate(_split(flat, params)))


def phyre_readout_with_grad(readout, slots, sel=None, video_index=None, p=None, seed=None, grad_out=None):
    """PHYREReadout.forward under autograd (readout.py: in_proj + temporal position row, CLS, the pre-LN encoder with its dropout, cls_mlp on the CLS
    row): slots [V, T_all, N, C] on the device -> logits [B], differentiable in every parameter.  One node over `sf_phyre_readout_train_fwd_f32` /
    `sf_phyre_readout_train_bwd_f32`.  sel: the frame of every token group (default readout.sel_slots; -1: a frame of zeros); video_index [B]:
    picks the batch out of the slots without a gather.  p: the dropout rate -- default the layers' own when readout.training, else 0; seed: the
    seed of the masks (default a fresh one).  grad_out: a flat fp32 buffer laid out as FlatAdam's bucket over phyre_readout_parameters(readout)
    (`FlatAdam.grad`): the backward writes the gradients there -- then step with `FlatAdam.step(gathered=True)` -- and leaves `.grad` alone."""
    require_device(slots, what='the slots')
    if p is None:
        p = float(readout.transformer_encoder.layers[0].dropout.p) if readout.training else 0.0
    if seed is None:
        seed = _new_seed() if p > 0 else 0
    sel = list(readout.sel_slots) if sel is None else [int(s) for s in sel]
    if len(sel) != readout.T:
        raise ValueError(f'PHYREReadout: the frame table holds {readout.T} entries (len(sel_slots)), got {len(sel)}')
    return _PhyreReadout.apply(readout, slots, sel, video_index, float(p), int(seed), grad_out, *phyre_readout_parameters(readout))


# ---------------------------------------------------------------------------------------------------------------------
# The Aloe reasoner (clevrer_vqa/models/transformer.py) under autograd: ONE node over the two calls of csrc/aloe_train.hip
# ---------------------------------------------------------------------------------------------------------------------
def aloe_parameters(tm):
    """The trainable leaves of a CLEVRERTransformerModel in bucket order -- the order `ops.aloe_grad_layout` lays the gradients out in: CLS, pos_enc,
    vision_in_proj, q_in_proj, every layer's leaves, the first linear of both answer MLPs, then the leaves of odd size: q_embedding and the second
    linear of both MLPs.  (The five id pairs are fixed: requires_grad False.)"""
    ps = [tm.CLS, tm.transformer_encoder.pos_enc, tm.vision_in_proj.weight, tm.vision_in_proj.bias, tm.q_in_proj.weight, tm.q_in_proj.bias]
    for layer in tm.transformer_encoder.layers:
        ps += [_leaf(layer, n) for n in _LAYER_LEAVES]
    return ps + [tm.cls_answer_mlp[0].weight, tm.cls_answer_mlp[0].bias, tm.mc_answer_mlp[0].weight, tm.mc_answer_mlp[0].bias, tm.q_embedding.weight,
                 tm.cls_answer_mlp[2].weight, tm.cls_answer_mlp[2].bias, tm.mc_answer_mlp[2].weight, tm.mc_answer_mlp[2].bias]


def aloe_model(tm, num_slots, T, text_len):
    """The `sf_aloe_model` descriptor of a CLEVRERTransformerModel on the device for sequences of 1 + T * num_slots + text_len tokens: raw pointers
    to its float32 parameters in their torch layouts.  -> (struct, keep): hold `keep` while the struct is in use.  The pointers follow the
    parameters' storage, so build it after a FlatAdam has re-pointed them at its bucket."""
    from ._lib import sf_aloe_model, sf_tfm_layer
    from . import ops
    td = tm.transformer_dict
    if 1 + T * num_slots + text_len != tm.input_len:
        raise ValueError(f'CLEVRERTransformerModel: 1 + {T} frames x {num_slots} slots + {text_len} text positions, the position table holds '
                         f'{tm.input_len}')
    if not (td['norm_first'] and ops.aloe_train_ok(num_slots, tm.vision_in_proj.in_features - 2, T, text_len, tm.d_model, td['num_heads'], td['ffn_dim'],
                                                   td['num_layers'])):
        raise NotImplementedError(f'CLEVRERTransformerModel({td!r}) on {num_slots} slots, {T} frames, {text_len} text positions has no training '
                                  f'kernel: {ops.ALOE_LIMITS}')
    keep = []

    def dp(t):
        t = t.detach()
        if not t.is_cuda:
            raise RuntimeError('slotformer_amd: CLEVRERAloe trains on a HIP device only; there is no CPU fallback')
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('slotformer_amd: CLEVRERAloe trains on contiguous float32 parameters')
        keep.append(t)
        return t.data_ptr()

    m = sf_aloe_model()
    m.num_slots, m.slot_size, m.T, m.text_len, m.question_len = num_slots, tm.vision_in_proj.in_features - 2, T, text_len, tm.question_len
    m.d_model, m.num_heads, m.ffn_dim, m.num_layers = tm.d_model, td['num_heads'], td['ffn_dim'], td['num_layers']
    m.vocab, m.emb_dim = tm.q_embedding.weight.shape
    m.mlp_hidden, m.num_answers = tm.cls_answer_mlp[0].out_features, tm.num_answer_classes
    m.cls, m.pos = dp(tm.CLS), dp(tm.transformer_encoder.pos_enc)
    m.vision_w, m.vision_b = dp(tm.vision_in_proj.weight), dp(tm.vision_in_proj.bias)
    m.q_embedding, m.q_in_proj_w, m.q_in_proj_b = dp(tm.q_embedding.weight), dp(tm.q_in_proj.weight), dp(tm.q_in_proj.bias)
    arr = (sf_tfm_layer * td['num_layers'])()
    for i, layer in enumerate(tm.transformer_encoder.layers):
        for leaf, field in zip(_LAYER_LEAVES, _LAYER_FIELDS):
            setattr(arr[i], field, dp(_leaf(layer, leaf)))
    m.layers = C.cast(arr, C.POINTER(sf_tfm_layer))
    for kind, mlp in (('cls', tm.cls_answer_mlp), ('mc', tm.mc_answer_mlp)):
        for name, t in (('w1', mlp[0].weight), ('b1', mlp[0].bias), ('w2', mlp[2].weight), ('b2', mlp[2].bias)):
            setattr(m, f'{kind}_{name}', dp(t))
    keep.append(arr)
    return m, keep


def _aloe_model_cached(tm, num_slots, T, text_len):
    """`aloe_model` kept in the module's plan cache (plans.py: it copies and pickles as empty, and `plans.invalidate` drops it) for as long as
    the geometry and the storage of every parameter stay what they were: an optimiser that re-points the parameters, a .to(), a load into new
    tensors give a new descriptor.  The descriptor holds pointers only, so a parameter's version does not enter the key."""
    from . import plans
    key = (num_slots, T, text_len) + tuple(p.data_ptr() for p in aloe_parameters(tm))
    return plans.cached(tm, 'aloe_train_model', key, aloe_model, tm, num_slots, T, text_len)


class _Aloe(torch.autograd.Function):
    """(cls_logits [B1, A], mc_logits [Bn]) = CLEVRERTransformerModel(batch) as a single autograd node; the slots are frozen inputs."""

    @staticmethod
    def forward(ctx, tm, slots, batch, p, seed, grad_out, *params):
        from . import ops
        model, keep = _aloe_model_cached(tm, slots.shape[2], int(batch.get('num_frames') or slots.shape[1]), batch['tokens'].shape[-1])
        cls_logits, mc_logits, ws, _, _ = ops.aloe_train_fwd(model, slots, batch, p=p, seed=seed)
        ctx.keep = (tm, model, keep, slots, batch, p, seed, grad_out, ws, params)
        return cls_logits, mc_logits

    @staticmethod
    def backward(ctx, g_cls, g_mc):
        from . import ops
        tm, model, keep, slots, batch, p, seed, grad_out, ws, params = ctx.keep
        flat = ops.aloe_train_bwd(model, slots, batch, g_cls, g_mc, ws, p=p, seed=seed, out=grad_out)
        ctx.keep = None
        if grad_out is not None:   # the caller's bucket holds them: nothing for autograd to accumulate
            return (None, ) * (6 + len(params))
        tm.last_grad_bucket = flat
        return (None, ) * 6 + tuple(g_ if ctx.needs_input_grad[6 + i] else None for i, g_ in enumerate(_split(flat, params)))


def aloe_with_grad(tm, slots, batch, p=None, seed=None, grad_out=None):
    """CLEVRERTransformerModel.forward under autograd: slots [V, T_all, N, C] on the device, batch = dict(tokens [B, text_len], pad_mask, B1 -- the
    first B1 sequences are descriptive questions, the others the choices of multiple-choice ones --, video_index [B], start [B], frame_offset,
    num_frames) -> (cls_logits [B1, A], mc_logits [Bn]), differentiable in every parameter.  One node over `sf_aloe_train_fwd_f32` /
    `sf_aloe_train_bwd_f32`.  p: the dropout rate -- default the layers' own when tm.training, else 0; seed: the seed of the masks (default a
    fresh one).  grad_out: a flat fp32 buffer laid out as FlatAdam's bucket over aloe_parameters(tm) (`FlatAdam.grad`): the backward writes the
    gradients there -- then step with `FlatAdam.step(gathered=True)` -- and leaves `.grad` alone."""
    require_device(slots, what='the slots')
    if p is None:
        p = float(tm.transformer_encoder.layers[0].dropout.p) if tm.training else 0.0
    if seed is None:
        seed = _new_seed() if p > 0 else 0
    return _Aloe.apply(tm, slots, batch, float(p), int(seed), grad_out, *aloe_parameters(tm))


class _AloeLoss(torch.autograd.Function):
    """w_cls * cross-entropy + w_mc * BCE-with-logits on the score-gradient launch; its backward is the two gradients that launch wrote."""

    @staticmethod
    def forward(ctx, cls_logits, mc_logits, cls_labels, mc_labels, w_cls, w_mc):
        from . import ops
        losses, g_cls, g_mc = ops.aloe_score_grad(cls_logits, cls_labels, mc_logits, mc_labels, w_cls, w_mc)
        ctx.save_for_backward(g_cls, g_mc)
        ctx.mark_non_differentiable(losses)
        return w_cls * losses[0] + w_mc * losses[1], losses

    @staticmethod
    def backward(ctx, d_loss, _d_losses):
        g_cls, g_mc = ctx.saved_tensors
        return g_cls * d_loss, g_mc * d_loss, None, None, None, None


def aloe_loss(cls_logits, mc_logits, cls_labels, mc_labels, w_cls=1., w_mc=1.):
    """(w_cls * F.cross_entropy(cls_logits, cls_labels) + w_mc * F.binary_cross_entropy_with_logits(mc_logits, mc_labels), losses [2]) -- the
    reference's training loss (transformer.py: loss_function; an empty kind counts 0) -- differentiable in both logits; one launch."""
    return _AloeLoss.apply(cls_logits, mc_logits, cls_labels, mc_labels, float(w_cls), float(w_mc))
