"""Torch-tensor wrappers over the C ABI building blocks (device memory + stream plumbing only).

Every function requires contiguous float32 tensors on a HIP device and launches on torch's
current stream.  There is no CPU path.
"""
import torch

from ._call import ptr, require_device, scratch, stream
from ._lib import lib, check


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError('slotformer_amd ops need contiguous float32 tensors on a HIP device '
                               f'(got {type(t).__name__} {getattr(t, "dtype", None)} '
                               f'{getattr(t, "device", None)}); there is no CPU fallback')


def linear(x, weight, bias=None, ln=None, residual=None, relu=False, ln_eps=1e-5):
    """act(LN?(x) @ weight.T + bias) + residual;  x [..., K], weight [N, K]."""
    _chk(x, weight, bias, residual, *(ln or ()))
    K = x.shape[-1]
    N = weight.shape[0]
    M = x.numel() // K
    out = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
    g, b = (ln if ln is not None else (None, None))
    check(lib().sf_linear_f32(ptr(x), K, ptr(weight), ptr(bias), ptr(g), ptr(b), ln_eps, ptr(residual), N, ptr(out), N,
                              M, N, K, int(relu), stream()))
    return out


def layernorm(x, gamma, beta, eps=1e-5):
    _chk(x, gamma, beta)
    out = torch.empty_like(x)
    D = x.shape[-1]
    check(lib().sf_layernorm_f32(ptr(x), ptr(gamma), ptr(beta), ptr(out), x.numel() // D, D, eps, stream()))
    return out


def pack_conv_weight(w):
    """[Cout,Cin,k,k] -> [Cout,k,k,Cin]."""
    _chk(w)
    out = torch.empty(w.shape[0], w.shape[2], w.shape[3], w.shape[1], device=w.device, dtype=torch.float32)
    check(lib().sf_pack_conv_weight_f32(ptr(w), ptr(out), w.shape[0], w.shape[1], w.shape[2], stream()))
    return out


def pack_conv_frag(w_packed):
    """[64,5,5,64] (pack_conv_weight) -> split-bf16 copy in MFMA-fragment order (uint8 buffer) for conv5x5_frag."""
    _chk(w_packed)
    Cout, ks, _, Cin = w_packed.shape
    out = torch.empty(lib().sf_conv_frag_bytes(Cout, Cin, ks), device=w_packed.device, dtype=torch.uint8)
    check(lib().sf_pack_conv_frag_weights(ptr(w_packed), out.data_ptr(), Cout, Cin, ks, stream()))
    return out


def pack_deconv_frag(w_packed):
    """[64,5,5,64] (pack_deconv_weight of a ConvTranspose2d weight) -> consumption-ordered split-bf16 fragments (uint8 buffer) for
    deconv5x5s2_frag / deconv5x5s2_head."""
    _chk(w_packed)
    Cout, ks, _, Cin = w_packed.shape
    out = torch.empty(lib().sf_deconv_frag_bytes(Cout, Cin, ks, 2), device=w_packed.device, dtype=torch.uint8)
    check(lib().sf_pack_deconv_frag_weights(ptr(w_packed), out.data_ptr(), Cout, Cin, ks, 2, stream()))
    return out


def deconv5x5s2_frag(x, w_frag, bias, relu=True):
    """x [R,H,W,64] NHWC, w_frag = pack_deconv_frag(...) -> [R,2H,2W,64]: ConvTranspose2d(64, 64, 5, stride 2, padding 2, output_padding 1)."""
    _chk(x, bias)
    R, H, W, _ = x.shape
    out = torch.empty(R, 2 * H, 2 * W, 64, device=x.device, dtype=torch.float32)
    check(lib().sf_deconv5x5s2_frag_f32(ptr(x), w_frag.data_ptr(), ptr(bias), ptr(out), R, H, W, int(relu), stream()))
    return out


def deconv5x5s2_head(x, w_frag, bias, head_w, head_b):
    """x [R,H,64,64] NHWC -> dec [R, 2H * 128, 4] = head_w [4,64] . relu(deconv(x) + bias) + head_b: the last decoder layer with the 1x1
    output convolution in its epilogue."""
    _chk(x, bias, head_w, head_b)
    R, H, W, _ = x.shape
    dec = torch.empty(R, 4 * H * W, 4, device=x.device, dtype=torch.float32)
    check(lib().sf_deconv5x5s2_head_frag_f32(ptr(x), w_frag.data_ptr(), ptr(bias), ptr(head_w), ptr(head_b), ptr(dec), R, H, W, stream()))
    return dec


def conv5x5_frag(x, w_frag, bias, relu=True, add=None):
    """x [F,H,64,64] NHWC, w_frag = pack_conv_frag(...) -> [F,H,64,64] (4-row tiles, streamed weight fragments)."""
    _chk(x, bias, add)
    F_, H, W, Cin = x.shape
    out = torch.empty(F_, H, W, 64, device=x.device, dtype=torch.float32)
    check(lib().sf_conv5x5_frag_f32(ptr(x), w_frag.data_ptr(), ptr(bias), ptr(add), ptr(out), F_, H, W, int(relu), stream()))
    return out


def conv5x5_ws(x, w_frag, bias, relu=True, add=None, n_workgroups=0):
    """conv5x5_frag with the weights stationary in registers (csrc/conv_ws.hip): the same bits; any H; n_workgroups 0 = one per CU of the stream."""
    _chk(x, bias, add)
    F_, H, W, Cin = x.shape
    out = torch.empty(F_, H, W, 64, device=x.device, dtype=torch.float32)
    check(lib().sf_conv5x5_ws_f32(ptr(x), w_frag.data_ptr(), ptr(bias), ptr(add), ptr(out), F_, H, W, int(relu), int(n_workgroups), stream()))
    return out


def pack_deconv_weight(w):
    """ConvTranspose2d weight [Cin,Cout,k,k] -> [Cout,k,k,Cin]."""
    _chk(w)
    out = torch.empty(w.shape[1], w.shape[2], w.shape[3], w.shape[0], device=w.device, dtype=torch.float32)
    check(lib().sf_pack_deconv_weight_f32(ptr(w), ptr(out), w.shape[0], w.shape[1], w.shape[2], stream()))
    return out


def conv_transpose2d_nhwc(x, w_packed, bias, stride, relu=True):
    """x [F,H,W,Cin] NHWC, w_packed [Cout,k,k,Cin] -> [F,H*s,W*s,Cout] (padding k//2, output_padding s-1)."""
    _chk(x, w_packed, bias)
    F_, H, W, Cin = x.shape
    Cout, ks = w_packed.shape[0], w_packed.shape[1]
    out = torch.empty(F_, H * stride, W * stride, Cout, device=x.device, dtype=torch.float32)
    check(lib().sf_conv_transpose2d_nhwc_f32(ptr(x), ptr(w_packed), ptr(bias), ptr(out), F_, H, W, Cin, Cout, ks, stride,
                                             int(relu), stream()))
    return out


def pos_embed_table(grid, dense_w, dense_b):
    """grid [1,H,W,4] -> [H*W, C]."""
    grid = grid.reshape(-1, 4).contiguous()
    _chk(grid, dense_w, dense_b)
    out = torch.empty(grid.shape[0], dense_w.shape[0], device=grid.device, dtype=torch.float32)
    check(lib().sf_pos_embed_table_f32(ptr(grid), ptr(dense_w), ptr(dense_b), ptr(out), grid.shape[0],
                                       dense_w.shape[0], stream()))
    return out


def conv2d_first(img, weight, bias, stride, relu=True, add=None):
    """img [F,Cin,H,W] NCHW -> [F,Ho,Wo,Cout] NHWC."""
    _chk(img, weight, bias, add)
    F_, Cin, H, W = img.shape
    Cout, ks = weight.shape[0], weight.shape[2]
    Ho = (H + 2 * (ks // 2) - ks) // stride + 1
    Wo = (W + 2 * (ks // 2) - ks) // stride + 1
    out = torch.empty(F_, Ho, Wo, Cout, device=img.device, dtype=torch.float32)
    check(lib().sf_conv2d_nchw_in_f32(ptr(img), Cin * H * W, ptr(weight), ptr(bias), ptr(add), ptr(out), F_, Cin, H, W,
                                      Cout, ks, stride, int(relu), stream()))
    return out


def conv2d_first_clip(clip, weight, bias, stride, relu=True, add=None):
    """clip [B,T,3,H,W] -> [T*B,Ho,Wo,64] NHWC, time-major (frame t * B + b = clip[b, t]): the grouped launch of the batched encode."""
    _chk(clip, weight, bias, add)
    B, T, Cin, H, W = clip.shape
    Cout, ks = weight.shape[0], weight.shape[2]
    Ho = (H + 2 * (ks // 2) - ks) // stride + 1
    Wo = (W + 2 * (ks // 2) - ks) // stride + 1
    out = torch.empty(T * B, Ho, Wo, Cout, device=clip.device, dtype=torch.float32)
    check(lib().sf_conv2d_nchw_in_grouped_f32(ptr(clip), T * Cin * H * W, B, Cin * H * W, ptr(weight), ptr(bias), ptr(add), ptr(out), T * B, Cin,
                                              H, W, Cout, ks, stride, int(relu), stream()))
    return out


def pixel_feat(x, ln0, fc1, fc2, ln1, form=3, eps=1e-5):
    """x [M,64] -> LN(fc2(relu(fc1(LN(x))))): [M,128] float32 (form 0 .. 3), or [M,256] bfloat16 rows hi | lo (form 4).  ln = (gamma, beta),
    fc = (weight, bias) in torch layout."""
    _chk(x, *ln0, *fc1, *fc2, *ln1)
    M = x.shape[0]
    out = torch.empty(M, 256, device=x.device, dtype=torch.bfloat16) if form == 4 else torch.empty(M, 128, device=x.device, dtype=torch.float32)
    check(lib().sf_pixel_feat_f32(ptr(x), ptr(ln0[0]), ptr(ln0[1]), ptr(fc1[0]), ptr(fc1[1]), ptr(fc2[0]), ptr(fc2[1]), ptr(ln1[0]), ptr(ln1[1]),
                                  out.data_ptr(), M, eps, form, stream()))
    return out


def conv2d_nhwc(x, w_packed, bias, relu=True, add=None):
    """x [F,H,W,Cin] NHWC, w_packed [Cout,k,k,Cin] -> [F,H,W,Cout]."""
    _chk(x, w_packed, bias, add)
    F_, H, W, Cin = x.shape
    Cout, ks = w_packed.shape[0], w_packed.shape[1]
    out = torch.empty(F_, H, W, Cout, device=x.device, dtype=torch.float32)
    check(lib().sf_conv2d_nhwc_f32(ptr(x), ptr(w_packed), ptr(bias), ptr(add), ptr(out), F_, H, W, Cin, Cout, ks,
                                   int(relu), stream()))
    return out


def conv_wgrad(a, x, stride=1, partial=None):
    """a [F,H,W,CA], x [F,H*s,W*s,64] NHWC -> dW [CA,64,5,5]: the weight gradient of a 5x5 "same" convolution (a = dY, x = its input, s = 1) or
    of a transposed convolution (a = its input, x = dY on the finer grid).  partial: scratch (float32, any size the call's splits fit in)."""
    _chk(a, x, partial)
    F_, H, W, CA = a.shape
    _, Hx, Wx, _ = x.shape
    if partial is None:
        partial = torch.empty(lib().sf_conv_wgrad_partial_floats(CA, 5), device=a.device, dtype=torch.float32)
    out = torch.empty(CA, 64, 5, 5, device=a.device, dtype=torch.float32)
    check(lib().sf_conv_wgrad_f32(ptr(a), CA, F_, H, W, ptr(x), Hx, Wx, int(stride), 5, F_ * H * W, ptr(out), ptr(partial), partial.numel(), stream()))
    return out


def pack_conv_bwd_weight(w):
    """Conv2d weight [Cout,Cin,k,k] -> [Cin,k,k,Cout], flipped: the packed weight of its backward-data convolution."""
    _chk(w)
    out = torch.empty(w.shape[1], w.shape[2], w.shape[3], w.shape[0], device=w.device, dtype=torch.float32)
    check(lib().sf_pack_conv_bwd_weight_f32(ptr(w), ptr(out), w.shape[0], w.shape[1], w.shape[2], stream()))
    return out


def conv2d_nhwc_bwd_data(g, w_packed, stride=1, relu_mask=None):
    """g [F,H,W,Cin] NHWC, w_packed [Cout,k,k,Cin] -> [F,H/s,W/s,Cout] = Conv2d(k, s, padding k//2)(g), zero where relu_mask <= 0."""
    _chk(g, w_packed, relu_mask)
    F_, H, W, Cin = g.shape
    Cout, ks = w_packed.shape[0], w_packed.shape[1]
    out = torch.empty(F_, H // stride, W // stride, Cout, device=g.device, dtype=torch.float32)
    check(lib().sf_conv2d_nhwc_bwd_data_f32(ptr(g), ptr(w_packed), ptr(relu_mask), ptr(out), F_, H, W, Cin, Cout, ks, int(stride), stream()))
    return out


def conv_first_wgrad(img, dy, frame_stride=None):
    """img [F,3,R,R] NCHW (R 64 or 128), dy [F*4096,64] -> dW [64,3,5,5] of the encoder's first convolution."""
    _chk(img, dy)
    F_, res = img.shape[0], img.shape[-1]
    ws = scratch(lib().sf_conv_first_wgrad_workspace_bytes, F_, device=img.device, at_least=16)
    out = torch.empty(64, 3, 5, 5, device=img.device, dtype=torch.float32)
    check(lib().sf_conv_first_wgrad_f32(ptr(img), int(frame_stride or 3 * res * res), res, ptr(dy), F_, ptr(out), ws.data_ptr(), ws.numel(),
                                        stream()))
    return out


def pos_dense_grad(d, grid):
    """d [F,HW,C], grid [HW,4] -> (dw [C,4], db [C], frame sum of d [HW,C])."""
    _chk(d, grid)
    F_, HW, C_ = d.shape
    dw, db = torch.empty(C_, 4, device=d.device), torch.empty(C_, device=d.device)
    dtab = torch.empty(HW, C_, device=d.device)
    check(lib().sf_pos_dense_grad_f32(ptr(d), F_, HW, C_, ptr(grid), ptr(dw), ptr(db), ptr(dtab), stream()))
    return dw, db, dtab


def savi_decode_head_bwd(dec, d_recon, act, out_w, want_param_grads=True):
    """dec [F,N,HW,4], d_recon [F,3,HW], act [F*N*HW,Cl], out_w [4,Cl] -> (d_dec, d_act, d_out_w | None, d_out_b | None)."""
    _chk(dec, d_recon, act, out_w)
    F_, N, HW, _ = dec.shape
    Cl = out_w.shape[1]
    d_dec, d_act = torch.empty_like(dec), torch.empty_like(act)
    gw = torch.empty(4, Cl, device=dec.device) if want_param_grads else None
    gb = torch.empty(4, device=dec.device) if want_param_grads else None
    ws = scratch(lib().sf_savi_decode_head_bwd_workspace_bytes, Cl, device=dec.device, at_least=16)
    check(lib().sf_savi_decode_head_bwd_f32(ptr(dec), ptr(d_recon), ptr(act), ptr(out_w), ptr(d_dec), ptr(d_act), ptr(gw), ptr(gb), F_, N, HW, Cl,
                                            ws.data_ptr(), ws.numel(), stream()))
    return d_dec, d_act, gw, gb


def slot_attn_iter(k, v, q, eps=1e-6, want_attn=False):
    """k, v [B,HW,D]; q [B,N,D] -> (part_num [B,P,N,D], part_den [B,P,N], attn [B,N,HW] | None)."""
    _chk(k, v, q)
    B, HW, D = k.shape
    N = q.shape[1]
    P = lib().sf_slot_attn_num_partials(HW)
    pn = torch.empty(B, P, N, D, device=k.device, dtype=torch.float32)
    pd = torch.empty(B, P, N, device=k.device, dtype=torch.float32)
    attn = torch.empty(B, N, HW, device=k.device, dtype=torch.float32) if want_attn else None
    check(lib().sf_slot_attn_iter_f32(ptr(k), ptr(v), D, HW * D, ptr(q), ptr(pn), ptr(pd), ptr(attn), B, HW, N, D,
                                      float(D)**-0.5, eps, stream()))
    return pn, pd, attn


def slot_attn_iter_planes(planes, q, eps=1e-6, want_attn=False):
    """slot_attn_iter for keys == values kept as planes [B,HW,256] bfloat16 (hi | lo of 128 channels; pixel_feat form 4); q [B,N,128]."""
    _chk(q)
    if not (planes.is_cuda and planes.dtype == torch.bfloat16 and planes.is_contiguous() and planes.shape[-1] == 256):
        raise RuntimeError('slot_attn_iter_planes needs contiguous bfloat16 rows [B, HW, 256] on a HIP device')
    B, HW, _ = planes.shape
    N, P = q.shape[1], HW // 256
    pn = torch.empty(B, P, N, 128, device=q.device, dtype=torch.float32)
    pd = torch.empty(B, P, N, device=q.device, dtype=torch.float32)
    attn = torch.empty(B, N, HW, device=q.device, dtype=torch.float32) if want_attn else None
    check(lib().sf_slot_attn_iter_planes_f32(planes.data_ptr(), HW, ptr(q), ptr(pn), ptr(pd), ptr(attn), N * HW, B, HW, N, 128.0**-0.5, eps,
                                             stream()))
    return pn, pd, attn


def slot_prologue(prev, init, pm, kd, q, noise=None, norm_first=True, want_kdist=False, B=None, ln_eps=1e-5):
    """The slots of a time step before its first iteration.  prev [B,N,D] or None (then B videos start from init [N,D]); pm = (ln_g, ln_b, w0, b0, w2,
    b2) of the residual-MLP predictor or None, kd = (w, b) of the kernel-distribution Linear, q = (ln_g, ln_b, w) of project_q, all in torch layout
    (transposed here); noise [B,N,D] or None -> (slots [B,N,D], q [B,N,D], kernel_dist [B,N,2D] | None)."""
    pm = pm or (None, ) * 6
    _chk(prev, init, *pm, *kd, *q, noise)
    N, D = init.shape
    B = prev.shape[0] if prev is not None else B
    t = lambda w: None if w is None else w.t().contiguous()   # noqa: E731
    w0_t, w2_t, kd_t, q_t = t(pm[2]), t(pm[4]), t(kd[0]), t(q[2])
    slots, q_out = torch.empty(B, N, D, device=init.device), torch.empty(B, N, D, device=init.device)
    kdist = torch.empty(B, N, 2 * D, device=init.device) if want_kdist else None
    check(lib().sf_slot_prologue_f32(ptr(prev), ptr(init), ptr(pm[0]), ptr(pm[1]), ptr(w0_t), ptr(pm[3]), ptr(w2_t), ptr(pm[5]), int(norm_first), ptr(kd_t),
                                     ptr(kd[1]), ptr(noise), N * D, ptr(kdist), N * 2 * D, ptr(q[0]), ptr(q[1]), ptr(q_t), ptr(slots), ptr(q_out), B, N, D,
                                     ln_eps, stream()))
    return slots, q_out, kdist


def slot_attn_iter_bwd(k, v, q, pn, pd, d_updates, dk=None, dv=None, eps=1e-6):
    """Backward of slot_attn_iter: gradient d_updates [B,N,D] of updates = sum(pn) / sum(pd) -> (dq, dk, dv).  Passing
    dk / dv accumulates into them (the iterations of a frame share k and v)."""
    _chk(k, v, q, pn, pd, d_updates)
    B, HW, D = k.shape
    N, P = q.shape[1], pn.shape[1]
    acc = dk is not None
    if not acc:
        dk, dv = torch.empty_like(k), torch.empty_like(v)
    dq = torch.empty_like(q)
    # N <= 8: the 8-slot entry point; 9 .. 16 slots: the two-launch form behind its own entry point
    ws_bytes, bwd = ((lib().sf_slot_attn_iter_bwd_workspace_bytes, lib().sf_slot_attn_iter_bwd_f32) if N <= 8 else
                     (lib().sf_slot_attn_iter_bwd16_workspace_bytes, lib().sf_slot_attn_iter_bwd16_f32))
    ws = scratch(ws_bytes, B, HW, N, D, device=k.device)
    check(bwd(ptr(k), ptr(v), D, HW * D, ptr(q), ptr(pn), ptr(pd), P, ptr(d_updates), ptr(dk), ptr(dv),
              int(acc), ptr(dq), B, HW, N, D, float(D)**-0.5, eps, ws.data_ptr(), ws.numel(), stream()))
    return dq, dk, dv


def slot_update(pn, pd, slots_prev, gru, ln_g, ln_b, w1, b1, w2, b2, ln_eps=1e-5):
    """gru = (w_ih, w_hh, b_ih, b_hh); all weights in torch layout (transposed here for the kernel)."""
    _chk(pn, pd, slots_prev, *gru, ln_g, ln_b, w1, b1, w2, b2)
    B, P, N, D = pn.shape
    out = torch.empty_like(slots_prev)
    w_ih_t, w_hh_t, w1_t, w2_t = (w.t().contiguous() for w in (gru[0], gru[1], w1, w2))
    check(lib().sf_slot_update_f32(ptr(pn), ptr(pd), P, ptr(slots_prev), ptr(w_ih_t), ptr(w_hh_t), ptr(gru[2]),
                                   ptr(gru[3]), ptr(ln_g), ptr(ln_b), ptr(w1_t), ptr(b1), ptr(w2_t), ptr(b2), ptr(out),
                                   B, N, D, w1.shape[0], ln_eps, stream()))
    return out


def pack_linear(w):
    """torch-layout weight [N, K] -> fragment-ordered split-bf16 copy (sf_pack_linear_weights)."""
    _chk(w)
    n, k = w.shape
    buf = torch.empty(lib().sf_packed_linear_bytes(n, k), dtype=torch.uint8, device=w.device)
    check(lib().sf_pack_linear_weights(ptr(w.contiguous()), buf.data_ptr(), n, k, stream()))
    return buf


def slot_update_packed(pn, pd, slots_prev, gru, ln_g, ln_b, w1, b1, w2, b2, q=None, ln_eps=1e-5):
    """slot_update on the matrix cores (slot size 128, MLP 256); q = (q_ln_g, q_ln_b, q_w) also returns project_q(out)."""
    _chk(pn, pd, slots_prev, *gru, ln_g, ln_b, w1, b1, w2, b2)
    B, P, N, D = pn.shape
    out = torch.empty_like(slots_prev)
    packed = [pack_linear(w) for w in (gru[0], gru[1], w1, w2)]
    q_out = torch.empty_like(slots_prev) if q is not None else None
    qp = pack_linear(q[2]) if q is not None else None
    check(lib().sf_slot_update_packed_f32(ptr(pn), ptr(pd), P, ptr(slots_prev), packed[0].data_ptr(), packed[1].data_ptr(), ptr(gru[2]),
                                          ptr(gru[3]), ptr(ln_g), ptr(ln_b), packed[2].data_ptr(), ptr(b1), packed[3].data_ptr(), ptr(b2),
                                          ptr(out), ptr(q[0]) if q is not None else None, ptr(q[1]) if q is not None else None,
                                          ptr(qp), ptr(q_out), B, N, D, w1.shape[0], ln_eps, stream()))
    return (out, q_out) if q is not None else out


def slot_update_packed_next(pn, pd, slots_prev, gru, ln_g, ln_b, w1, b1, w2, b2, q, pm, kd, noise=None, norm_first=True, want_kdist=False,
                            p_step=1, ln_eps=1e-5):
    """slot_update_packed followed, in the same launch, by the slot prologue of the next time step (slot_prologue's pm / kd in torch layout, packed
    here) -> (slots_out, next_slots, q of next_slots, kernel_dist | None); only every p_step-th partial record is read."""
    _chk(pn, pd, slots_prev, *gru, ln_g, ln_b, w1, b1, w2, b2, *q, *pm, *kd, noise)
    B, P, N, D = pn.shape
    out, nxt, q_out = torch.empty_like(slots_prev), torch.empty_like(slots_prev), torch.empty_like(slots_prev)
    kdist = torch.empty(B, N, 2 * D, device=pn.device) if want_kdist else None
    pk = [pack_linear(w) for w in (gru[0], gru[1], w1, w2, q[2], pm[2], pm[4], kd[0])]
    check(lib().sf_slot_update_packed_next_f32(ptr(pn), ptr(pd), P, ptr(slots_prev), pk[0].data_ptr(), pk[1].data_ptr(), ptr(gru[2]), ptr(gru[3]), ptr(ln_g),
                                               ptr(ln_b), pk[2].data_ptr(), ptr(b1), pk[3].data_ptr(), ptr(b2), ptr(out), ptr(q[0]), ptr(q[1]),
                                               pk[4].data_ptr(), ptr(q_out), B, N, D, w1.shape[0], ln_eps, None, 0, p_step, ptr(pm[0]), ptr(pm[1]),
                                               pk[5].data_ptr(), ptr(pm[3]), pk[6].data_ptr(), ptr(pm[5]), int(norm_first), pk[7].data_ptr(),
                                               ptr(kd[1]), ptr(noise), N * D, ptr(kdist), N * 2 * D, ptr(nxt), stream()))
    return out, nxt, q_out, kdist


def mha(qkv, B, L, d_model, num_heads, Lq=None):
    """qkv [B*L, 3d] -> [B*Lq, d]."""
    _chk(qkv)
    Lq = L if Lq is None else Lq
    out = torch.empty(B * Lq, d_model, device=qkv.device, dtype=torch.float32)
    check(lib().sf_mha_f32(ptr(qkv), ptr(out), B, L, Lq, d_model, num_heads, stream()))
    return out


def qkv_attention(x, in_proj_w, in_proj_b, B, L, num_heads, ln=None, Lq=None, ln_eps=1e-5):
    """Fused LN? -> q|k|v projection -> attention;  x [B*L, d] -> [B*Lq, d] (before out_proj)."""
    _chk(x, in_proj_w, in_proj_b, *(ln or ()))
    d = x.shape[-1]
    Lq = L if Lq is None else Lq
    out = torch.empty(B * Lq, d, device=x.device, dtype=torch.float32)
    g, b = ln if ln is not None else (None, None)
    check(lib().sf_qkv_attention_f32(ptr(x), ptr(g), ptr(b), ln_eps, ptr(in_proj_w), ptr(in_proj_b), ptr(out), B, L, Lq, d,
                                     num_heads, stream()))
    return out


def lstm_pointwise(gates, c_prev):
    _chk(gates, c_prev)
    R, H4 = gates.shape
    h = torch.empty(R, H4 // 4, device=gates.device, dtype=torch.float32)
    c = torch.empty_like(h)
    check(lib().sf_lstm_pointwise_f32(ptr(gates), ptr(c_prev), ptr(h), ptr(c), R, H4 // 4, stream()))
    return h, c


def sample_dist(dist, noise=None):
    _chk(dist, noise)
    D = dist.shape[-1] // 2
    out = torch.empty(*dist.shape[:-1], D, device=dist.device, dtype=torch.float32)
    check(lib().sf_sample_dist_f32(ptr(dist), ptr(noise), ptr(out), dist.numel() // (2 * D), D, stream()))
    return out


def bilinear_resize(x, size):
    """x [..., Hi, Wi] -> [..., Ho, Wo]  (F.interpolate bilinear, align_corners=False)."""
    _chk(x)
    Hi, Wi = x.shape[-2:]
    out = torch.empty(*x.shape[:-2], size[0], size[1], device=x.device, dtype=torch.float32)
    check(lib().sf_bilinear_resize_f32(ptr(x), ptr(out), x.numel() // (Hi * Wi), Hi, Wi, size[0], size[1],
                                       stream()))
    return out


def groupnorm1_nhwc(x, gamma, beta, eps=1e-5, relu=True, pixel_shuffle=1):
    """F.group_norm(x, 1, gamma, beta) (+ReLU) on NHWC x [F,H,W,C]; pixel_shuffle=2 also applies nn.PixelShuffle(2)
    (-> [F,2H,2W,C/4]).  steve_utils.py:124-126, dVAE.py:44,49."""
    _chk(x, gamma, beta)
    F_, H, W, C_ = x.shape
    r = pixel_shuffle
    out = torch.empty(F_, H * r, W * r, C_ // (r * r), device=x.device, dtype=torch.float32)
    ws = scratch(lib().sf_groupnorm1_workspace_bytes, F_, device=x.device, empty_ok=F_ == 0, at_least=8)   # (no frames: an empty batch, which is taken)
    check(lib().sf_groupnorm1_nhwc_f32(ptr(x), ptr(gamma), ptr(beta), ptr(out), F_, H, W, C_, eps, int(relu), r, ws.data_ptr(), ws.numel(),
                                       stream()))
    return out


def slate_attention(q, k, v, num_heads, causal, q_off=0, k_off=0, v_off=0, d_model=None):
    """softmax(q k^T hd^-0.5 [causal]) v per head (steve_transformer.py:12-55).  q [B,Lq,ldq], k/v [B,Lk,ld*]: the head
    block starts at column *_off of each row (so q|k|v may live side by side in one projection buffer)."""
    _chk(q, k, v)
    B, Lq, ldq = q.shape
    Lk, ldk, ldv = k.shape[1], k.shape[2], v.shape[2]
    d = d_model if d_model is not None else ldq
    out = torch.empty(B, Lq, d, device=q.device, dtype=torch.float32)
    check(lib().sf_slate_attention_f32(q.data_ptr() + 4 * q_off, k.data_ptr() + 4 * k_off, v.data_ptr() + 4 * v_off, ptr(out),
                                       ldq, ldk, ldv, d, B, Lq, Lk, num_heads, d // num_heads, int(causal), stream()))
    return out


def slate_attention_bwd(q, k, v, out, d_out, num_heads, causal):
    """Adjoint of slate_attention for contiguous q [B,Lq,d], k, v [B,Lk,d]: (dq, dk, dv)."""
    _chk(q, k, v, out, d_out)
    B, Lq, d = q.shape
    Lk = k.shape[1]
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws = scratch(lib().sf_slate_attention_bwd_workspace_bytes, B, Lq, num_heads, device=q.device)
    check(lib().sf_slate_attention_bwd_f32(ptr(q), ptr(k), ptr(v), ptr(out), ptr(d_out), ptr(dq), ptr(dk), ptr(dv), d, d, d, d, Lq * d, Lk * d,
                                           Lk * d, Lq * d, B, Lq, Lk, num_heads, d // num_heads, int(causal), ws.data_ptr(), ws.numel(), stream()))
    return dq, dk, dv


def embed_tokens(idx, tok_emb, pos):
    """tok_emb[idx] + pos[:L];  idx int64 [B,L] on device."""
    _chk(tok_emb, pos)
    if idx.dtype != torch.int64 or not idx.is_cuda or not idx.is_contiguous():
        raise TypeError('embed_tokens: idx must be a contiguous int64 device tensor')
    B, L = idx.shape
    d = tok_emb.shape[1]
    out = torch.empty(B, L, d, device=tok_emb.device, dtype=torch.float32)
    check(lib().sf_embed_tokens_f32(idx.data_ptr(), ptr(tok_emb), ptr(pos), ptr(out), B, L, d, stream()))
    return out


def argmax_rows(x):
    """First index of the maximum of each row of x [..., V] -> int64 [...]."""
    _chk(x)
    V = x.shape[-1]
    R = x.numel() // V
    out = torch.empty(x.shape[:-1], device=x.device, dtype=torch.int64)
    check(lib().sf_argmax_rows_f32(ptr(x), V, out.data_ptr(), R, V, stream()))
    return out


def dvae_tokens_ok(V, K, C, H, W):
    """Whether patch_embed / linear_argmax take these shapes (`sf_dvae_tokens_ok`; shapes only, no device needed)."""
    return bool(lib().sf_dvae_tokens_ok(int(V), int(K), int(C), int(H), int(W)))


def patch_embed(imgs, weight):
    """imgs [F,3,H,W] NCHW, weight [64,3,4,4] -> [F,H/4,W/4,64] NHWC: the bias-free 4x4 / stride-4 convolution of the dVAE's first block, read
    straight from the frames (`sf_dvae_patch_embed_f32`, split-bf16 whatever the library's precision mode)."""
    _chk(imgs, weight)
    F_, C_, H, W = imgs.shape
    out = torch.empty(F_, H // 4, W // 4, 64, device=imgs.device, dtype=torch.float32)
    check(lib().sf_dvae_patch_embed_f32(ptr(imgs), ptr(weight), ptr(out), F_, C_, H, W, stream()))
    return out


def pack_head_weight(w):
    """[V,64] -> the split-bf16 fragment-order copy `linear_argmax` streams (uint8 buffer, `sf_dvae_pack_head_weights`)."""
    _chk(w)
    V, K = w.shape
    nb = lib().sf_dvae_head_packed_bytes(V, K)
    if nb == 0:
        raise RuntimeError(f'slotformer_amd pack_head_weight: K must be 64 and V a multiple of 32, got [{V}, {K}]')
    out = torch.empty(nb, device=w.device, dtype=torch.uint8)
    check(lib().sf_dvae_pack_head_weights(ptr(w), out.data_ptr(), V, K, stream()))
    return out


def linear_argmax(x, w_packed, bias, V, out=None, out_i16=None):
    """First index of the maximum of each row of x @ W.T + bias WITHOUT the product in memory (`sf_dvae_head_argmax_f32`).  x [..., 64] (rows may
    be strided: a 2-D x with stride(1) == 1), w_packed = pack_head_weight(W [V,64]), bias [V] or None.  Returns int64 ids [...] by default; out
    (int64) / out_i16 (int16) are contiguous device tensors of x's leading shape to write into -- give either or both, and what was given is
    returned (a tuple for both)."""
    strided = torch.is_tensor(x) and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) > x.shape[1]
    _chk(x[:1] if strided else x, bias)
    if not (torch.is_tensor(w_packed) and w_packed.is_cuda and w_packed.dtype == torch.uint8 and w_packed.is_contiguous()):
        raise RuntimeError('linear_argmax: w_packed is the uint8 device buffer of pack_head_weight; there is no CPU fallback')
    K = x.shape[-1]
    ld = x.stride(0) if strided else K
    lead = tuple(x.shape[:-1])
    R = x.numel() // K
    if out is None and out_i16 is None:
        out = torch.empty(lead, device=x.device, dtype=torch.int64)
    for t, dt in ((out, torch.int64), (out_i16, torch.int16)):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == R):
            raise TypeError(f'linear_argmax: outputs must be contiguous {dt} device tensors of {R} elements')
    check(lib().sf_dvae_head_argmax_f32(x.data_ptr(), ld, w_packed.data_ptr(), ptr(bias), ptr(out), ptr(out_i16), R, int(V), K, stream()))
    return out if out_i16 is None else out_i16 if out is None else (out, out_i16)


def gather_rows(table, ids):
    """table[ids]: table [rows, d] float32, ids int64 [...] on the device -> [..., d] (`sf_gather_rows_f32`)."""
    _chk(table)
    if ids.dtype != torch.int64 or not ids.is_cuda or not ids.is_contiguous():
        raise TypeError('gather_rows: ids must be a contiguous int64 device tensor')
    rows, d = table.shape
    out = torch.empty(tuple(ids.shape) + (d, ), device=table.device, dtype=torch.float32)
    check(lib().sf_gather_rows_f32(ptr(table), ids.data_ptr(), ptr(out), ids.numel(), d, rows, stream()))
    return out


def pack_head_ce_weight(w):
    """[V,K] -> the two split-bf16 fragment-order copies `head_ce_forward` / `head_ce_backward` stream (uint8 buffer, `sf_head_ce_pack_weights`)."""
    _chk(w)
    V, K = w.shape
    nb = lib().sf_head_ce_packed_bytes(V, K)
    if nb == 0:
        raise RuntimeError(f'slotformer_amd pack_head_ce_weight: K a multiple of 32 in [32, 256] and V a multiple of 32 in [32, 2^20], got [{V}, {K}]')
    out = torch.empty(nb, device=w.device, dtype=torch.uint8)
    check(lib().sf_head_ce_pack_weights(ptr(w), out.data_ptr(), V, K, stream()))
    return out


def _head_ce_args(x, w_packed, target, group_w, group, V):
    """Checks shared by the two head_ce launches -> (ld, R, K, target_i64 pointer, target_i16 pointer)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1]):
        raise RuntimeError('slotformer_amd head_ce: x is a float32 [R, K] device tensor with unit column stride; there is no CPU fallback')
    if not (torch.is_tensor(w_packed) and w_packed.is_cuda and w_packed.dtype == torch.uint8 and w_packed.is_contiguous()):
        raise RuntimeError('slotformer_amd head_ce: w_packed is the uint8 device buffer of pack_head_ce_weight; there is no CPU fallback')
    R, K = x.shape
    if w_packed.numel() != lib().sf_head_ce_packed_bytes(int(V), K) or w_packed.numel() == 0:
        raise ValueError(f'slotformer_amd head_ce: w_packed does not hold a [{V}, {K}] head')
    if not (torch.is_tensor(target) and target.is_cuda and target.dtype in (torch.int64, torch.int16) and target.is_contiguous()
            and target.numel() == R):
        raise TypeError(f'slotformer_amd head_ce: target is a contiguous int64 or int16 device tensor of {R} elements')
    group = int(group)
    if group < 1 or R % group:
        raise ValueError(f'slotformer_amd head_ce: group {group} does not divide {R} rows')
    if group_w is not None:
        _chk(group_w)
        if group_w.numel() != R // group:
            raise ValueError(f'slotformer_amd head_ce: group_w has {group_w.numel()} elements for {R // group} groups')
    i64 = target.dtype == torch.int64
    return x.stride(0), R, K, target.data_ptr() if i64 else None, None if i64 else target.data_ptr()


def head_ce_forward(x, w_packed, target, V, group_w=None, group=1, stats=None, want_rows=True):
    """lse[r] = logsumexp_v(W[v] . x[r]) and loss[r] = lse[r] - W[target[r]] . x[r] WITHOUT the logits in memory (`sf_head_ce_fwd_f32`).
    x [R, K] (rows may be strided), w_packed = pack_head_ce_weight(W [V,K]), target int64 / int16 [R]; group_w [R / group] weighs runs of `group`
    rows.  stats: float64 [2] on the device, has (sum w loss, sum w) ADDED to it.  -> (lse [R], loss_rows [R], or None with want_rows=False)."""
    ld, R, K, t64, t16 = _head_ce_args(x, w_packed, target, group_w, group, V)
    lse = torch.empty(R, device=x.device, dtype=torch.float32)
    rows = torch.empty(R, device=x.device, dtype=torch.float32) if want_rows else None
    ws = None
    if stats is not None:
        if not (stats.is_cuda and stats.dtype == torch.float64 and stats.numel() == 2 and stats.is_contiguous()):
            raise TypeError('slotformer_amd head_ce: stats is a contiguous float64 [2] device tensor')
        ws = scratch(lib().sf_head_ce_workspace_bytes, R, device=x.device)
    check(lib().sf_head_ce_fwd_f32(x.data_ptr(), ld, w_packed.data_ptr(), t64, t16, ptr(group_w), int(group), ptr(lse), ptr(rows), ptr(stats), R, int(V), K,
                                   ptr(ws), 0 if ws is None else ws.numel(), stream()))
    return lse, rows


def head_ce_backward(x, w_packed, target, V, lse, g, group_w=None, group=1, out=None):
    """dx[r] = g * w(r) * (softmax(W x[r]) - onehot(target[r])) @ W, the logits recomputed from x and `lse` (`sf_head_ce_bwd_f32`).  g: a float32
    device tensor of one element (never read on the host).  out: float32 [R, K] with unit column stride to write into."""
    ld, R, K, t64, t16 = _head_ce_args(x, w_packed, target, group_w, group, V)
    _chk(lse, g)
    if lse.numel() != R or g.numel() != 1:
        raise ValueError(f'slotformer_amd head_ce: lse has {R} elements and g one')
    if out is None:
        out = torch.empty(R, K, device=x.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (R, K) and out.stride(1) == 1 and out.stride(0) >= K):
        raise TypeError(f'slotformer_amd head_ce: out is a float32 [{R}, {K}] device tensor with unit column stride')
    check(lib().sf_head_ce_bwd_f32(x.data_ptr(), ld, w_packed.data_ptr(), t64, t16, ptr(group_w), int(group), ptr(lse), ptr(g), out.data_ptr(),
                                   out.stride(0), R, int(V), K, stream()))
    return out


def head_ce_wgrad(x, w_packed, target, V, lse, g, group_w=None, group=1, out=None):
    """dW[v] = sum_r g * w(r) * (softmax(W x[r])[v] - [v == target[r]]) x[r], the head's own gradient with the logits recomputed from x and `lse`
    (`sf_head_ce_wgrad_f32`); arguments as for `head_ce_backward`.  out: float32 [V, K] with unit column stride, OVERWRITTEN.  The workspace holds
    at most eight [V, K] blocks, whatever R is."""
    ld, R, K, t64, t16 = _head_ce_args(x, w_packed, target, group_w, group, V)
    _chk(lse, g)
    if lse.numel() != R or g.numel() != 1:
        raise ValueError(f'slotformer_amd head_ce: lse has {R} elements and g one')
    V = int(V)
    if out is None:
        out = torch.empty(V, K, device=x.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (V, K) and out.stride(1) == 1 and out.stride(0) >= K):
        raise TypeError(f'slotformer_amd head_ce: out is a float32 [{V}, {K}] device tensor with unit column stride')
    ws = scratch(lib().sf_head_ce_wgrad_workspace_bytes, R, V, K, device=x.device)
    check(lib().sf_head_ce_wgrad_f32(x.data_ptr(), ld, w_packed.data_ptr(), t64, t16, ptr(group_w), ptr(lse), ptr(g), out.data_ptr(), out.stride(0),
                                     R, V, K, int(group), ws.data_ptr(), ws.numel(), stream()))
    return out


def cross_entropy(logits, target):
    """F.cross_entropy(logits [R,V], target int64 [R]) with mean reduction -> 0-dim tensor."""
    _chk(logits)
    if target.dtype != torch.int64 or not target.is_cuda or not target.is_contiguous():
        raise TypeError('cross_entropy: target must be a contiguous int64 device tensor')
    R, V = logits.shape
    rows = torch.empty(R, device=logits.device, dtype=torch.float32)
    mean = torch.empty(1, device=logits.device, dtype=torch.float32)
    check(lib().sf_cross_entropy_f32(ptr(logits), target.data_ptr(), ptr(rows), ptr(mean), R, V, stream()))
    return mean[0]


def softmax_rows(x, add=None, scale=1.0):
    """softmax((x + add) * scale) over the last dim."""
    _chk(x, add)
    V = x.shape[-1]
    out = torch.empty_like(x)
    check(lib().sf_softmax_rows_f32(ptr(x), ptr(add), float(scale), ptr(out), x.numel() // V, V, stream()))
    return out


def log_softmax_rows(x):
    """F.log_softmax over the last dim."""
    _chk(x)
    V = x.shape[-1]
    out = torch.empty_like(x)
    check(lib().sf_log_softmax_rows_f32(ptr(x), ptr(out), x.numel() // V, V, stream()))
    return out


def gumbel_softmax_rows(x, seed, scale=1.0):
    """softmax((x + g) * scale) over the last dim with Gumbel(0, 1) noise g generated inside the kernel from `seed`
    (train.gumbel_noise rebuilds it on the host)."""
    _chk(x)
    V = x.shape[-1]
    out = torch.empty_like(x)
    check(lib().sf_gumbel_softmax_rows_f32(ptr(x), int(seed) & 0xffffffffffffffff, float(scale), ptr(out), x.numel() // V, V, stream()))
    return out


_U64 = 0xffffffffffffffff
_KERNEL_SAMPLE_WS = {}


def normal_noise(seed, tag, shape, device=None):
    """sf_normal_noise_f32: standard-normal noise as a pure function of (seed, tag, flat element index) -> float32 `shape` (an int or a
    tuple) on `device` (default: the current HIP device).  train.normal_noise rebuilds it on the host."""
    shape = (int(shape), ) if not hasattr(shape, '__len__') else tuple(int(s) for s in shape)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('slotformer_amd: normal_noise is generated on a HIP device; there is no CPU fallback (train.normal_noise is the host twin)')
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    check(lib().sf_normal_noise_f32(ptr(out), out.numel(), int(seed) & _U64, int(tag) & 0xffffffff, stream(out)))
    return out


def _kernel_sample_ws(device, R, D):
    """The forward's workspace, one per device: zero-filled once; every launch leaves its arrival counter at zero (as train._clip_mse_ws)."""
    old = _KERNEL_SAMPLE_WS.get(device)
    ws = scratch(lib().sf_kernel_sample_workspace_bytes, R, D, device=device, reuse=old, at_least=4096)
    if ws is not old:
        _KERNEL_SAMPLE_WS[device] = ws.zero_()
    return ws


def _kernel_sample_args(dist, noise, seed, D):
    _chk(dist, noise)
    D = int(D)
    if dist.dim() < 1 or dist.shape[-1] != 2 * D:
        raise ValueError(f'slotformer_amd: kernel_sample takes dist [..., {2 * D}] = (mu | log_var), got {tuple(dist.shape)}')
    R = dist.numel() // (2 * D)
    if noise is not None and noise.numel() != R * D:
        raise ValueError(f'slotformer_amd: kernel_sample noise has {R * D} elements, got {tuple(noise.shape)}')
    if noise is None and seed is None:
        raise ValueError('slotformer_amd: kernel_sample needs noise= or seed=')
    return R, D


def kernel_sample_fwd(dist, D, prior_log_var, kld_sum, noise=None, seed=None, tag=0):
    """sf_kernel_sample_fwd_f32: dist [..., 2 D] -> kernels [..., D] = mu + eps * exp(log_var / 2); the KL sum against the prior of log-variance
    `prior_log_var` is ADDED to kld_sum (float64 [1] on the device).  eps: `noise` (kernels' shape), else generated from (seed, tag)."""
    R, D = _kernel_sample_args(dist, noise, seed, D)
    if not (torch.is_tensor(kld_sum) and kld_sum.is_cuda and kld_sum.dtype == torch.float64 and kld_sum.numel() == 1):
        raise ValueError('slotformer_amd: kernel_sample adds the KL sum to a float64 [1] device tensor')
    out = torch.empty(*dist.shape[:-1], D, dtype=torch.float32, device=dist.device)
    ws = _kernel_sample_ws(dist.device, R, D)
    check(lib().sf_kernel_sample_fwd_f32(ptr(dist), ptr(noise), int(seed or 0) & _U64, int(tag) & 0xffffffff, float(prior_log_var), ptr(out),
                                         kld_sum.data_ptr(), R, D, ws.data_ptr(), ws.numel(), stream(dist)))
    return out


def kernel_sample_bwd(dist, D, prior_log_var, d_kernels, d_kld, kld_scale, noise=None, seed=None, tag=0):
    """sf_kernel_sample_bwd_f32 -> d_dist, dist's shape.  d_kernels: kernels' shape or None (zero); d_kld: float32 [1] on the device, the gradient
    at the mean KL term; kld_scale: 1 / rows of that mean."""
    R, D = _kernel_sample_args(dist, noise, seed, D)
    _chk(d_kernels, d_kld)
    if d_kernels is not None and d_kernels.numel() != R * D:
        raise ValueError(f'slotformer_amd: kernel_sample d_kernels has {R * D} elements, got {tuple(d_kernels.shape)}')
    if d_kld.numel() != 1:
        raise ValueError('slotformer_amd: kernel_sample d_kld is a float32 scalar on the device')
    out = torch.empty_like(dist)
    check(lib().sf_kernel_sample_bwd_f32(ptr(dist), ptr(noise), int(seed or 0) & _U64, int(tag) & 0xffffffff, float(prior_log_var), ptr(d_kernels),
                                         ptr(d_kld), float(kld_scale), ptr(out), R, D, stream(dist)))
    return out


def slate_attention_cached(q, kv_cache, Lk, num_heads, d_model, k_off, v_off):
    """One-query-per-sequence attention over the first Lk rows of a K/V cache.  q [B,1,ldq] (head block at column 0),
    kv_cache [B,Lmax,ld] holding k at column k_off and v at column v_off of each row."""
    _chk(q, kv_cache)
    B, Lq, ldq = q.shape
    Lmax, ld = kv_cache.shape[1], kv_cache.shape[2]
    out = torch.empty(B, Lq, d_model, device=q.device, dtype=torch.float32)
    check(lib().sf_slate_attention_strided_f32(q.data_ptr(), kv_cache.data_ptr() + 4 * k_off, kv_cache.data_ptr() + 4 * v_off,
                                               ptr(out), ldq, ld, ld, d_model, Lq * ldq, Lmax * ld, Lmax * ld, Lq * d_model, B, Lq,
                                               Lk, num_heads, d_model // num_heads, 0, stream()))
    return out


# ---- Physion VQA readout (csrc/physion_readout.hip) ------------------------------------------------------------------------------------------
READOUT_AGG = {'max': 0, 'sum': 1, 'mean': 2}
READOUT_LIMITS = '2 <= num_slots <= 16, slot_size and feats_dim multiples of 32 in [32, 256]'
READOUT_MAX_THRESH = 16


def physion_readout_ok(N, C, F):
    """Whether the readout kernels take these shapes (`sf_physion_readout_ok`; shapes only, no device needed)."""
    return bool(lib().sf_physion_readout_ok(int(N), int(C), int(F)))


def _readout_slots(slots, video_len):
    """slots [V, T_all, N, C] as the kernels read them -- any video / frame stride, [N, C] contiguous inside a frame, so a `[:, :video_len]` view
    costs no copy -> (slots, T)."""
    if not (torch.is_tensor(slots) and slots.is_cuda):
        raise RuntimeError('slotformer_amd: the readout needs its slots on a HIP device; there is no CPU fallback')
    if slots.dim() != 4:
        raise ValueError(f'slotformer_amd: readout slots are [V, T, N, C], got {tuple(slots.shape)}')
    if slots.dtype != torch.float32:
        slots = slots.float()
    N, C = slots.shape[2:]
    if slots.stride(3) != 1 or slots.stride(2) != C or slots.stride(1) < N * C or slots.stride(1) % 4 or slots.stride(0) % 4 or slots.data_ptr() % 16:
        slots = slots.contiguous()
    T = slots.shape[1] if video_len is None else min(int(video_len), slots.shape[1])
    return slots, T


def _readout_heads(W1, b1, w2, b2):
    """A head or a stack of K heads -> ([K,F,2C], [K,F], [K,F], [K]) contiguous float32."""
    W1 = W1.detach()
    W1 = W1.unsqueeze(0) if W1.dim() == 2 else W1
    K, F = W1.shape[:2]
    out = (W1.float().contiguous(), b1.detach().float().reshape(K, F).contiguous(), w2.detach().float().reshape(K, F).contiguous(),
           b2.detach().float().reshape(K).contiguous())
    _chk(*out)
    return out


def _index32(idx, dev):
    return None if idx is None else torch.as_tensor(idx, device=dev).to(torch.int32).contiguous()


def physion_readout_fwd(slots, W1, b1, w2, b2, agg, video_index=None, video_len=None, want_steps=False, want_pairs=False):
    """logits [K,B] = max over the first `video_len` frames of the readout of each of K heads (`sf_physion_readout_fwd_f32`; split-bf16 whatever the
    library's precision mode).  slots [V,T_all,N,C] (see `_readout_slots`); batch entry b is video `video_index[b]` (any order, repeats allowed),
    or the V videos in order.  Returns (logits [K,B], t_star [K,B] int32, step_logits [K,B,T] or None, pair_star [K,B,F] uint8 or None)."""
    slots, T = _readout_slots(slots, video_len)
    W1, b1, w2, b2 = _readout_heads(W1, b1, w2, b2)
    V, _, N, C = slots.shape
    K, F = W1.shape[:2]
    if W1.shape[2] != 2 * C:
        raise ValueError(f'slotformer_amd: linear1 takes {W1.shape[2]} inputs, a slot pair has {2 * C}')
    video_index = _index32(video_index, slots.device)
    B = V if video_index is None else video_index.numel()
    dev = slots.device
    logits = torch.empty(K, B, dtype=torch.float32, device=dev)
    t_star = torch.empty(K, B, dtype=torch.int32, device=dev)
    steps = torch.empty(K, B, T, dtype=torch.float32, device=dev) if want_steps else None
    pairs = torch.empty(K, B, F, dtype=torch.uint8, device=dev) if want_pairs else None
    check(lib().sf_physion_readout_fwd_f32(slots.data_ptr(), slots.stride(0), slots.stride(1), V, ptr(video_index), ptr(W1), ptr(b1), ptr(w2), ptr(b2),
                                           ptr(logits), ptr(t_star), ptr(steps), ptr(pairs), K, B, T, N, C, F, READOUT_AGG[agg], stream()))
    return logits, t_star, steps, pairs


def physion_readout_bwd(slots, W1, b1, w2, g, t_star, agg, pair_star=None, video_index=None, video_len=None, out=None):
    """Gradients of ONE head from g [B] = dL/dlogit and the forward's routing (`sf_physion_readout_bwd_f32`): (dW1 [F,2C], db1 [F], dw2 [F],
    db2 [1]); `out`: a flat float32 buffer of F * 2C + 2F + 1 elements to write them into, in that order (the views are returned)."""
    slots, T = _readout_slots(slots, video_len)
    W1, b1, w2, _ = _readout_heads(W1, b1, w2, torch.zeros(1, device=slots.device))
    if W1.shape[0] != 1:
        raise ValueError('slotformer_amd: the readout backward takes one head')
    V, _, N, C = slots.shape
    F = W1.shape[1]
    video_index = _index32(video_index, slots.device)
    B = V if video_index is None else video_index.numel()
    g = g.detach().float().reshape(B).contiguous()
    t_star = t_star.reshape(B).to(torch.int32).contiguous()
    if pair_star is not None:
        pair_star = pair_star.reshape(B, F).to(torch.uint8).contiguous()
    n = F * 2 * C + 2 * F + 1
    flat = torch.empty(n, dtype=torch.float32, device=slots.device) if out is None else out
    if flat.numel() != n or flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError(f'slotformer_amd: the readout gradient buffer holds {n} contiguous float32 elements')
    dW1, db1, dw2, db2 = flat[:F * 2 * C].view(F, 2 * C), flat[F * 2 * C:F * 2 * C + F], flat[F * 2 * C + F:F * 2 * C + 2 * F], flat[n - 1:]
    ws = scratch(lib().sf_physion_readout_bwd_workspace_bytes, B, N, F, device=slots.device, at_least=16)
    check(lib().sf_physion_readout_bwd_f32(slots.data_ptr(), slots.stride(0), slots.stride(1), V, ptr(video_index), ptr(W1), ptr(b1), ptr(w2), ptr(g),
                                           ptr(t_star), ptr(pair_star), ptr(dW1), ptr(db1), ptr(dw2), ptr(db2), B, T, N, C, F, READOUT_AGG[agg],
                                           ws.data_ptr(), ws.numel(), stream()))
    return dW1, db1, dw2, db2


def physion_readout_score(logits, labels, threshs=(), task_idx=None, n_tasks=0, want_loss=True, want_grad=True, counts=None, task_counts=None):
    """One launch over logits [K,B] (`sf_physion_readout_score_f32`): the mean BCE-with-logits loss [K], g [K,B] = dloss/dlogit, and the int32 counts
    [K,thresholds] (and [K,n_tasks,thresholds]) of (sigmoid(logit) > thresh) == label, ADDED to `counts` / `task_counts` when those are passed, so
    that batches accumulate.  Returns (loss, g, counts, task_counts); what was not asked for is None."""
    import ctypes as C
    if not (torch.is_tensor(logits) and logits.is_cuda):
        raise RuntimeError('slotformer_amd: the readout score needs its logits on a HIP device; there is no CPU fallback')
    logits = logits.detach().float()
    logits = (logits.unsqueeze(0) if logits.dim() == 1 else logits).contiguous()
    K, B = logits.shape
    dev = logits.device
    labels = torch.as_tensor(labels, device=dev).float().reshape(B).contiguous()
    threshs = [float(t) for t in threshs]
    if len(threshs) > READOUT_MAX_THRESH:
        raise ValueError(f'slotformer_amd: at most {READOUT_MAX_THRESH} thresholds per score launch, got {len(threshs)}')
    task_idx = _index32(task_idx, dev)
    n_tasks = int(n_tasks) if task_idx is not None else 0
    loss = torch.empty(K, dtype=torch.float32, device=dev) if want_loss else None
    g = torch.empty(K, B, dtype=torch.float32, device=dev) if want_grad else None
    if threshs and counts is None:
        counts = torch.zeros(K, len(threshs), dtype=torch.int32, device=dev)
    if threshs and n_tasks and task_counts is None:
        task_counts = torch.zeros(K, n_tasks, len(threshs), dtype=torch.int32, device=dev)
    th = (C.c_float * max(len(threshs), 1))(*threshs)
    check(lib().sf_physion_readout_score_f32(ptr(logits), ptr(labels), ptr(task_idx), th, len(threshs), n_tasks, ptr(loss), ptr(g), ptr(counts),
                                             ptr(task_counts), K, B, stream()))
    return loss, g, counts, task_counts


# ---- PHYRE task-success readout and AUCCESS ranks (csrc/phyre_readout.hip) ---------------------------------------------------------------------
PHYRE_LIMITS = ('1 <= num_slots <= 16, slot_size a multiple of 32 in [32, 256], 1 + len(sel_slots) * num_slots <= 96 tokens, '
                '(d_model, num_heads, ffn_dim) = (128, 8, 512), norm_first, 1 <= num_layers <= 8')


def phyre_readout_ok(num_slots, slot_size, T, d_model=128, num_heads=8, ffn=512, num_layers=4):
    """Whether the PHYRE readout kernels take these shapes (`sf_phyre_readout_ok`; shapes only, no device needed)."""
    return bool(lib().sf_phyre_readout_ok(int(num_slots), int(slot_size), int(T), int(d_model), int(num_heads), int(ffn), int(num_layers)))


def phyre_readout_fwd(slots, sel, in_proj_w, in_proj_b, enc_t_pe, cls, layers, num_layers, mlp_w1, mlp_b1, mlp_w2, mlp_b2, video_index=None,
                      want_conf=False, scatter_index=None, scatter_table=None, d_model=128, num_heads=8, ffn=512):
    """logits [B] of the PHYRE readout (`sf_phyre_readout_fwd_f32`: embed, the layers as one launch, head).  slots [V,T_all,N,C] (see
    `_readout_slots`: read in place through their strides); sel: the frame of every token group as host integers, -1 = a frame of zeros; batch
    entry b is video `video_index[b]`, or the V videos in order.  layers: a host array of `sf_tfm_layer` whose `tok_packed` copies exist
    (engine.phyre_readout_plan).  want_conf: also sigmoid(logit) [B]; scatter_table (float32, contiguous) with scatter_index [B]: the
    confidences are written to scatter_table[scatter_index[b]] by the head kernel.  Returns (logits, conf or None)."""
    import ctypes as C
    slots, T_all = _readout_slots(slots, None)
    V, _, N, Cs = slots.shape
    dev = slots.device
    sel = [int(s) for s in sel]
    T = len(sel)
    video_index = _index32(video_index, dev)
    B = V if video_index is None else video_index.numel()
    _chk(in_proj_w, in_proj_b, enc_t_pe, cls, mlp_w1, mlp_b1, mlp_w2, mlp_b2, scatter_table)
    scatter_index = _index32(scatter_index, dev)
    if scatter_table is not None and (scatter_index is None or scatter_index.numel() != B):
        raise ValueError(f'slotformer_amd: a scatter table needs one scatter_index entry per batch entry ({B})')
    logits = torch.empty(B, dtype=torch.float32, device=dev)
    conf = torch.empty(B, dtype=torch.float32, device=dev) if want_conf else None
    ws = scratch(lib().sf_phyre_readout_workspace_bytes, B, N, T, device=dev, at_least=16)
    check(lib().sf_phyre_readout_fwd_f32(slots.data_ptr(), slots.stride(0), slots.stride(1), V, T_all, ptr(video_index), (C.c_int * max(T, 1))(*sel),
                                         ptr(in_proj_w), ptr(in_proj_b), ptr(enc_t_pe), ptr(cls), layers, int(num_layers), int(d_model), int(num_heads),
                                         int(ffn), ptr(mlp_w1), ptr(mlp_b1), ptr(mlp_w2), ptr(mlp_b2), ptr(logits), ptr(conf), ptr(scatter_index),
                                         ptr(scatter_table), 0 if scatter_table is None else scatter_table.numel(), B, T, N, Cs, ws.data_ptr(),
                                         ws.numel(), stream()))
    return logits, conf


PHYRE_LAYER_FIELDS = ('norm1_g', 'norm1_b', 'in_proj_w', 'in_proj_b', 'out_proj_w', 'out_proj_b', 'norm2_g', 'norm2_b', 'lin1_w', 'lin1_b', 'lin2_w',
                      'lin2_b')


def phyre_grad_layout(slot_size, T, num_layers, learnable_pe, d_model=128, ffn=512):
    """[(name, numel)] of the flat gradient buffer `phyre_readout_train_bwd` writes -- the order of `train.phyre_readout_parameters`: in_proj.weight,
    in_proj.bias, CLS, enc_t_pe (learnable tables only), each layer's twelve leaves (PHYRE_LAYER_FIELDS), cls_mlp.0.weight, cls_mlp.0.bias,
    cls_mlp.2.weight, cls_mlp.2.bias.  Every leaf but the last starts on a multiple of four floats."""
    d, f = int(d_model), int(ffn)
    out = [('in_proj_w', d * int(slot_size)), ('in_proj_b', d), ('cls', d)]
    if learnable_pe:
        out.append(('enc_t_pe', int(T) * d))
    sizes = (d, d, 3 * d * d, 3 * d, d * d, d, d, d, f * d, f, d * f, d)
    for i in range(int(num_layers)):
        out += [(f'layers.{i}.{n}', k) for n, k in zip(PHYRE_LAYER_FIELDS, sizes)]
    return out + [('mlp_w1', d * d), ('mlp_b1', d), ('mlp_w2', d), ('mlp_b2', 1)]


def _phyre_train_args(model, slots, sel, video_index):
    import ctypes as C
    slots, T_all = _readout_slots(slots, None)
    V, _, N, Cs = slots.shape
    if (N, Cs) != (model.num_slots, model.slot_size):
        raise ValueError(f'slotformer_amd: the readout takes slots [V, T, {model.num_slots}, {model.slot_size}], got {tuple(slots.shape)}')
    sel = [int(s) for s in sel]
    video_index = _index32(video_index, slots.device)
    B = V if video_index is None else video_index.numel()
    return slots, T_all, V, sel, (C.c_int * max(len(sel), 1))(*sel), video_index, B


def phyre_readout_train_workspace_bytes(model, B, T):
    """Bytes of the workspace the two training calls share for a batch of B (`sf_phyre_readout_train_workspace_bytes`; 0: unsupported)."""
    import ctypes as C
    return int(lib().sf_phyre_readout_train_workspace_bytes(C.byref(model), int(B), int(T)))


def phyre_readout_train_fwd(model, slots, sel, video_index=None, p=0., seed=0, want_gates=False, ws=None):
    """The training forward of the PHYRE readout (`sf_phyre_readout_train_fwd_f32`: the token rows, ONE launch per layer with dropout at its four
    sites, the head).  model: an `sf_phyre_readout_model` descriptor (train.phyre_readout_model); slots / sel / video_index as
    `phyre_readout_fwd`.  p, seed: the dropout rate and the seed of its masks (train.dropout_keep_mask restates them).  ws: a uint8 workspace to
    reuse (a larger one is fine), else one is allocated.  -> (logits [B], ws, gates, head_gates): the workspace holds what the backward reads;
    with want_gates the ReLU decisions the forward took, uint8 [num_layers, B * L, 512] and [B, 128], else None."""
    import ctypes as C
    slots, T_all, V, sel, sel_c, video_index, B = _phyre_train_args(model, slots, sel, video_index)
    dev, T = slots.device, len(sel)
    if phyre_readout_train_workspace_bytes(model, B, T) == 0:
        raise NotImplementedError(f'slotformer_amd: the PHYRE readout has no training kernel for these shapes: {PHYRE_LIMITS}')
    ws = scratch(lib().sf_phyre_readout_train_workspace_bytes, C.byref(model), B, T, device=dev, reuse=ws)
    L = 1 + T * model.num_slots
    logits = torch.empty(B, dtype=torch.float32, device=dev)
    gates = torch.empty(model.num_layers, B * L, model.ffn_dim, dtype=torch.uint8, device=dev) if want_gates else None
    head_gates = torch.empty(B, model.d_model, dtype=torch.uint8, device=dev) if want_gates else None
    check(lib().sf_phyre_readout_train_fwd_f32(C.byref(model), slots.data_ptr(), slots.stride(0), slots.stride(1), V, T_all, ptr(video_index), sel_c, B, T,
                                               float(p), int(seed), ptr(logits), ptr(gates), ptr(head_gates), ws.data_ptr(), ws.numel(), stream()))
    return logits, ws, gates, head_gates


def phyre_readout_train_bwd(model, slots, sel, g, ws, video_index=None, p=0., seed=0, learnable_pe=False, out=None):
    """Every parameter gradient of the PHYRE readout from g [B] = dL/dlogit and the workspace of `phyre_readout_train_fwd` (same slots, sel,
    video_index, p, seed): `sf_phyre_readout_train_bwd_f32`, ONE launch per layer for the activation gradients.  The gradients are WRITTEN into one
    flat float32 buffer in `phyre_grad_layout` order (out: a caller's buffer of that size, e.g. `FlatAdam.grad`); learnable_pe: whether enc_t_pe
    has a slot in it.  -> the flat buffer."""
    import ctypes as C
    from ._lib import sf_phyre_readout_grads, sf_tfm_layer_grads
    slots, T_all, V, sel, sel_c, video_index, B = _phyre_train_args(model, slots, sel, video_index)
    T = len(sel)
    layout = phyre_grad_layout(model.slot_size, T, model.num_layers, learnable_pe, model.d_model, model.ffn_dim)
    n = sum(k for _, k in layout)
    flat = torch.empty(n, dtype=torch.float32, device=slots.device) if out is None else out
    if not (torch.is_tensor(flat) and flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous() and flat.numel() == n):
        raise ValueError(f'slotformer_amd: the PHYRE readout gradient buffer holds {n} contiguous float32 elements on the device')
    g = g.detach().float().reshape(B).contiguous()
    gs = sf_phyre_readout_grads()
    arr = (sf_tfm_layer_grads * model.num_layers)()
    off = 0
    for name, k in layout:
        addr = flat.data_ptr() + 4 * off
        if name.startswith('layers.'):
            _, i, field = name.split('.')
            setattr(arr[int(i)], field, addr)
        else:
            setattr(gs, name, addr)
        off += k
    gs.layers = C.cast(arr, C.POINTER(sf_tfm_layer_grads))
    check(lib().sf_phyre_readout_train_bwd_f32(C.byref(model), slots.data_ptr(), slots.stride(0), slots.stride(1), V, T_all, ptr(video_index), sel_c, B, T,
                                               ptr(g), C.byref(gs), float(p), int(seed), ws.data_ptr(), ws.numel(), stream()))
    return flat


def phyre_auccess_ranks(conf, status):
    """first_rank [tasks] int32 (`sf_phyre_auccess_f32`): for every task the number of valid actions (status != 0) whose confidence lies strictly
    above the best solved action's (status > 0) -- `actions` when no action of the task is solved.  conf [tasks, actions] float32 and status
    [tasks, actions] (any integer dtype) on the device."""
    if not (torch.is_tensor(conf) and conf.is_cuda and torch.is_tensor(status) and status.is_cuda):
        raise RuntimeError('slotformer_amd: AUCCESS ranks need conf and status on a HIP device; there is no CPU fallback')
    if conf.dim() != 2 or tuple(status.shape) != tuple(conf.shape) or conf.numel() == 0:
        raise ValueError(f'slotformer_amd: conf and status are [tasks, actions], got {tuple(conf.shape)} and {tuple(status.shape)}')
    conf = conf.detach().float().contiguous()
    status = status.to(torch.int32).contiguous()
    tasks, actions = conf.shape
    ranks = torch.empty(tasks, dtype=torch.int32, device=conf.device)
    check(lib().sf_phyre_auccess_f32(ptr(conf), ptr(status), ptr(ranks), tasks, actions, stream()))
    return ranks


# ---- CLEVRER VQA: the Aloe reasoner (csrc/aloe.hip) --------------------------------------------------------------------------------------------
ALOE_LIMITS = ('1 <= num_slots <= 16, slot_size a multiple of 32 in [32, 256], 1 + frames * num_slots + text positions <= 256 tokens, '
               'd_model = heads * head_dim <= 256 and a multiple of 4, head_dim even in [4, 32], ffn_dim a multiple of 64 in [64, 1024], '
               'norm_first, 1 <= num_layers <= 32')
ALOE_COUNT_KEYS = ('descriptive', 'multiple-choice', 'explanatory', 'predictive', 'counterfactual')   # (right, questions) pairs of the counts


def aloe_ok(num_slots, slot_size, T, text_len, d_model, num_heads, ffn, num_layers):
    """Whether the Aloe kernels take these shapes (`sf_aloe_ok`; shapes only, no device needed)."""
    return bool(lib().sf_aloe_ok(int(num_slots), int(slot_size), int(T), int(text_len), int(d_model), int(num_heads), int(ffn), int(num_layers)))


def aloe_text_table(q_embedding, q_in_proj_w, q_in_proj_b):
    """table [vocab, d_model] = q_in_proj over [q_embedding[w] | . . | 1 0] without the type pair (`sf_aloe_text_table_f32`)."""
    _chk(q_embedding, q_in_proj_w, q_in_proj_b)
    vocab, E = q_embedding.shape
    d = q_in_proj_w.shape[0]
    if q_in_proj_w.shape[1] != E + 4:
        raise ValueError(f'slotformer_amd: q_in_proj takes {q_in_proj_w.shape[1]} inputs, an embedding with its two id pairs has {E + 4}')
    table = torch.empty(vocab, d, dtype=torch.float32, device=q_embedding.device)
    check(lib().sf_aloe_text_table_f32(ptr(q_embedding), ptr(q_in_proj_w), ptr(q_in_proj_b), ptr(table), vocab, E, d, stream()))
    return table


def aloe_fwd(model_struct, slots, tokens, pad_mask, head, multiple_choice, video_index=None, start=None, frame_offset=1, want_answers=False):
    """logits [B, A] of the Aloe reasoner (`sf_aloe_fwd_f32`).  model_struct: the `sf_aloe` of engine.aloe_plan; slots [V,T_all,N,C] read in place
    (see `_readout_slots`) at video `video_index[b]` (default b), frames `start[b] + t * frame_offset` (default from 0); tokens / pad_mask
    [B, text_len] (pad_mask True = padded); head: (W1, b1, W2, b2) of the answer MLP.  Returns (logits, answers [B] int32 or None)."""
    import ctypes as C
    slots, T_all = _readout_slots(slots, None)
    V = slots.shape[0]
    dev = slots.device
    tokens = torch.as_tensor(tokens, device=dev).to(torch.int32).contiguous()
    pad_mask = torch.as_tensor(pad_mask, device=dev).to(torch.uint8).contiguous()
    m = model_struct
    if tokens.dim() != 2 or tokens.shape[1] != m.text_len or tuple(pad_mask.shape) != tuple(tokens.shape):
        raise ValueError(f'slotformer_amd: tokens and pad mask are [B, {m.text_len}], got {tuple(tokens.shape)} and {tuple(pad_mask.shape)}')
    if tuple(slots.shape[2:]) != (m.num_slots, m.slot_size):
        raise ValueError(f'slotformer_amd: slots are [V, T, {m.num_slots}, {m.slot_size}], got {tuple(slots.shape)}')
    B = tokens.shape[0]
    video_index, start = _index32(video_index, dev), _index32(start, dev)
    for name, t in (('video_index', video_index), ('start', start)):
        if t is not None and t.numel() != B:
            raise ValueError(f'slotformer_amd: {name} holds one entry per batch entry ({B}), got {t.numel()}')
    W1, b1, W2, b2 = head
    _chk(W1, b1, W2, b2)
    H, A = W1.shape[0], W2.shape[0]
    logits = torch.empty(B, A, dtype=torch.float32, device=dev)
    answers = torch.empty(B, dtype=torch.int32, device=dev) if want_answers else None
    ws = scratch(lib().sf_aloe_workspace_bytes, B, m.num_slots, m.T, m.text_len, m.d_model, m.ffn_dim, device=dev, at_least=16)
    check(lib().sf_aloe_fwd_f32(C.byref(m), slots.data_ptr(), slots.stride(0), slots.stride(1), V, T_all, ptr(video_index), ptr(start), int(frame_offset),
                                ptr(tokens), ptr(pad_mask), int(bool(multiple_choice)), ptr(W1), ptr(b1), ptr(W2), ptr(b2), H, A, ptr(logits), ptr(answers), B,
                                ws.data_ptr(), ws.numel(), stream()))
    return logits, answers


def aloe_score(cls_logits=None, cls_labels=None, mc_logits=None, mc_labels=None, mc_flag=None, mc_subtype=None, counts=None, device=None):
    """One launch (`sf_aloe_score_f32`): losses [2] = (mean cross-entropy of the descriptive logits [B1, A], mean BCE-with-logits of the
    multiple-choice logits [Bn]; 0 for an absent kind), ques_correct [Q] int32 (Q = len(mc_subtype): every choice of the question right) and the
    int32 counts [10] -- (right, questions) for ALOE_COUNT_KEYS -- ADDED to `counts` when it is passed, so that batches accumulate."""
    have_cls, have_mc = cls_logits is not None and cls_logits.numel() > 0, mc_logits is not None and mc_logits.numel() > 0
    dev = cls_logits.device if have_cls else (mc_logits.device if have_mc else device)
    if dev is None or torch.device(dev).type != 'cuda':
        raise RuntimeError('slotformer_amd: the answer score needs its logits on a HIP device; there is no CPU fallback')
    B1 = A = Bn = Q = 0
    if have_cls:
        cls_logits = cls_logits.detach().float().contiguous()
        B1, A = cls_logits.shape
        cls_labels = torch.as_tensor(cls_labels, device=dev).reshape(B1).to(torch.int32).contiguous()
    else:
        cls_logits = cls_labels = None
    if have_mc:
        mc_logits = mc_logits.detach().float().reshape(-1).contiguous()
        Bn = mc_logits.numel()
        mc_labels = torch.as_tensor(mc_labels, device=dev).reshape(Bn).float().contiguous()
        mc_flag = torch.as_tensor(mc_flag, device=dev).reshape(Bn).to(torch.int32).contiguous()
        mc_subtype = _index32(mc_subtype, dev)
        Q = 0 if mc_subtype is None else mc_subtype.numel()
    else:
        mc_logits = mc_labels = mc_flag = mc_subtype = None
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    ques = torch.empty(Q, dtype=torch.int32, device=dev)
    if counts is None:
        counts = torch.zeros(10, dtype=torch.int32, device=dev)
    check(lib().sf_aloe_score_f32(ptr(cls_logits), ptr(cls_labels), B1, A, ptr(mc_logits), ptr(mc_labels), ptr(mc_flag), Bn, ptr(mc_subtype), Q, ptr(losses),
                                  ques.data_ptr() if Q else None, ptr(counts), stream()))
    return losses, ques, counts


# ---- training of the Aloe reasoner (csrc/aloe_train.hip) -----------------------------------------------------------------------------------------
ALOE_LAYER_FIELDS = PHYRE_LAYER_FIELDS


def aloe_train_ok(num_slots, slot_size, T, text_len, d_model, num_heads, ffn, num_layers):
    """Whether the Aloe training kernels take these shapes (`sf_aloe_train_ok`: what `aloe_ok` accepts; no device needed)."""
    return bool(lib().sf_aloe_train_ok(int(num_slots), int(slot_size), int(T), int(text_len), int(d_model), int(num_heads), int(ffn), int(num_layers)))


def aloe_grad_layout(slot_size, L, d_model, ffn, num_layers, vocab, emb_dim, mlp_hidden, num_answers):
    """[(name, numel)] of the flat gradient buffer `aloe_train_bwd` writes -- the order of `train.aloe_parameters`: CLS, pos_enc,
    vision_in_proj.weight / .bias, q_in_proj.weight / .bias, each layer's twelve leaves (ALOE_LAYER_FIELDS), the first linear of both answer MLPs,
    then the leaves whose size need not be a multiple of four: q_embedding, cls_answer_mlp.2, mc_answer_mlp.2.  Every leaf up to and including the
    layers' starts on a multiple of four floats (d_model is one)."""
    d, f, H, A, E = int(d_model), int(ffn), int(mlp_hidden), int(num_answers), int(emb_dim)
    out = [('cls', d), ('pos', int(L) * d), ('vision_w', d * (int(slot_size) + 2)), ('vision_b', d), ('q_in_proj_w', d * (E + 4)), ('q_in_proj_b', d)]
    sizes = (d, d, 3 * d * d, 3 * d, d * d, d, d, d, f * d, f, d * f, d)
    for i in range(int(num_layers)):
        out += [(f'layers.{i}.{n}', k) for n, k in zip(ALOE_LAYER_FIELDS, sizes)]
    return out + [('cls_w1', H * d), ('cls_b1', H), ('mc_w1', H * d), ('mc_b1', H), ('q_embedding', int(vocab) * E), ('cls_w2', A * H), ('cls_b2', A),
                  ('mc_w2', H), ('mc_b2', 1)]


def _aloe_layout_of(model):
    L = 1 + model.T * model.num_slots + model.text_len
    return aloe_grad_layout(model.slot_size, L, model.d_model, model.ffn_dim, model.num_layers, model.vocab, model.emb_dim, model.mlp_hidden,
                            model.num_answers)


def _aloe_train_args(model, slots, batch):
    """batch: dict(tokens [B, text_len], pad_mask [B, text_len], B1 -- the first B1 sequences are descriptive, the others choices --, video_index
    [B] or None, start [B] or None, frame_offset) -> the checked device tensors."""
    slots, T_all = _readout_slots(slots, None)
    dev = slots.device
    if tuple(slots.shape[2:]) != (model.num_slots, model.slot_size):
        raise ValueError(f'slotformer_amd: slots are [V, T, {model.num_slots}, {model.slot_size}], got {tuple(slots.shape)}')
    tokens = torch.as_tensor(batch['tokens'], device=dev).to(torch.int32).contiguous()
    pad = torch.as_tensor(batch['pad_mask'], device=dev).to(torch.uint8).contiguous()
    if tokens.dim() != 2 or tokens.shape[1] != model.text_len or tuple(pad.shape) != tuple(tokens.shape):
        raise ValueError(f'slotformer_amd: tokens and pad mask are [B, {model.text_len}], got {tuple(tokens.shape)} and {tuple(pad.shape)}')
    B = tokens.shape[0]
    B1 = int(batch['B1'])
    if not 0 <= B1 <= B:
        raise ValueError(f'slotformer_amd: B1 = {B1} descriptive sequences in a batch of {B}')
    vidx, start = _index32(batch.get('video_index'), dev), _index32(batch.get('start'), dev)
    for name, t in (('video_index', vidx), ('start', start)):
        if t is not None and t.numel() != B:
            raise ValueError(f'slotformer_amd: {name} holds one entry per batch entry ({B}), got {t.numel()}')
    return slots, T_all, tokens, pad, B, B1, vidx, start, int(batch.get('frame_offset', 1))


def aloe_train_fwd(model, slots, batch, p=0., seed=0, want_gates=False, ws=None):
    """The training forward of the Aloe reasoner (`sf_aloe_train_fwd_f32`).  model: an `sf_aloe_model` (train.aloe_model); slots [V, T_all, N, C] read
    in place; batch: see `_aloe_train_args`.  p, seed: the dropout rate and the seed of its masks.  ws: a uint8 workspace to reuse.
    -> (cls_logits [B1, A], mc_logits [Bn], ws, gates, head_gates): the workspace holds what the backward reads; with want_gates the ReLU
    decisions, uint8 [num_layers, B * L, ffn] and [B, mlp_hidden], else None."""
    import ctypes as C
    slots, T_all, tokens, pad, B, B1, vidx, start, offset = _aloe_train_args(model, slots, batch)
    dev = slots.device
    if int(lib().sf_aloe_train_workspace_bytes(C.byref(model), B)) == 0:
        raise NotImplementedError(f'slotformer_amd: the Aloe reasoner has no training kernel for this model or batch of {B}: {ALOE_LIMITS}, '
                                  '1 <= B <= 65535')
    ws = scratch(lib().sf_aloe_train_workspace_bytes, C.byref(model), B, device=dev, reuse=ws)
    L = 1 + model.T * model.num_slots + model.text_len
    cls_logits = torch.empty(B1, model.num_answers, dtype=torch.float32, device=dev)
    mc_logits = torch.empty(B - B1, dtype=torch.float32, device=dev)
    gates = torch.empty(model.num_layers, B * L, model.ffn_dim, dtype=torch.uint8, device=dev) if want_gates else None
    head_gates = torch.empty(B, model.mlp_hidden, dtype=torch.uint8, device=dev) if want_gates else None
    check(lib().sf_aloe_train_fwd_f32(C.byref(model), slots.data_ptr(), slots.stride(0), slots.stride(1), slots.shape[0], T_all, ptr(vidx), ptr(start),
                                      offset, ptr(tokens), ptr(pad), B1, B - B1, float(p), int(seed), ptr(cls_logits) if B1 else None,
                                      ptr(mc_logits) if B > B1 else None, ptr(gates), ptr(head_gates), ws.data_ptr(), ws.numel(), stream()))
    return cls_logits, mc_logits, ws, gates, head_gates


def aloe_train_bwd(model, slots, batch, g_cls, g_mc, ws, p=0., seed=0, out=None):
    """Every parameter gradient of the Aloe reasoner from g_cls [B1, A] and g_mc [Bn] = dL/dlogits and the workspace of `aloe_train_fwd` (same
    slots, batch, p, seed): `sf_aloe_train_bwd_f32`.  The gradients are WRITTEN into one flat float32 buffer in `aloe_grad_layout` order (out: a
    caller's buffer of that size, e.g. `FlatAdam.grad`).  -> the flat buffer."""
    import ctypes as C
    from ._lib import sf_aloe_grads, sf_tfm_layer_grads
    slots, T_all, tokens, pad, B, B1, vidx, start, offset = _aloe_train_args(model, slots, batch)
    layout = _aloe_layout_of(model)
    n = sum(k for _, k in layout)
    flat = torch.empty(n, dtype=torch.float32, device=slots.device) if out is None else out
    if not (torch.is_tensor(flat) and flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous() and flat.numel() == n):
        raise ValueError(f'slotformer_amd: the Aloe gradient buffer holds {n} contiguous float32 elements on the device')
    g_cls = None if B1 == 0 else g_cls.detach().float().reshape(B1, model.num_answers).contiguous()
    g_mc = None if B == B1 else g_mc.detach().float().reshape(B - B1).contiguous()
    gs = sf_aloe_grads()
    arr = (sf_tfm_layer_grads * model.num_layers)()
    off = 0
    for name, k in layout:
        addr = flat.data_ptr() + 4 * off
        if name.startswith('layers.'):
            _, i, field = name.split('.')
            setattr(arr[int(i)], field, addr)
        else:
            setattr(gs, name, addr)
        off += k
    gs.layers = C.cast(arr, C.POINTER(sf_tfm_layer_grads))
    check(lib().sf_aloe_train_bwd_f32(C.byref(model), slots.data_ptr(), slots.stride(0), slots.stride(1), slots.shape[0], T_all, ptr(vidx), ptr(start),
                                      offset, ptr(tokens), ptr(pad), B1, B - B1, ptr(g_cls), ptr(g_mc), C.byref(gs), float(p), int(seed), ws.data_ptr(),
                                      ws.numel(), stream()))
    return flat


def aloe_score_grad(cls_logits, cls_labels, mc_logits, mc_labels, w_cls=1., w_mc=1., want_grad=True):
    """One launch (`sf_aloe_score_grad_f32`): losses [2] = (mean cross-entropy of cls_logits [B1, A] against cls_labels, mean BCE-with-logits of
    mc_logits [Bn] against mc_labels; 0 for an empty kind) and the gradient of w_cls * losses[0] + w_mc * losses[1] in the logits.
    -> (losses, g_cls [B1, A], g_mc [Bn]); the gradients are None with want_grad=False."""
    require_device(cls_logits, mc_logits, what='the logits')
    dev = cls_logits.device
    cls_logits = cls_logits.detach().float().contiguous()
    mc_logits = mc_logits.detach().float().reshape(-1).contiguous()
    B1, A = cls_logits.shape
    Bn = mc_logits.numel()
    cls_labels = torch.as_tensor(cls_labels, device=dev).reshape(B1).to(torch.int32).contiguous() if B1 else None
    mc_labels = torch.as_tensor(mc_labels, device=dev).reshape(Bn).float().contiguous() if Bn else None
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    g_cls = torch.empty_like(cls_logits) if want_grad else None
    g_mc = torch.empty_like(mc_logits) if want_grad else None
    check(lib().sf_aloe_score_grad_f32(ptr(cls_logits) if B1 else None, ptr(cls_labels), B1, A, ptr(mc_logits) if Bn else None, ptr(mc_labels), Bn,
                                       float(w_cls), float(w_mc), ptr(losses), ptr(g_cls) if B1 else None, ptr(g_mc) if Bn else None, stream()))
    return losses, g_cls, g_mc
