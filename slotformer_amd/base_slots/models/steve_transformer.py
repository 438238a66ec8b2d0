"""STEVE's slot-conditioned Transformer decoder on the MI355X engine
(reference: slotformer/base_slots/models/steve_transformer.py, after singhgautam/slate).

The nn.Modules hold parameters under the reference's state-dict names; `STEVETransformerDecoder.forward/generate` run
on the HIP library: bias-free q|k|v projections as one GEMM per attention (LayerNorm fused as the GEMM prologue),
`sf_slate_attention_f32` (online-softmax attention, causal for the token stream, plain for the slots), output
projection with the residual fused in the GEMM epilogue, FFN as two GEMMs, `sf_embed_tokens_f32`,
`sf_argmax_rows_f32`.  Inference only."""
import torch
from torch import nn

from ... import ops, plans
from ..._call import ptr, scratch, stream


def linear(in_features, out_features, bias=True, weight_init='xavier', gain=1.):
    """Parameter holder with the reference's initialisers (steve_utils.py:151-166)."""
    m = nn.Linear(in_features, out_features, bias)
    if weight_init == 'kaiming':
        nn.init.kaiming_uniform_(m.weight, nonlinearity='relu')
    else:
        nn.init.xavier_uniform_(m.weight, gain)
    if bias:
        nn.init.zeros_(m.bias)
    return m


class MultiHeadAttention(nn.Module):
    """steve_transformer.py:12-55 (bias-free projections)."""

    def __init__(self, d_model, num_heads, dropout=0., gain=1.):
        super().__init__()
        assert d_model % num_heads == 0, 'd_model must be divisible by num_heads'
        self.d_model = d_model
        self.num_heads = num_heads
        self.attn_dropout = nn.Dropout(dropout)
        self.output_dropout = nn.Dropout(dropout)
        self.proj_q = linear(d_model, d_model, bias=False)
        self.proj_k = linear(d_model, d_model, bias=False)
        self.proj_v = linear(d_model, d_model, bias=False)
        self.proj_o = linear(d_model, d_model, bias=False, gain=gain)


class PositionalEncoding(nn.Module):
    """Learned position table (steve_transformer.py:58-74)."""

    def __init__(self, max_len, d_model, dropout=0.1):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        self.pe = nn.Parameter(torch.zeros(1, max_len, d_model), requires_grad=True)
        nn.init.trunc_normal_(self.pe)


class TransformerDecoderBlock(nn.Module):
    """steve_transformer.py:146-199."""

    def __init__(self, max_len, d_model, num_heads, dropout=0., gain=1., is_first=False):
        super().__init__()
        self.is_first = is_first
        self.self_attn_layer_norm = nn.LayerNorm(d_model)
        self.self_attn = MultiHeadAttention(d_model, num_heads, dropout, gain)
        mask = torch.triu(torch.ones((max_len, max_len), dtype=torch.bool), diagonal=1)
        self.self_attn_mask = nn.Parameter(mask, requires_grad=False)
        self.encoder_decoder_attn_layer_norm = nn.LayerNorm(d_model)
        self.encoder_decoder_attn = MultiHeadAttention(d_model, num_heads, dropout, gain)
        self.ffn_layer_norm = nn.LayerNorm(d_model)
        self.ffn = nn.Sequential(
            linear(d_model, 4 * d_model, weight_init='kaiming'), nn.ReLU(),
            linear(4 * d_model, d_model, gain=gain), nn.Dropout(dropout))


class TransformerDecoder(nn.Module):
    """steve_transformer.py:202-241."""

    def __init__(self, num_blocks, max_len, d_model, num_heads, dropout=0.):
        super().__init__()
        if num_blocks > 0:
            gain = (3 * num_blocks)**(-0.5)
            self.blocks = nn.ModuleList(
                [TransformerDecoderBlock(max_len, d_model, num_heads, dropout, gain, is_first=True)] +
                [TransformerDecoderBlock(max_len, d_model, num_heads, dropout, gain, is_first=False)
                 for _ in range(num_blocks - 1)])
        else:
            self.blocks = nn.ModuleList()
        self.layer_norm = nn.LayerNorm(d_model)


class STEVETransformerDecoder(nn.Module):
    """steve_transformer.py:244-333."""

    def __init__(self, vocab_size, d_model, n_head, max_len, num_slots, num_layers, dropout=0.1):
        super().__init__()
        self.max_len = max_len
        self.vocab_size = vocab_size
        self.num_slots = num_slots
        self.d_model = d_model
        self.n_head = n_head
        self.in_proj = nn.Linear(d_model, d_model)
        self.tok_emb = nn.Embedding(vocab_size + 1, d_model)
        self.pos_emb = PositionalEncoding(max_len + 1, d_model, dropout)
        self.tf_dec = TransformerDecoder(num_blocks=num_layers, max_len=max_len + 1, d_model=d_model, num_heads=n_head,
                                         dropout=dropout)
        self.head = nn.Linear(d_model, vocab_size, bias=False)

    # ---- HIP compute ------------------------------------------------------------------------------------
    def _catw(self, name, *ws):
        """cat of projection weights (q|k|v or k|v), rebuilt when a weight changes."""
        return plans.cached(self, name, plans.signature(*ws), lambda: torch.cat([w.detach() for w in ws], 0).contiguous())

    def forward(self, slots, idx):
        """slots [B,N,d], idx int64 [B,t] (targets without the last token) -> logits [B,1+t,V]."""
        assert slots.shape[1] == self.num_slots
        B, T = idx.shape
        assert T <= self.max_len
        if torch.is_grad_enabled() and (slots.requires_grad or any(p.requires_grad for p in self.parameters())):
            from ... import train
            return train.slate_decoder_forward(self, slots, idx)   # chain of HIP-backed autograd nodes (row N1)
        if self.training:
            raise RuntimeError('slotformer_amd STEVETransformerDecoder: train() mode without autograd; use .eval() + torch.no_grad()')
        d, H = self.d_model, self.n_head
        mem = ops.linear(slots.contiguous(), self.in_proj.weight.detach(), self.in_proj.bias.detach())   # [B,N,d]
        bos = torch.full((B, 1), self.vocab_size, dtype=torch.int64, device=idx.device)
        tokens = torch.cat([bos, idx.to(torch.int64)], 1).contiguous()                                # [B,1+t]
        x = ops.embed_tokens(tokens, self.tok_emb.weight.detach(), self.pos_emb.pe.detach()[0])        # [B,L,d]
        for i, blk in enumerate(self.tf_dec.blocks):
            sa, ca = blk.self_attn, blk.encoder_decoder_attn
            ln1 = (blk.self_attn_layer_norm.weight.detach(), blk.self_attn_layer_norm.bias.detach())
            wqkv = self._catw(f'sa{i}', sa.proj_q.weight, sa.proj_k.weight, sa.proj_v.weight)
            if blk.is_first:   # the first block normalises its input IN PLACE (steve_transformer.py:186-190)
                x = ops.layernorm(x, *ln1)
                qkv = ops.linear(x, wqkv)
            else:
                qkv = ops.linear(x, wqkv, ln=ln1)
            att = ops.slate_attention(qkv, qkv, qkv, H, True, 0, d, 2 * d, d_model=d)
            x = ops.linear(att, sa.proj_o.weight.detach(), residual=x)
            ln2 = (blk.encoder_decoder_attn_layer_norm.weight.detach(), blk.encoder_decoder_attn_layer_norm.bias.detach())
            q = ops.linear(x, ca.proj_q.weight.detach(), ln=ln2)
            kv = ops.linear(mem, self._catw(f'ca{i}', ca.proj_k.weight, ca.proj_v.weight))             # [B,N,2d]
            att = ops.slate_attention(q, kv, kv, H, False, 0, 0, d, d_model=d)
            x = ops.linear(att, ca.proj_o.weight.detach(), residual=x)
            ln3 = (blk.ffn_layer_norm.weight.detach(), blk.ffn_layer_norm.bias.detach())
            hdn = ops.linear(x, blk.ffn[0].weight.detach(), blk.ffn[0].bias.detach(), ln=ln3, relu=True)
            x = ops.linear(hdn, blk.ffn[2].weight.detach(), blk.ffn[2].bias.detach(), residual=x)
        fin = self.tf_dec.layer_norm
        return ops.linear(x, self.head.weight.detach(), ln=(fin.weight.detach(), fin.bias.detach()))

    def _slate_plan(self):
        """sf_slate_decoder descriptor (device pointers of the weights + concatenated projections), rebuilt when a
        parameter changes."""
        return plans.cached(self, 'slate', plans.signature(self), self._build_slate_plan)

    def _build_slate_plan(self):
        import ctypes as C
        from ..._lib import sf_slate_block, sf_slate_decoder
        plan = plans.Plan()
        dp = plan.dp
        blocks = (sf_slate_block * len(self.tf_dec.blocks))()
        for i, blk in enumerate(self.tf_dec.blocks):
            sa, ca, k = blk.self_attn, blk.encoder_decoder_attn, blocks[i]
            k.ln1_g, k.ln1_b = dp(blk.self_attn_layer_norm.weight), dp(blk.self_attn_layer_norm.bias)
            k.wqkv = dp(torch.cat([sa.proj_q.weight, sa.proj_k.weight, sa.proj_v.weight], 0))
            k.wo = dp(sa.proj_o.weight)
            k.ln2_g, k.ln2_b = dp(blk.encoder_decoder_attn_layer_norm.weight), dp(blk.encoder_decoder_attn_layer_norm.bias)
            k.wq_c, k.wo_c = dp(ca.proj_q.weight), dp(ca.proj_o.weight)
            k.wkv_c = dp(torch.cat([ca.proj_k.weight, ca.proj_v.weight], 0))
            k.ln3_g, k.ln3_b = dp(blk.ffn_layer_norm.weight), dp(blk.ffn_layer_norm.bias)
            k.w1, k.b1, k.w2, k.b2 = dp(blk.ffn[0].weight), dp(blk.ffn[0].bias), dp(blk.ffn[2].weight), dp(blk.ffn[2].bias)
            k.is_first = int(blk.is_first)
        m = sf_slate_decoder()
        m.d_model, m.num_heads, m.num_layers = self.d_model, self.n_head, len(self.tf_dec.blocks)
        m.vocab_size, m.num_slots, m.max_len = self.vocab_size, self.num_slots, self.max_len
        m.in_proj_w, m.in_proj_b = dp(self.in_proj.weight), dp(self.in_proj.bias)
        m.tok_emb, m.pos_emb = dp(self.tok_emb.weight), dp(self.pos_emb.pe[0])
        m.lnf_g, m.lnf_b = dp(self.tf_dec.layer_norm.weight), dp(self.tf_dec.layer_norm.bias)
        m.head_w = dp(self.head.weight)
        m.blocks = C.cast(blocks, C.POINTER(sf_slate_block))
        plan.keep.append(blocks)
        plan.struct = m
        return plan

    def generate_cached(self, slots, steps):
        """Greedy generation with a K/V cache (`sf_slate_generate_f32`): the same arithmetic as `generate(sample=False)`,
        one new token per step instead of re-running the prefix, the whole loop inside one C call; returns (tokens
        [B,steps] on device, logits [B,steps,V] on the CPU like the reference)."""
        import ctypes as C
        from ..._lib import check, lib
        if self.training or torch.is_grad_enabled():
            raise RuntimeError('slotformer_amd STEVETransformerDecoder is inference-only: .eval() + torch.no_grad()')
        if not (slots.is_cuda and slots.dtype == torch.float32):
            raise RuntimeError('generate_cached needs float32 slots on a HIP device; there is no CPU fallback')
        assert slots.shape[1] == self.num_slots and steps - 1 <= self.max_len
        slots = slots.contiguous()
        B = slots.shape[0]
        m = self._slate_plan().struct
        tokens = torch.empty(B, steps, dtype=torch.int64, device=slots.device)
        logits = torch.empty(B, steps, self.vocab_size, dtype=torch.float32, device=slots.device)
        ws = scratch(lib().sf_slate_generate_workspace_bytes, C.byref(m), B, steps, device=slots.device)
        check(lib().sf_slate_generate_f32(C.byref(m), slots.data_ptr(), B, steps, tokens.data_ptr(), logits.data_ptr(),
                                          ws.data_ptr(), ws.numel(), stream()))
        return tokens, logits.cpu()

    def generate_tokens(self, slots, steps, return_logits=False, frames_per_wg=0, *, soft_table=None, soft_scale=10.0, soft_seed=0,
                        sample=False, temperature=1.0, sample_seed=0, row_base=0):
        """Generation that stays on the device (`sf_slate_generate_tok_opts_f32`): one launch per token where the fused step
        applies (`sf_slate_step_ok`), a workgroup owning `frames_per_wg` frames (1, 2 or 4; 0 = the library's choice, which may
        be the launch chain of `generate_cached`).  Returns (tokens [B,steps] int64, logits [B,steps,V] or None), both on the
        device; the logits are only written with return_logits=True.  `self.last_generate_form` is the form that ran: 0 for the
        launch chain, else the frames per workgroup of the fused step.

        Keyword-only, inside the fused step's vocabulary sweep (an error where the fused step refuses the decoder; frames_per_wg = 0
        then means one frame per workgroup).  `soft_table` [V,64] (`dVAE.conv0_table()`): a third value is returned, the soft rows
        [B,steps,64] = softmax((logits + Gumbel(soft_seed)) * soft_scale) @ soft_table, without the [B,steps,V] buffers.
        `sample=True`: the tokens are drawn from softmax(logits / temperature) by Gumbel-max with the noise of `sample_seed` instead
        of taken greedily.  Noise row r = row_base + b * steps + t, element r * V + v of `train.gumbel_noise`: a caller that splits a
        sequence of frames over several calls passes the rows before the call as `row_base`."""
        import ctypes as C
        from ..._lib import check, lib, sf_slate_step_opts
        if self.training or torch.is_grad_enabled():
            raise RuntimeError('slotformer_amd STEVETransformerDecoder is inference-only: .eval() + torch.no_grad()')
        if not (torch.is_tensor(slots) and slots.is_cuda and slots.dtype == torch.float32):
            raise RuntimeError('generate_tokens needs float32 slots on a HIP device; there is no CPU fallback')
        if frames_per_wg not in (0, 1, 2, 4):
            raise ValueError(f'generate_tokens: frames_per_wg is 0 (the library\'s choice), 1, 2 or 4, got {frames_per_wg!r}')
        assert slots.shape[1] == self.num_slots and steps - 1 <= self.max_len
        slots = slots.contiguous()
        B = slots.shape[0]
        m = self._slate_plan().struct
        tokens = torch.empty(B, steps, dtype=torch.int64, device=slots.device)
        logits = torch.empty(B, steps, self.vocab_size, dtype=torch.float32, device=slots.device) if return_logits else None
        ran = C.c_int(-1)
        if soft_table is None and not sample:
            ws = scratch(lib().sf_slate_generate_tok_workspace_bytes, C.byref(m), B, steps, device=slots.device)
            check(lib().sf_slate_generate_tok_f32(C.byref(m), slots.data_ptr(), B, steps, tokens.data_ptr(), ptr(logits), int(frames_per_wg),
                                                  ws.data_ptr(), ws.numel(), stream(), C.byref(ran)))
            self.last_generate_form = ran.value
            return tokens, logits
        o = sf_slate_step_opts()
        soft = None
        if soft_table is not None:
            if not (torch.is_tensor(soft_table) and soft_table.is_cuda and soft_table.dtype == torch.float32 and soft_table.is_contiguous()
                    and soft_table.dim() == 2 and soft_table.shape[0] == self.vocab_size):
                raise TypeError('generate_tokens: soft_table is a contiguous float32 device tensor [vocab_size, 64]')
            soft = torch.empty(B, steps, soft_table.shape[1], dtype=torch.float32, device=slots.device)
            o.soft_rows, o.conv0_t, o.conv0_width = soft.data_ptr(), soft_table.data_ptr(), int(soft_table.shape[1])
            o.soft_scale, o.soft_seed = float(soft_scale), int(soft_seed) & 0xffffffffffffffff
        if sample:
            o.sample, o.inv_temperature, o.sample_seed = 1, 1.0 / float(temperature), int(sample_seed) & 0xffffffffffffffff
        o.row_base = int(row_base)
        ws = scratch(lib().sf_slate_generate_tok_opts_workspace_bytes, C.byref(m), B, steps, C.byref(o), device=slots.device)
        check(lib().sf_slate_generate_tok_opts_f32(C.byref(m), slots.data_ptr(), B, steps, tokens.data_ptr(), ptr(logits), int(frames_per_wg),
                                                   ws.data_ptr(), ws.numel(), stream(), C.byref(ran), C.byref(o)))
        self.last_generate_form = ran.value
        return (tokens, logits) if soft_table is None else (tokens, logits, soft)

    def step_ok(self):
        """whether the fused token step (`sf_slate_step_ok`) takes this decoder's shapes"""
        import ctypes as C
        from ..._lib import lib, sf_slate_decoder
        m = sf_slate_decoder()   # shapes only: the query reads no weight
        m.d_model, m.num_heads, m.num_layers = self.d_model, self.n_head, len(self.tf_dec.blocks)
        m.vocab_size, m.num_slots, m.max_len = self.vocab_size, self.num_slots, self.max_len
        return bool(lib().sf_slate_step_ok(C.byref(m)))

    def generate(self, slots, steps, sample=False, temperature=1.0, seed=None):
        """Autoregressive generation (steve_transformer.py:305-333): the whole prefix is re-run every step, as in the reference;
        greedy (sample=False: argmax) or sampled (sample=True: one draw per step from softmax(logits / temperature) -- the softmax a HIP
        launch, the draw torch.multinomial on the device generator, as the reference draws it).  Returns (tokens [B,steps] on device,
        logits [B,steps,V] on the CPU like the reference).  sample=True with `seed`: the same distribution drawn by Gumbel-max inside the
        fused token step over the K/V cache (`generate_tokens(sample=True, sample_seed=seed)`), one launch per token instead of a forward
        over the prefix; NotImplementedError where the fused step refuses the decoder."""
        assert not self.training
        B = slots.shape[0]
        assert steps - 1 <= self.max_len
        if sample and seed is not None:
            if not self.step_ok():
                raise NotImplementedError('generate(sample=True, seed=...) runs the fused token step, which refuses this decoder '
                                          '(sf_slate_step_ok); without seed the draw is torch.multinomial over a prefix re-run')
            tokens, logits = self.generate_tokens(slots, steps, return_logits=True, sample=True, temperature=temperature, sample_seed=seed)
            return tokens, logits.cpu()
        idx_cond = torch.zeros((B, 0), dtype=torch.int64, device=slots.device)
        all_logits = []
        for _ in range(steps):
            logits = self.forward(slots, idx_cond)[:, -1].contiguous()   # [B,V]
            all_logits.append(logits.cpu())
            if sample:
                ix = torch.multinomial(ops.softmax_rows(logits, scale=1.0 / float(temperature)), num_samples=1)
            else:
                ix = ops.argmax_rows(logits).unsqueeze(1)                 # argmax of softmax(logits / T) = argmax of logits
            idx_cond = torch.cat((idx_cond, ix), dim=1)
        return idx_cond, torch.stack(all_logits, dim=1)
