"""dVAE image tokenizer on the MI355X engine (reference: slotformer/base_slots/models/dVAE.py, steve_utils.py:73-126).

The modules below only hold parameters under the reference's state-dict names (`encoder.{i}.m.weight`,
`encoder.{i}.weight/bias`, `decoder.…`); `tokenize` / `detokenize` run on the HIP library: 1x1 convolutions and the
4x4/stride-4 patch embedding as GEMMs over channels-last pixels (`sf_linear_f32`), the 3x3 convolutions on the
implicit-GEMM conv (`sf_conv2d_nhwc_f32`), GroupNorm(1)+ReLU(+PixelShuffle) in `sf_groupnorm1_nhwc_f32`, the token
pick in `sf_argmax_rows_f32`.  `tokenize_ids` is the dataset tokeniser: the patch embedding straight from NCHW frames and the vocabulary head with
the argmax inside (`sf_dvae_patch_embed_f32`, `sf_dvae_head_argmax_f32`), no logits in memory.  In training (`forward` outside `testing`, row N1) the same kernels run as autograd nodes of
`slotformer_amd.train` (`sf_linear_bwd_f32`, `sf_groupnorm1_nhwc_bwd_f32`, `sf_softmax_rows_bwd_f32`)."""
import torch
from torch import nn

from ...nerv_compat import BaseModel
from ... import ops, plans
from ..._call import require_device


def conv2d(in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, weight_init='xavier'):
    """Parameter holder with the reference's initialisers (steve_utils.py:73-97)."""
    m = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=bias)
    if weight_init == 'kaiming':
        nn.init.kaiming_uniform_(m.weight, nonlinearity='relu')
    else:
        nn.init.xavier_uniform_(m.weight)
    if bias:
        nn.init.zeros_(m.bias)
    return m


class Conv2dBlock(nn.Module):
    """bias-free conv -> GroupNorm(1 group, affine weight/bias) -> ReLU (steve_utils.py:100-126)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        self.m = conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=False, weight_init='kaiming')
        self.weight = nn.Parameter(torch.ones(out_channels))
        self.bias = nn.Parameter(torch.zeros(out_channels))


class dVAE(BaseModel):

    def __init__(self, vocab_size, img_channels=3):
        super().__init__()
        self.vocab_size = vocab_size
        self.img_channels = img_channels
        self.tau = 1.
        # dVAE.py:24-50
        self.encoder = nn.Sequential(
            Conv2dBlock(img_channels, 64, 4, 4), *[Conv2dBlock(64, 64, 1, 1) for _ in range(6)],
            conv2d(64, vocab_size, 1))
        self.decoder = nn.Sequential(
            Conv2dBlock(vocab_size, 64, 1), Conv2dBlock(64, 64, 3, 1, 1), Conv2dBlock(64, 64, 1, 1),
            Conv2dBlock(64, 64, 1, 1), Conv2dBlock(64, 256, 1), nn.PixelShuffle(2),
            Conv2dBlock(64, 64, 3, 1, 1), Conv2dBlock(64, 64, 1, 1), Conv2dBlock(64, 64, 1, 1),
            Conv2dBlock(64, 256, 1), nn.PixelShuffle(2), conv2d(64, img_channels, 1))
        self.testing = False

    # ---- HIP compute ------------------------------------------------------------------------------------
    def _block(self, x, blk, pixel_shuffle=1):
        """x NHWC [F,H,W,Cin] -> Conv2dBlock(x) (optionally followed by PixelShuffle(2)), NHWC."""
        w = blk.m.weight.detach()
        if w.shape[2] == 1:
            y = ops.linear(x, w.reshape(w.shape[0], w.shape[1]).contiguous())
        else:   # (the OHWI copy of a 3x3 weight: kept on its block, rebuilt when the weight changes)
            w3x3 = plans.cached(blk, 'w3x3', plans.signature(w), lambda: ops.pack_conv_weight(w.contiguous()))
            y = ops.conv2d_nhwc(x, w3x3, None, relu=False)
        return ops.groupnorm1_nhwc(y, blk.weight.detach(), blk.bias.detach(), relu=True, pixel_shuffle=pixel_shuffle)

    def _logits_nhwc(self, imgs):
        """imgs [F,3,H,W] -> logits [F,h,w,V] (channels-last)."""
        if torch.is_grad_enabled():
            raise RuntimeError('slotformer_amd dVAE.tokenize is a hard argmax: call it under torch.no_grad()')
        F_, C_, H, W = imgs.shape
        h, w = H // 4, W // 4
        # 4x4 / stride-4 convolution = GEMM over (c, ky, kx) patch vectors (dVAE.py:26)
        x = imgs.reshape(F_, C_, h, 4, w, 4).permute(0, 2, 4, 1, 3, 5).reshape(F_, h, w, C_ * 16).contiguous()
        b0 = self.encoder[0]
        y = ops.linear(x, b0.m.weight.detach().reshape(64, C_ * 16).contiguous())
        x = ops.groupnorm1_nhwc(y, b0.weight.detach(), b0.bias.detach(), relu=True)
        for i in range(1, 7):
            x = self._block(x, self.encoder[i])
        last = self.encoder[7]
        return ops.linear(x, last.weight.detach().reshape(self.vocab_size, 64).contiguous(), last.bias.detach())

    def tokenize(self, imgs, one_hot=True):
        """dVAE.py:52-77: one-hot map [B,(T,)V,h,w] or token ids [B,(T,)h,w]."""
        B = imgs.shape[0]
        unflatten = imgs.dim() == 5
        if unflatten:
            imgs = imgs.flatten(0, 1)
        logits = self._logits_nhwc(imgs.contiguous())
        idx = ops.argmax_rows(logits)                      # [F,h,w]
        if one_hot:
            F_, h, w, V = logits.shape
            z = torch.zeros(F_, V, h, w, device=logits.device, dtype=logits.dtype).scatter_(1, idx.unsqueeze(1), 1.)
        else:
            z = idx
        return z.unflatten(0, (B, -1)) if unflatten else z

    def _head_packed(self):
        """The vocabulary head in the fragment order `ops.linear_argmax` streams; rebuilt when the parameter changes."""
        w = self.encoder[7].weight
        return plans.cached(self.encoder[7], 'head', plans.signature(w),
                            lambda: ops.pack_head_weight(w.detach().reshape(self.vocab_size, 64).float().contiguous()))

    @torch.no_grad()
    def tokenize_ids(self, imgs, out=None, dtype=torch.int64):
        """Token ids of frames for tokenising a dataset (base_slots/tokenize_images.py): imgs [B,(T,)3,H,W] device float32 -> ids [B,(T,)h,w]
        int64 or int16 (`dtype`; int16 is what the token files hold), written into `out` when given (contiguous, that dtype, that many
        elements).  What `tokenize(one_hot=False)` computes, without the patchify copy in front and without the logits [F,h,w,V] behind: the 4x4
        convolution reads the frames as they lie (`ops.patch_embed`) and the head picks the id from its accumulators (`ops.linear_argmax`), both in
        split-bf16 whatever the precision mode, so ids may differ from `tokenize` where the two best logits are closer than that arithmetic resolves.
        Asynchronous on the current stream; never syncs with the host.  Shapes `sf_dvae_tokens_ok` refuses go through `tokenize`."""
        if not (torch.is_tensor(imgs) and imgs.is_cuda and imgs.dtype == torch.float32 and imgs.dim() in (4, 5)):
            raise RuntimeError('slotformer_amd dVAE.tokenize_ids needs float32 frames [B,(T,)3,H,W] on a HIP device; there is no CPU fallback')
        if dtype not in (torch.int64, torch.int16):
            raise TypeError(f'dVAE.tokenize_ids: dtype is torch.int64 or torch.int16, got {dtype}')
        if dtype == torch.int16 and self.vocab_size > 32768:
            raise ValueError(f'dVAE.tokenize_ids: int16 ids cannot hold a vocabulary of {self.vocab_size}')
        lead = tuple(imgs.shape[:-3])
        flat = imgs.reshape((-1, ) + tuple(imgs.shape[-3:])).contiguous()
        F_, C_, H, W = flat.shape
        shape = lead + (H // 4, W // 4)
        if out is not None and not (out.is_cuda and out.dtype == dtype and out.is_contiguous() and out.numel() == F_ * (H // 4) * (W // 4)):
            raise TypeError(f'dVAE.tokenize_ids: out must be a contiguous {dtype} device tensor of {shape}')
        if not ops.dvae_tokens_ok(self.vocab_size, 64, C_, H, W):
            ids = self.tokenize(flat, one_hot=False).to(dtype).reshape(shape)   # the slower path, never an error
            if out is None:
                return ids
            out.view(shape).copy_(ids)
            return out.view(shape)
        e = self.encoder
        x = ops.patch_embed(flat, e[0].m.weight.detach().contiguous())
        x = ops.groupnorm1_nhwc(x, e[0].weight.detach(), e[0].bias.detach(), relu=True)
        for i in range(1, 7):
            x = self._block(x, e[i])
        if out is None:
            out = torch.empty(shape, device=flat.device, dtype=dtype)
        kw = {'out': out} if dtype == torch.int64 else {'out_i16': out}
        ops.linear_argmax(x, self._head_packed(), e[7].bias.detach(), self.vocab_size, **kw)
        return out.view(shape)

    def detokenize(self, z):
        """dVAE.py:79-100: z [B,(T,)V,h,w] (probabilities over the vocabulary) -> image [B,(T,)3,4h,4w]."""
        assert z.shape[-3] == self.vocab_size
        B = z.shape[0]
        unflatten = z.dim() == 5
        if unflatten:
            z = z.flatten(0, 1)
        if torch.is_grad_enabled():   # under autograd: the same arithmetic as a chain of differentiable nodes
            recon = self.decode_nhwc(z.permute(0, 2, 3, 1).float()).permute(0, 3, 1, 2)
            return recon.unflatten(0, (B, -1)) if unflatten else recon
        recon = self._decoder_tail(self._block(z.permute(0, 2, 3, 1).contiguous().float(), self.decoder[0]))
        return recon.unflatten(0, (B, -1)) if unflatten else recon

    def _decoder_tail(self, x):
        """The decoder stack after its first block: x NHWC [F,h,w,64] -> image [F,3,4h,4w]."""
        d = self.decoder
        x = self._block(x, d[1])
        x = self._block(x, d[2])
        x = self._block(x, d[3])
        x = self._block(x, d[4], pixel_shuffle=2)
        x = self._block(x, d[6])
        x = self._block(x, d[7])
        x = self._block(x, d[8])
        x = self._block(x, d[9], pixel_shuffle=2)
        last = d[11]
        x = ops.linear(x, last.weight.detach().reshape(self.img_channels, 64).contiguous(), last.bias.detach())
        return x.permute(0, 3, 1, 2).contiguous()

    def detokenize_nhwc(self, z):
        """`detokenize` of a channels-last map z [F,h,w,V] (no transpose on the way in) -> image [F,3,4h,4w]."""
        assert z.dim() == 4 and z.shape[-1] == self.vocab_size
        if torch.is_grad_enabled():
            raise RuntimeError('slotformer_amd dVAE.detokenize_nhwc is inference-only: call it under torch.no_grad()')
        return self._decoder_tail(self._block(z.contiguous().float(), self.decoder[0]))

    def detokenize_ids(self, ids):
        """Token ids [F,h,w] int64 on the device -> image [F,3,4h,4w]: `detokenize` of their one-hot map without building it.  The first
        decoder block's bias-free 1x1 convolution on a one-hot vector is one column of its weight, so it runs as a row gather of the
        transposed weight (`sf_gather_rows_f32`); the rest of the stack runs as in `detokenize`."""
        if torch.is_grad_enabled():
            raise RuntimeError('slotformer_amd dVAE.detokenize_ids is inference-only: call it under torch.no_grad()')
        if not (torch.is_tensor(ids) and ids.is_cuda and ids.dtype == torch.int64 and ids.dim() == 3):
            raise RuntimeError('detokenize_ids needs int64 token ids [F,h,w] on a HIP device; there is no CPU fallback')
        return self.detokenize_rows(ops.gather_rows(self.conv0_table(), ids.contiguous()))          # [F,h,w,64]

    def conv0_table(self):
        """The first decoder block's bias-free 1x1 convolution as a table [V, 64] (its transposed weight; cached until the weight changes):
        what `detokenize_ids` gathers from and the fused token step of the STEVE decoder weighs its soft rows with."""
        blk = self.decoder[0]
        w = blk.m.weight
        return plans.cached(blk, 'ids', plans.signature(w), lambda: w.detach().reshape(w.shape[0], w.shape[1]).t().float().contiguous())

    def detokenize_rows(self, y):
        """y [F,h,w,64] float32 on the device -- the output of the first decoder block's convolution, however it was computed (a row gather for
        token ids, the fused token step's soft rows for a relaxed sample) -> image [F,3,4h,4w]: block 0's GroupNorm + ReLU, then the rest of
        the decoder stack."""
        if torch.is_grad_enabled():
            raise RuntimeError('slotformer_amd dVAE.detokenize_rows is inference-only: call it under torch.no_grad()')
        blk = self.decoder[0]
        if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 4 and y.shape[-1] == blk.m.weight.shape[0]):
            raise RuntimeError('detokenize_rows needs float32 rows [F,h,w,%d] on a HIP device; there is no CPU fallback' % blk.m.weight.shape[0])
        return self._decoder_tail(ops.groupnorm1_nhwc(y.contiguous(), blk.weight.detach(), blk.bias.detach(), relu=True))

    # ---- training forward (dVAE.py:113-139) ---------------------------------------------------------------
    def _block_t(self, x, blk, pixel_shuffle=1):
        from ... import train
        w = blk.m.weight
        y = train.linear_weight(x, w.reshape(w.shape[0], w.shape[1])) if w.shape[2] == 1 else train.conv3x3_nhwc(x, w)
        return train.groupnorm1(y, blk.weight, blk.bias, relu=True, pixel_shuffle=pixel_shuffle)

    def decode_nhwc(self, z):
        """The decoder stack (dVAE.py:36-50) on a channels-last token map z [F,h,w,V] as autograd nodes -> image [F,4h,4w,3]
        channels-last.  Also what STEVE's Gumbel image loss differentiates through with the dVAE frozen (steve.py:327-335)."""
        from ... import train
        d = self.decoder
        y = self._block_t(z, d[0])
        y = self._block_t(y, d[1])
        y = self._block_t(y, d[2])
        y = self._block_t(y, d[3])
        y = self._block_t(y, d[4], pixel_shuffle=2)
        y = self._block_t(y, d[6])
        y = self._block_t(y, d[7])
        y = self._block_t(y, d[8])
        y = self._block_t(y, d[9], pixel_shuffle=2)
        return train.linear_weight(y, d[11].weight.reshape(self.img_channels, 64), d[11].bias)

    def forward(self, data_dict):
        """`img` [B,(T,)3,H,W]; optional `gumbel_tau`, `hard` as in the reference, and `gumbel` [B,(T,)V,h,w]: the Gumbel noise
        to use instead of a fresh draw (the reference draws it inside steve_utils.gumbel_softmax), or `gumbel_seed` (an int): the
        seed of the noise generated inside the softmax kernel (`train.gumbel_noise` rebuilds it), in place of one drawn from torch's
        CPU generator."""
        if self.testing:
            return self.tokenize(data_dict['img'], one_hot=False)
        from ... import train
        x = data_dict['img']
        require_device(x)
        tau = data_dict.get('gumbel_tau', self.tau)
        hard = data_dict.get('hard', False)
        B = x.shape[0]
        unflatten = x.dim() == 5
        if unflatten:
            x = x.flatten(0, 1)
        F_, C_, H, W = x.shape
        h, w = H // 4, W // 4
        e = self.encoder
        # encoder: 4x4 / stride-4 patch embedding as a GEMM over (c, ky, kx) patch vectors, six 1x1 blocks, logits
        p = x.float().reshape(F_, C_, h, 4, w, 4).permute(0, 2, 4, 1, 3, 5).reshape(F_, h, w, C_ * 16)
        y = train.linear_weight(p, e[0].m.weight.reshape(64, C_ * 16))
        y = train.groupnorm1(y, e[0].weight, e[0].bias, relu=True)
        for i in range(1, 7):
            y = self._block_t(y, e[i])
        logits = train.linear_weight(y, e[7].weight.reshape(self.vocab_size, 64), e[7].bias)     # [F,h,w,V]
        # relaxed sample of the token map
        g = data_dict.get('gumbel')
        if g is not None:
            g = (g.flatten(0, 1) if unflatten else g).permute(0, 2, 3, 1).to(logits.device).float().contiguous()
        # without `gumbel`: noise generated inside the softmax kernel, from `gumbel_seed` when given, else from a fresh seed
        z = train.gumbel_softmax(logits, g, tau, hard, seed=data_dict.get('gumbel_seed'))
        recon = self.decode_nhwc(z).permute(0, 3, 1, 2)
        # log-probabilities of the token map: reported, not part of the loss
        z_logits = ops.log_softmax_rows(logits.detach()).permute(0, 3, 1, 2)
        if unflatten:
            recon, z_logits = recon.unflatten(0, (B, -1)), z_logits.unflatten(0, (B, -1))
        return {'recon': recon, 'z_logits': z_logits}

    def calc_train_loss(self, data_dict, out_dict):
        """dVAE.py:141-146."""
        from ...host import losses
        return {'recon_loss': losses.image_recon_loss(out_dict['recon'], data_dict['img'])}

    @property
    def dtype(self):
        return self.encoder[-1].weight.dtype

    @property
    def device(self):
        return self.encoder[-1].weight.device
