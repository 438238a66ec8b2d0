"""The reference's video_prediction/vp_vis.py -- add_boundary, make_video, draw_bbox, batch_draw_bbox, same names, signatures and return values --
on the egress kernels (slotformer_amd/egress.py, csrc/egress.hip): device tensors are composed, quantised and drawn on on the device and downloaded
once; CPU tensors take egress's plain-torch home.  torchvision is not needed.

Beside them the forms that stay on the device and return uint8 in a video writer's layout -- make_video_u8, batch_draw_bbox_u8 --, STEVE's three-tile
video (make_steve_video, make_steve_video_u8: base_slots/method.py:293-310) and
slot_decomposition_grid, the grid of the trainers' sample videos (base_slots/method.py:102-131), for anyone porting a trainer off its make_grid loops.

One difference from the reference: a box with a side thinner than 2 * bbox_width is outlined inside the box only (PIL, which torchvision draws with,
paints outside such a box); see egress.draw_boxes_.
"""
import torch

from .. import egress
from ..base_slots.models import to_rgb_from_tensor  # noqa: F401  (the reference's module has both names too)
from .vp_utils import PALETTE  # noqa: F401


def _f32(x):
    return x.float().contiguous()


def add_boundary(img, width=2, color='red'):
    """img (T, 3, H, W) in [0, 1] -> (T, 3, H + 2 width, W + 2 width): the frames inside a red (0.7, 0, 0) or green (0, 0.7, 0) frame of `width` pixels,
    which marks rollout / ground-truth frames.  (A stand-alone helper: make_video frames its tiles inside the grid kernel.)"""
    if color not in ('red', 'green'):
        raise ValueError(f"slotformer_amd.vp_vis: color is 'red' or 'green', got {color!r}")
    T, C, H, W = img.shape
    framed = img.new_zeros(T, C, H + 2 * width, W + 2 * width)
    framed[:, 0 if color == 'red' else 1] = 0.7
    framed[:, :, width:width + H, width:width + W] = img
    return framed


def _video_tiles(video, pred_video, history_len):
    T = video.shape[0]
    return [egress.Img(_f32(video), border=(2, T)), egress.Img(_f32(pred_video), border=(2, history_len))]


def make_video(video, pred_video, history_len=6):
    """videos are of shape [T, C, H, W] in [-1, 1] -> float32 [T, 3, 2 (H + 4), W + 4] in [0, 1] on the CPU: the ground truth framed in green above
    the prediction, framed in green for the burn-in frames and in red from `history_len` on."""
    return egress.video_grid(_video_tiles(video, pred_video, history_len), nrow=1, padding=0).cpu()


def make_video_u8(video, pred_video, history_len=6, layout='hwc'):
    """make_video as uint8 ((video * 255.) cast toward zero, what _save_video writes) [T, 2 (H + 4), W + 4, 3] ('hwc') or [T, 3, 2 (H + 4), W + 4]
    ('chw'), left on the inputs' device."""
    return egress.video_grid(_video_tiles(video, pred_video, history_len), nrow=1, padding=0, dtype=torch.uint8, layout=layout)


def _steve_tiles(video, soft_video, hard_video):
    return [egress.Img(_f32(video)), egress.Img(_f32(soft_video)), egress.Img(_f32(hard_video))]


def make_steve_video(video, soft_video, hard_video):
    """STEVEMethod._make_video (base_slots/method.py:293-310): videos [T, 3, H, W] in [-1, 1] -> float32 [T, 3, H + 4, 3 (W + 2) + 2] in [0, 1]: per
    frame the original, the Gumbel-softmax reconstruction and the argmax-token reconstruction in one row (make_grid, nrow 3, padding 2); left on the
    inputs' device (the reference's is on the CPU: `.cpu()` it where that matters)."""
    return egress.video_grid(_steve_tiles(video, soft_video, hard_video), nrow=3, padding=2)


def make_steve_video_u8(video, soft_video, hard_video, layout='hwc'):
    """make_steve_video as uint8 ((video * 255.) cast toward zero) [T, H + 4, 3 (W + 2) + 2, 3] ('hwc') or [T, 3, H + 4, 3 (W + 2) + 2] ('chw'), left on
    the inputs' device."""
    return egress.video_grid(_steve_tiles(video, soft_video, hard_video), nrow=3, padding=2, dtype=torch.uint8, layout=layout)


def batch_draw_bbox_u8(imgs, bboxes, pres_masks=None, bbox_width=2):
    """imgs (B, 3, H, W) in [-1, 1], bboxes (B, N, 4), pres_masks None or (B, N) -> uint8 (B, 3, H, W): torch.round(to_rgb(imgs) * 255) with the
    boxes that are present and not padded (x0 >= 0) outlined, the k-th surviving box in PALETTE[k]; left on the images' device."""
    imgs = _f32(imgs)
    u8 = egress.frames_to_uint8(imgs, to_rgb=True, layout='chw', rounding='nearest')
    bboxes = _f32(bboxes).to(imgs.device)
    if pres_masks is not None:
        pres_masks = pres_masks.to(imgs.device).bool().contiguous()
    return egress.draw_boxes_(u8, bboxes, pres_masks, width=bbox_width)


def draw_bbox(img, bbox, bbox_width=2):
    """One image with its boxes outlined.  img (3, H, W) in [-1, 1], bbox (N, 4) -> float (3, H, W) in [-1, 1] after the round to uint8 and back."""
    return batch_draw_bbox_u8(img[None], bbox[None], bbox_width=bbox_width)[0].float() / 255. * 2. - 1.


def batch_draw_bbox(imgs, bboxes, pres_masks=None, bbox_width=2):
    """Every image with its own boxes outlined; boxes that `pres_masks` marks absent or that are padded (x0 < 0) are left out.
    imgs (B, 3, H, W), bboxes (B, N, 4), pres_masks (B, N) -> float (B, 3, H, W) in [-1, 1] on the CPU (one download, of the uint8 frames)."""
    return batch_draw_bbox_u8(imgs, bboxes, pres_masks, bbox_width).cpu().float() / 255. * 2. - 1.


def slot_decomposition_grid(imgs, recon_combined, recons, masks, scale=1., dtype=torch.float32, layout='chw'):
    """SAViMethod._make_video_grid (base_slots/method.py:102-131) without the PHYRE pause, which callers prepend: per frame the image, the
    reconstruction and every slot `recons * masks + (1 - masks) * scale` in one row, pad_value 1 - scale.  imgs, recon_combined [T, 3, H, W], recons
    [T, N, 3, H, W], masks [T, N, 1, H, W] -> [T, 3, H + 4, (N + 2) (W + 2) + 2] float32 in [0, 1], or with dtype=torch.uint8 the bytes a writer
    takes ('chw', or 'hwc' [T, H + 4, (N + 2) (W + 2) + 2, 3]); left on the inputs' device."""
    tiles = [egress.Img(_f32(imgs)), egress.Img(_f32(recon_combined)), egress.Slots(_f32(recons), _f32(masks), scale)]
    return egress.video_grid(tiles, nrow=recons.shape[1] + 2, padding=2, pad_value=1. - scale, dtype=dtype, layout=layout)
