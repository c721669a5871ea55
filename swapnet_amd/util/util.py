"""The few host-side helpers of the reference that its models call on display ticks
(/root/reference/datasets/data_utils.py:41-90, util/util.py): not on the hot path."""
import os

import numpy as np


def unnormalize(tensor, mean, std, clamp=True, inplace=False):
    """datasets/data_utils.py:41-58 (note the reference compares `tensor.shape == 4`, which is
    never true, so the per-channel loop always runs over dim 0 -- reproduced)."""
    if not inplace:
        tensor = tensor.clone()
    for t, m, s in zip(tensor, mean, std):
        t.mul_(s).add_(m)
        if clamp:
            t.clamp_(0, 1)
    return tensor


def scale_tensor(tensor, scale_each=False, range=None):
    """datasets/data_utils.py:61-90 (torchvision.utils.make_grid's normalisation)."""
    tensor = tensor.clone()

    def norm_ip(img, lo, hi):
        img.clamp_(min=lo, max=hi)
        img.add_(-lo).div_(hi - lo + 1e-5)

    def norm_range(t):
        if range is not None:
            norm_ip(t, range[0], range[1])
        else:
            norm_ip(t, float(t.min()), float(t.max()))

    if scale_each:
        for t in tensor:
            norm_range(t)
    else:
        norm_range(tensor)
    return tensor


def tensor2im(input_image, imtype=np.uint8, *, ctx=None):
    """util/util.py:9-32 with its signature: the FIRST image of a batch as an (H,W,3) array.  A float
    tensor takes the device path (engine.op_image_u8: (x + 1) / 2 * 255, grayscale replicated, cast like numpy's wherever that is
    defined and saturating elsewhere); a numpy array passes through as the reference's does (first of a 4-d batch, astype); a uint8
    tensor returns its own bytes as HWC (the reference pushes them through the float formula, which wraps: not reproduced); anything
    else is handed back untouched."""
    import torch
    if isinstance(input_image, np.ndarray):
        if len(input_image.shape) == 4:
            input_image = input_image[0]
        return input_image.astype(imtype)
    if not isinstance(input_image, torch.Tensor):
        return input_image
    first = input_image.detach()[0:1]
    if first.dtype == torch.uint8:
        image = first[0].cpu()
        if image.shape[0] == 1:
            image = image.expand(3, -1, -1)
        return image.permute(1, 2, 0).contiguous().numpy().astype(imtype)
    from .. import engine
    ctx = ctx or engine.default_context()
    return engine.op_image_u8(ctx, first.float())[0].cpu().numpy().astype(imtype)


class PromptOnce:
    @staticmethod
    def makedirs(path, confirm=False):
        os.makedirs(path, exist_ok=True)
