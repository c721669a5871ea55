"""Warp batches in their compact form (the warp half).

The reference's `WarpDataset.__getitem__` (datasets/warp_dataset.py:139-183) builds, per sample and on the host, two 19-channel
float one-hot cloth maps -- the input one augmented channel by channel with up to four PIL resamplings each -- resizes both to the
load size, normalises and bilinearly resizes the body image, and crops all three.  Here a sample stays what it is after decoding -- a
uint8 HWC body image and the uint8 label maps -- and ONE device launch (swn_op_warp_batch / swn_model_set_input_warp_batch) writes
everything the model reads.  The augmentation PARAMETERS are drawn on the host exactly like `gpu_augment.GpuPerChannelTransform`
draws them (the same `random` calls in the same order as torchvision's transforms make) and travel as its map table.

    wb = GpuWarpBatch(opt)
    batch = wb.collate([{"body_u8": ..., "target_labels_u8": ..., "paths": (cloth, body)}, ...])
    model.set_input(batch)                 # WarpModel: one launch, about 10 MB instead of 343 MB cross PCIe at bs 32, 256 x 256
    reference_form = wb.expand(batch)      # the dict the reference's DataLoader would have collated, on the device

A sample without "input_labels_u8" takes its target map as the input (--dataset_mode image, and inference); in video mode the
dataset picks another frame's map and passes it.  What stays on the host: the PIL decode of the body and the .npz decompression.
Exactness is that of gpu_augment: flips and RandomAffine are bit-identical to the per-channel PIL calls; RandomPerspective is
resampled NEAREST by default, and with `perspective_resample="bicubic"` (opt-in: `opt.perspective_resample` or the keyword) BICUBIC
like torchvision 0.4.0 does, bit-identical to Pillow given the same coefficients -- what remains unpinned is torchvision's float32
least-squares fit of them (the one documented deviation); the body is torch's published bilinear
formula in fp32, one rounded operation per step (torch's own vectorised CPU kernel differs from that by a few ulp, and from
itself between thread counts).  The maps of a batch are drawn after all its samples were loaded, sample-major and channel-minor:
the order a single-worker reference loader consumes `random` in image mode.
"""
import random

import numpy as np
import torch

from .. import engine
from .gpu_augment import GpuPerChannelTransform, check_perspective_resample, has_bicubic
from .gpu_texture_batch import GpuTextureBatch


def expand_batch(ctx, batch, cloth_channels=19, targets=True):
    """Compact batch -> the reference-form dict (tensors on the context's device), through swn_op_warp_batch (swn_op_warp_batch_ex
    where the batch carries perspective_resample "bicubic")."""
    x_min, y_min, width, height = batch["crop"]
    mean, std = batch["norm_stats"]
    bodys, inputs, tgts = engine.op_warp_batch(ctx, batch["bodys_u8"], batch["input_labels_u8"], batch["target_labels_u8"] if targets else None,
                                               batch.get("maps"), mean, std, batch["load_size"], x_min, y_min, height, width, cloth_channels,
                                               bicubic=engine.warp_batch_bicubic(batch))
    out = {"body_paths": batch["body_paths"], "bodys": bodys, "cloth_paths": batch["cloth_paths"], "input_cloths": inputs}
    if targets:
        out["target_cloths"] = tgts
    return out


class GpuWarpBatch:
    """Collates warp samples in compact form.  `opt` carries the reference's options: `input_transforms` ("none", "hflip", "vflip",
    "affine", "perspective", "all"), `load_size`, `crop_size` / `crop_bounds`, `body_norm_stats`, `cloth_channels` and `is_train`
    (an inference batch is not augmented, warp_dataset.py:114-116), and `perspective_resample` ("nearest", the default, or "bicubic")
    where present; the keyword of the same name overrides it."""

    _parse_crop_bounds = staticmethod(GpuTextureBatch._parse_crop_bounds)

    def __init__(self, opt, ctx=None, rng=random, perspective_resample=None):
        self.opt, self.ctx, self.rng = opt, ctx, rng
        self.is_train = bool(getattr(opt, "is_train", True))
        if perspective_resample is None:
            perspective_resample = getattr(opt, "perspective_resample", "nearest")
        self.perspective_resample = check_perspective_resample(perspective_resample)
        self.transform = GpuPerChannelTransform(getattr(opt, "input_transforms", "none"), rng=rng, perspective_resample=perspective_resample)
        self.load_size = int(opt.load_size)
        self.crop_bounds = self._parse_crop_bounds(opt)
        self.cloth_channels = int(getattr(opt, "cloth_channels", 19))
        mean, std = opt.body_norm_stats
        self.norm_stats = (tuple(float(v) for v in mean), tuple(float(v) for v in std))

    def collate(self, samples, maps=None):
        """samples: dicts {body_u8 (Hb,Wb,3) uint8 = the decoded RGB body image, target_labels_u8 (Hl,Wl) uint8 = the stored cloth
        label map, optional input_labels_u8 (Hl,Wl) uint8 = the map to augment when it is another one (video mode), paths
        (cloth_path, body_path)}.  maps: a (B, cloth_channels, nmaps, 9) table to use instead of drawing one (kind 3 in it needs
        perspective_resample "bicubic": a ValueError otherwise).  A bicubic batch carries the choice as "perspective_resample"."""
        n = len(samples)
        bodys = [np.asarray(s["body_u8"], dtype=np.uint8) for s in samples]
        tgts = [np.asarray(s["target_labels_u8"], dtype=np.uint8) for s in samples]
        own_input = [s.get("input_labels_u8") is not None for s in samples]
        if any(a.ndim != 3 or a.shape != bodys[0].shape or a.shape[2] != 3 for a in bodys):
            raise ValueError("warp batch: bodies of one batch must all be (Hb, Wb, 3) of one size, got %s" % [a.shape for a in bodys])
        if any(a.ndim != 2 or a.shape != tgts[0].shape for a in tgts):
            raise ValueError("warp batch: label maps of one batch must share one size, got %s" % [a.shape for a in tgts])
        if any(own_input) != all(own_input):
            raise ValueError("warp batch: either every sample of a batch carries input_labels_u8 or none does")
        target = torch.from_numpy(np.stack(tgts))
        if own_input[0]:
            ins = [np.asarray(s["input_labels_u8"], dtype=np.uint8) for s in samples]
            if any(a.shape != tgts[0].shape for a in ins):
                raise ValueError("warp batch: input label maps must have the targets' size, got %s" % [a.shape for a in ins])
            inputs = torch.from_numpy(np.stack(ins))
        else:
            inputs = target                  # the same tensor: handed over once, read twice
        hl, wl = tgts[0].shape
        if maps is None and self.is_train and self.transform.transforms:
            maps = self.transform.draw_maps(n, self.cloth_channels, wl, hl)
        if maps is not None:
            maps = np.ascontiguousarray(maps, dtype=np.float64).reshape(n, self.cloth_channels, -1, 9)
            if has_bicubic(maps) and self.perspective_resample != "bicubic":
                raise ValueError("warp batch: the map table holds kind 3 (bicubic perspective) but perspective_resample is %r"
                                 % (self.perspective_resample,))
            maps = torch.from_numpy(maps)
        if self.crop_bounds:
            (x_min, y_min), (x_max, y_max) = self.crop_bounds
            crop = (int(x_min), int(y_min), int(x_max - x_min), int(y_max - y_min))
        else:
            crop = (0, 0, self.load_size, self.load_size)
        batch = {"bodys_u8": torch.from_numpy(np.stack(bodys)), "input_labels_u8": inputs, "target_labels_u8": target, "maps": maps,
                 "load_size": self.load_size, "crop": crop, "norm_stats": self.norm_stats,
                 "cloth_paths": [s["paths"][0] for s in samples], "body_paths": [s["paths"][1] for s in samples]}
        if self.perspective_resample != "nearest":       # (a batch without the key is a "nearest" one: the default form is unchanged)
            batch["perspective_resample"] = self.perspective_resample
        return batch

    def expand(self, batch):
        return expand_batch(self.ctx or engine.default_context(), batch, self.cloth_channels)
