"""Texture batches in their compact form (the texture half).

The reference's `TextureDataset.__getitem__` (datasets/texture_dataset.py:87-160, datasets/data_utils.py:169-295)
builds, per sample and on the host, two normalised float32 copies of the same image (the target and its randomly flipped
twin), a 19-channel float one-hot cloth map resized to the load size, and the ROI table rescaled, flipped and cropped.  Here a
sample stays what it is on disk plus one PIL resize -- a uint8 HWC image, the uint8 label map, the raw ROI rows -- and ONE device
launch (swn_op_texture_batch / swn_model_set_input_texture_batch) writes everything the model reads, bit-identical to that
chain.  The random flip DECISIONS are drawn on the host exactly like `random_image_roi_flip` draws them.

    tb = GpuTextureBatch(opt)
    batch = tb.collate([{"image_u8": ..., "labels_u8": ..., "rois_raw": ..., "original_size": (W0, H0), "paths": (cloth, texture)}, ...])
    model.set_input(batch)                 # TextureModel: one launch, no float tensors cross PCIe
    reference_form = tb.expand(batch)      # the dict the reference's DataLoader would have collated, on the device

What stays on the host: the PIL decode and `tf.resize(img, load_size)` -- or the decode alone: a sample may carry `source_u8`, the
decoded image at its own size, instead of `image_u8` + `original_size`, and Pillow's bilinear resize then runs on the device as
well, byte for byte (swn_op_resize_u8 / swn_model_set_input_texture_sources; tests/test_texture_sources.py).  The reference flips
the ORIGINAL image and resizes it a second time; here the resized image is flipped.  Pillow's resize commutes with both flips bit
for bit (tests/test_texture_batch.py pins that).  The ROIs flip about the centre of the ORIGINAL image, as in the reference (`random_image_roi_flip` receives the
un-resized PIL image): that centre travels per sample.
"""
import ast
import random

import numpy as np
import torch

from .. import engine


def tv_resize_size(w, h, size):
    """(width, height) after torchvision 0.4.0's `resize(img, size)` of a w x h image (functional.py resize): an int matches the
    SMALLER edge and keeps the aspect ratio, the other edge truncated; nothing changes if the smaller edge already has that length;
    a (h, w) pair is taken as is."""
    if not isinstance(size, int):
        oh, ow = size
        return int(ow), int(oh)
    if (w <= h and w == size) or (h <= w and h == size):
        return w, h
    if w < h:
        return size, int(size * h / w)
    return int(size * w / h), size


def expand_batch(ctx, batch, cloth_channels=19):
    """Compact batch -> the reference-form dict (tensors on the context's device), through swn_op_texture_batch; the sources form
    through swn_op_resize_u8 first."""
    x_min, y_min, width, height = batch["crop"]
    mean, std = batch["norm_stats"]
    if "sources_u8" in batch:
        hs, ws = batch["resized"]
        textures_u8 = engine.op_resize_u8_packed(ctx, batch["sources_u8"], batch["source_geom"], hs, ws)
    else:
        textures_u8 = batch["textures_u8"]
    inp, tgt, cloths, rois = engine.op_texture_batch(ctx, textures_u8, batch["cloth_labels_u8"], batch["rois_raw"],
                                                     batch["sample_params"], mean, std, x_min, y_min, height, width, cloth_channels)
    return {"input_textures": inp, "rois": rois, "cloths": cloths, "target_textures": tgt,
            "cloth_paths": batch["cloth_paths"], "texture_paths": batch["texture_paths"]}


class GpuTextureBatch:
    """Collates texture samples in compact form.  `opt` carries the reference's options: `input_transforms` ("none", "hflip",
    "vflip", "all"), `load_size`, `crop_size` / `crop_bounds`, `texture_norm_stats` and `cloth_channels`."""

    def __init__(self, opt, ctx=None, rng=random):
        self.opt, self.ctx, self.rng = opt, ctx, rng
        t = getattr(opt, "input_transforms", "none")
        t = [t] if isinstance(t, str) else list(t)
        # texture_dataset.py:123-128: the probability is 0.5 if the axis (or "all") is named, else 0
        self.vp = 0.5 if any(k in t for k in ("vflip", "all")) else 0
        self.hp = 0.5 if any(k in t for k in ("hflip", "all")) else 0
        self.load_size = int(opt.load_size)
        self.crop_bounds = self._parse_crop_bounds(opt)
        self.cloth_channels = int(getattr(opt, "cloth_channels", 19))
        mean, std = opt.texture_norm_stats
        self.norm_stats = (tuple(float(v) for v in mean), tuple(float(v) for v in std))

    @staticmethod
    def _parse_crop_bounds(opt):
        """BaseDataset.parse_crop_bounds (datasets/base_dataset.py:51-58): a centred square when crop_size < load_size, else
        the --crop_bounds literal "((x_min, y_min), (x_max, y_max))", else no crop."""
        crop_size, load_size = getattr(opt, "crop_size", None), int(opt.load_size)
        if isinstance(crop_size, int) and crop_size < load_size:
            minimum = int((load_size - crop_size) / 2)
            maximum = load_size - minimum
            return (minimum, minimum), (maximum, maximum)
        cb = getattr(opt, "crop_bounds", None)
        if not cb:
            return None
        return ast.literal_eval(cb) if isinstance(cb, str) else cb

    def draw(self, n):
        """(n, 2) flip flags {vflip, hflip}: `random_image_roi_flip` calls random.random() exactly twice per sample, vertical
        first, also when a probability is 0."""
        flags = np.zeros((n, 2), dtype=np.float32)
        for i in range(n):
            flags[i, 0] = self.rng.random() < self.vp
            flags[i, 1] = self.rng.random() < self.hp
        return flags

    def collate(self, samples, flips=None):
        """samples: dicts {labels_u8 (Hl,Wl) uint8 = the stored cloth label map, rois_raw (R,4) float32 = the ROI table's row block,
        paths (cloth_path, texture_path)} and the image in ONE of two forms, the same for the whole batch:
          image_u8 (Hs,Ws,3) uint8 = the image after tf.resize(img, load_size), with original_size (W0, H0) of the image before it;
          source_u8 (H0,W0,3) uint8 = the DECODED image at its own size: the resize runs on the device (swn_op_resize_u8), to
            tv_resize_size(W0, H0, load_size), which must be one size for the whole batch.
        flips: (n, 2) flags to use instead of drawing them."""
        n = len(samples)
        forms = {("source_u8" in s, "image_u8" in s) for s in samples}
        if forms not in ({(True, False)}, {(False, True)}):
            raise ValueError("texture batch: every sample of one batch carries image_u8 (+ original_size) or every sample source_u8, not a mix")
        from_sources = forms == {(True, False)}
        flips = self.draw(n) if flips is None else np.asarray(flips, dtype=np.float32).reshape(n, 2)
        imgs = [np.asarray(s["source_u8" if from_sources else "image_u8"], dtype=np.uint8) for s in samples]
        labs = [np.asarray(s["labels_u8"], dtype=np.uint8) for s in samples]
        rois = [np.asarray(s["rois_raw"], dtype=np.float32) for s in samples]
        if from_sources:
            if any(a.ndim != 3 or a.shape[2] != 3 for a in imgs):
                raise ValueError("texture batch: sources must be (H0, W0, 3), got %s" % [a.shape for a in imgs])
            originals = [(a.shape[1], a.shape[0]) for a in imgs]
            resized = [tv_resize_size(w0, h0, self.load_size) for w0, h0 in originals]
            if len(set(resized)) != 1:
                raise ValueError("texture batch: the resized sizes (W, H) of one batch differ: %s from the sources %s at load size %d"
                                 % (resized, originals, self.load_size))
            ws, hs = resized[0]
        else:
            if any(a.ndim != 3 or a.shape != imgs[0].shape or a.shape[2] != 3 for a in imgs):
                raise ValueError("texture batch: images of one batch must all be (Hs, Ws, 3) of one size, got %s" % [a.shape for a in imgs])
            hs, ws = imgs[0].shape[:2]
            originals = [s["original_size"] for s in samples]
        if any(a.ndim != 2 or a.shape != labs[0].shape for a in labs):
            raise ValueError("texture batch: label maps of one batch must share one size, got %s" % [a.shape for a in labs])
        if any(a.ndim != 2 or a.shape != rois[0].shape or a.shape[1] != 4 for a in rois):
            raise ValueError("texture batch: ROI tables of one batch must all be (R, 4), got %s" % [a.shape for a in rois])
        params = np.zeros((n, 5), dtype=np.float32)
        params[:, :2] = flips
        for i, (w0, h0) in enumerate(originals):
            params[i, 2] = float(self.load_size) / w0          # texture_dataset.py:116-118 (float32 rows * this scalar, in float32)
            params[i, 3], params[i, 4] = int(h0 / 2), int(w0 / 2)      # data_utils.py:252,257: centres of the ORIGINAL image
        if self.crop_bounds:
            (x_min, y_min), (x_max, y_max) = self.crop_bounds
            crop = (int(x_min), int(y_min), int(x_max - x_min), int(y_max - y_min))
        else:
            crop = (0, 0, ws, hs)
        if from_sources:
            packed, geom = engine.pack_u8_images(imgs)
            images = {"sources_u8": packed, "source_geom": geom, "resized": (hs, ws)}
        else:
            images = {"textures_u8": torch.from_numpy(np.stack(imgs))}
        return dict(images, **{"cloth_labels_u8": torch.from_numpy(np.stack(labs)),
                               "rois_raw": torch.from_numpy(np.stack(rois)), "sample_params": torch.from_numpy(params), "crop": crop,
                               "norm_stats": self.norm_stats, "cloth_paths": [s["paths"][0] for s in samples],
                               "texture_paths": [s["paths"][1] for s in samples]})

    def expand(self, batch):
        return expand_batch(self.ctx or engine.default_context(), batch, self.cloth_channels)
