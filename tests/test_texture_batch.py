"""SURVEY.md 8(f) rank 3, the texture half: a texture batch handed over in compact form -- uint8 HWC images, uint8 label maps, the
raw ROI table, five scalars per sample -- and expanded into every model slot by ONE device launch (csrc/texture_batch.hip; the
host loop of engine.cpp on the simulator).  The oracle is the host chain of the reference's TextureDataset.__getitem__
(datasets/texture_dataset.py:87-160, datasets/data_utils.py:169-295), written out below with Pillow, torch and numpy.  Every
comparison is an equality: each step is an integer gather or one correctly rounded fp32 operation."""
import argparse
import functools
import random
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from oracle import swapnet_oracle as O
from swapnet_amd import engine
from swapnet_amd.datasets import gpu_texture_batch as TB
from tests import backends

BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]

# the texture statistics of the reference's README (norm_stats.json of its DeepFashion preparation)
MEAN = (0.8319639705048438, 0.8105952930426163, 0.8038053056173073)
STD = (0.22878186598352074, 0.245635337367858, 0.2517315913036158)
FLIPS = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=np.float32)          # (vflip, hflip): the four combinations


def _ctx(kind):
    return backends.gpu_ctx() if kind == "gpu" else backends.hostsim_ctx()


# ---- the reference chain, in this file's own words ---------------------------------------------------------------------------
def ref_texture(pil):
    t = torch.from_numpy(np.asarray(pil).copy()).permute(2, 0, 1).contiguous().float().div(255)       # tf.to_tensor
    mean, std = torch.tensor(MEAN, dtype=torch.float32), torch.tensor(STD, dtype=torch.float32)
    return t.sub(mean[:, None, None]).div(std[:, None, None])                                        # transforms.Normalize


def ref_onehot(labels, C):
    lab = torch.from_numpy(labels.astype(np.int64))
    out = torch.zeros((C,) + tuple(lab.shape), dtype=torch.float32)
    fg = (lab > 0) & (lab < C)
    out.scatter_(0, lab.clamp(0, C - 1)[None], fg[None].float())                                     # label 0: the all-zero vector
    return out


def ref_flip_rois(rois, first, second, center):
    """flip_rois_: (values - center) * -1 + center on both columns, which then swap."""
    a, b = rois[:, first].clone(), rois[:, second].clone()
    rois[:, first] = (b - center) * -1 + center
    rois[:, second] = (a - center) * -1 + center


def ref_sample(img_u8, labels, rois_raw, vflip, hflip, scale, original_size, crop, C):
    """One __getitem__: (input_texture, target_texture, cloth, rois, rois before the crop, the scaled ROIs before rounding)."""
    Hs, Ws = img_u8.shape[:2]
    pil = Image.fromarray(img_u8)
    target = ref_texture(pil)
    flipped = pil
    if vflip:
        flipped = flipped.transpose(Image.FLIP_TOP_BOTTOM)
    if hflip:
        flipped = flipped.transpose(Image.FLIP_LEFT_RIGHT)
    inp = ref_texture(flipped)
    cloth = F.interpolate(ref_onehot(labels, C)[None], size=(Hs, Ws))[0]
    scaled = rois_raw * scale                                   # float32 rows * a Python float: a float32 product
    assert scaled.dtype == np.float32
    rois = torch.from_numpy(np.rint(scaled))
    W0, H0 = original_size
    if vflip:
        ref_flip_rois(rois, 1, 3, int(H0 / 2))
    if hflip:
        ref_flip_rois(rois, 0, 2, int(W0 / 2))
    uncropped = rois.clone()
    if crop is not None:
        (x_min, y_min), (x_max, y_max) = crop
        inp, cloth, target = (t[:, y_min:y_max, x_min:x_max] for t in (inp, cloth, target))
        xs = torch.clamp(rois[:, [0, 2]], x_min, x_max - 1) - x_min
        ys = torch.clamp(rois[:, [1, 3]], y_min, y_max - 1) - y_min
        rois = torch.stack((xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1]), 1)
    return inp, target, cloth, rois, uncropped, scaled


# raw ROI rows (x1, y1, x2, y2) as the CSV holds them, in the pixels of an original twice the source's size (scale 0.5)
ROI_ROWS = np.array([
    [0, 0, 0, 0],            # "None" in the CSV
    [10, 10, 10, 10],        # degenerate box
    [1, 3, 5, 7],            # ties after scaling by 0.5: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    [0, 8, 12, 20],          # left of the crop window
    [10, 0, 20, 16],         # above it
    [12, 8, 44, 20],         # right of it
    [10, 8, 20, 44],         # below it
    [8, 6, 30, 24], [14, 10, 22, 18], [7, 9, 33, 27], [16, 12, 17, 13], [9, 5, 21, 25]], dtype=np.float32)
# (W0, H0) of the originals: none equals the 19 x 23 source, so cy, cx are not the source's centre; scales 0.5, 1/3, 1, 0.5
ORIGINALS = [(38, 46), (57, 69), (19, 25), (38, 40)]


@functools.lru_cache(maxsize=None)
def op_case(Hl, Wl, cropped, C):
    """Compact arrays of one B = 4 case on the 23 x 19 source and its reference tensors (computed once, shared, never changed)."""
    B, Hs, Ws = 4, 23, 19
    g = np.random.RandomState(100 * Hl + 10 * C + cropped)
    img = g.randint(0, 256, (B, Hs, Ws, 3)).astype(np.uint8)
    img[0, 0, 0], img[0, 0, 1] = 0, 255                         # both ends of the byte range are present
    labels = g.randint(0, C, (B, Hl, Wl)).astype(np.uint8)
    rois_raw = np.stack([ROI_ROWS] * B)
    crop = ((3, 2), (3 + 16, 2 + 12)) if cropped else None
    sample = np.zeros((B, 5), dtype=np.float32)
    ref = []
    for b in range(B):
        W0, H0 = ORIGINALS[b]
        scale = float(Ws) / W0                                   # load_size / original width
        sample[b] = (FLIPS[b, 0], FLIPS[b, 1], scale, int(H0 / 2), int(W0 / 2))
        ref.append(ref_sample(img[b], labels[b], rois_raw[b], FLIPS[b, 0], FLIPS[b, 1], scale, ORIGINALS[b], crop, C))
    inp, tgt, cloth, rois, uncropped, scaled = (torch.stack([torch.as_tensor(r[i]) for r in ref]) for i in range(6))
    window = (3, 2, 16, 12) if cropped else (0, 0, Ws, Hs)
    return dict(img=img, labels=labels, rois_raw=rois_raw, sample=sample, window=window, C=C, inp=inp, tgt=tgt, cloth=cloth, rois=rois,
                uncropped=uncropped, scaled=scaled)


OP_CASES = [(hl, wl, cropped, C) for (hl, wl) in ((11, 13), (40, 31)) for cropped in (1, 0) for C in (19, 5, 4)]


def test_the_reference_chain_covers_the_roi_edge_cases():
    """On the reference chain alone: at least one box is clamped by the crop on every side, at least one scaled coordinate is a
    tie, ties round both ways, and the flip centres are not the source's."""
    c = op_case(11, 13, 1, 19)
    x_min, y_min, W, H = c["window"]
    u = c["uncropped"]
    assert (u[..., [0, 2]] < x_min).any() and (u[..., [0, 2]] > x_min + W - 1).any()
    assert (u[..., [1, 3]] < y_min).any() and (u[..., [1, 3]] > y_min + H - 1).any()
    assert not torch.equal(c["rois"], u - torch.tensor([x_min, y_min, x_min, y_min], dtype=torch.float32))
    s = c["scaled"][0]                                          # sample 0: scale 0.5
    ties = (s - torch.floor(s)) == 0.5
    assert ties.any()
    assert s[2].tolist() == [0.5, 1.5, 2.5, 3.5] and c["uncropped"][0, 2].tolist() == [0.0, 2.0, 2.0, 4.0]       # down, up, down, up
    assert all((int(h0 / 2), int(w0 / 2)) != (23 // 2, 19 // 2) for w0, h0 in ORIGINALS)
    # without a crop the reference leaves ROIs outside the image as they are
    n = op_case(11, 13, 0, 19)
    assert (n["rois"] > 22).any() and torch.equal(n["rois"], n["uncropped"])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("Hl,Wl,cropped,C", OP_CASES)
def test_op_is_bit_identical_to_the_reference_chain(backend, Hl, Wl, cropped, C):
    ctx = _ctx(backend)
    c = op_case(Hl, Wl, cropped, C)
    x_min, y_min, W, H = c["window"]
    inp, tgt, cloth, rois = engine.op_texture_batch(ctx, c["img"], c["labels"], c["rois_raw"], c["sample"], MEAN, STD, x_min, y_min, H, W, C)
    for name, got in (("inp", inp), ("tgt", tgt), ("cloth", cloth), ("rois", rois)):
        got, want = got.cpu(), c[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        assert torch.equal(got, want), (name, int((got != want).sum()), float((got - want).abs().max()))


@pytest.mark.parametrize("src,dst", [(300, 256), (512, 256), (200, 256), (256, 256), (97, 64)])
def test_pillow_resize_commutes_with_the_flips(src, dst):
    """The reference flips the original image and resizes it a second time (texture_dataset.py:129-134); the compact form
    flips the RESIZED image.  Pillow's bilinear resize (tf.resize's default) gives the same bytes either way, on both axes."""
    g = np.random.RandomState(src)
    for h, w in ((src, src), (src, src + 37)):                      # square, and wider than high (tf.resize keeps the aspect ratio)
        img = Image.fromarray(g.randint(0, 256, (h, w, 3)).astype(np.uint8))
        size = (dst * w // h, dst) if w > h else (dst, dst)         # (width, height): the smaller edge becomes dst
        for flips in ([Image.FLIP_TOP_BOTTOM], [Image.FLIP_LEFT_RIGHT], [Image.FLIP_TOP_BOTTOM, Image.FLIP_LEFT_RIGHT]):
            a = b = img
            for f in flips:
                a = a.transpose(f)
            a = a.resize(size, Image.BILINEAR)
            b = b.resize(size, Image.BILINEAR)
            for f in flips:
                b = b.transpose(f)
            assert np.array_equal(np.asarray(a), np.asarray(b)), (src, dst, (h, w), flips)


# ---- model hand-over -----------------------------------------------------------------------------------------------------------
def _originals(Hs):
    return [(Hs + 2, Hs + 5), (Hs + 6, Hs + 2)]                     # (W0, H0)


@functools.lru_cache(maxsize=None)
def model_case(Hs, cropped):
    """B = 2 at 64 x 64 (the smallest the U-Net accepts): compact batch dict + the reference tensors."""
    B, C, R = 2, 19, 12
    g = np.random.RandomState(Hs)
    img = g.randint(0, 256, (B, Hs, Hs, 3)).astype(np.uint8)
    Hl, Wl = (40, 44) if cropped else (100, 90)
    labels = (g.randint(0, C, (B, Hl // 4 + 1, Wl // 4 + 1)).repeat(4, 1).repeat(4, 2)[:, :Hl, :Wl]).astype(np.uint8)
    rois_raw = np.sort(g.randint(0, Hs, (B, R, 2, 2)), axis=2).reshape(B, R, 4).astype(np.float32)       # (x1, y1) <= (x2, y2)
    rois_raw[:, 0] = 0
    crop = ((4, 4), (68, 68)) if cropped else None
    # originals a little larger than the source: the boxes stay mostly inside the image when they flip about the original's centre
    originals, flips = _originals(Hs), [(1, 1), (0, 1)]
    sample = np.zeros((B, 5), dtype=np.float32)
    ref = []
    for b in range(B):
        W0, H0 = originals[b]
        scale = float(Hs) / W0
        sample[b] = (flips[b][0], flips[b][1], scale, int(H0 / 2), int(W0 / 2))
        ref.append(ref_sample(img[b], labels[b], rois_raw[b], flips[b][0], flips[b][1], scale, originals[b], crop, C))
    inp, tgt, cloth, rois = (torch.stack([r[i] for r in ref]) for i in range(4))
    compact = {"textures_u8": torch.from_numpy(img), "cloth_labels_u8": torch.from_numpy(labels), "rois_raw": torch.from_numpy(rois_raw),
               "sample_params": torch.from_numpy(sample), "crop": (4, 4, 64, 64) if cropped else (0, 0, 64, 64), "norm_stats": (MEAN, STD),
               "cloth_paths": ["c0", "c1"], "texture_paths": ["t0", "t1"]}
    return compact, (inp, rois, cloth, tgt)


@functools.lru_cache(maxsize=None)
def texture_weights():
    from tests.test_texture_step import vgg_state_dict
    torch.manual_seed(21)
    return O.texture_module_params(img_size=64), O.patchgan_params(22), O.vgg16_feature_params(), vgg_state_dict


def _poison(m):
    """Other values in every input slot, so that a slot the hand-over under test fails to write cannot pass by inheritance."""
    tex, rois, cloth, tgt = O.synth_texture_batch(2, 64, 64, seed=77)
    for slot, t in enumerate((tex, rois, cloth, tgt)[: 4 if m.is_train else 3]):
        m.set_input(slot, t)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("Hs,cropped", [(72, 1), (64, 0)])
def test_model_handover_equals_the_four_set_input_calls(backend, Hs, cropped):
    ctx = _ctx(backend)
    compact, floats = model_case(Hs, cropped)
    G, D, vgg, vgg_state_dict = texture_weights()
    m = backends.get_model(ctx, "texture", 2, 64)
    state = {engine.NET_G: G, engine.NET_D: D, engine.NET_VGG: vgg_state_dict(m, vgg)}
    runs = []
    for compact_path in (False, True):
        backends.reset_state(m, state)
        _poison(m)
        if compact_path:
            m.set_input_texture_batch(compact)
        else:
            for slot, t in enumerate(floats):
                m.set_input(slot, t)
        m.forward(False, 0)
        taps = [m.tap(engine.NET_G, "unet_in").cpu(), m.tap(engine.NET_G, "pooled").cpu(), m.output().cpu()]
        m.step([0.9, 0.8, 1.0], training=True, seed=3)
        ctx.sync()
        runs.append((taps, m.losses(), m.grad_arena(engine.NET_D).cpu().clone()))
    (ta, la, ga), (tb, lb, gb) = runs
    for name, a, b in zip(("unet_in", "pooled", "fakes"), ta, tb):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert torch.equal(ta[0][:, 36:55], floats[2])                  # the cloth channels of the U-Net input ARE the reference one-hot
    assert la == lb, (la, lb)
    assert torch.equal(ga, gb) and float(ga.abs().sum()) > 0
    # an inference model takes the same call (it has no target slot and no second discriminator half to write)
    mi = backends.get_model(ctx, "texture", 2, 64, is_train=False)
    mi.load_state_dict(engine.NET_G, G)
    outs = []
    for compact_path in (False, True):
        _poison(mi)
        if compact_path:
            mi.set_input_texture_batch(compact)
        else:
            for slot, t in enumerate(floats[:3]):
                mi.set_input(slot, t)
        mi.forward(False, 0)
        outs.append(mi.output().cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], ta[2])


# ---- Python surface ------------------------------------------------------------------------------------------------------------
def _opt(**kw):
    o = dict(input_transforms=("hflip", "vflip"), load_size=72, crop_size=64, crop_bounds=None, texture_norm_stats=(MEAN, STD),
             cloth_channels=19)
    o.update(kw)
    return argparse.Namespace(**o)


def test_draw_replays_the_reference_rng_call_for_call():
    tb = TB.GpuTextureBatch(_opt(), rng=random.Random(7))
    flags = tb.draw(5)
    r = random.Random(7)
    want = [[float(r.random() < 0.5), float(r.random() < 0.5)] for _ in range(5)]          # vertical first, two draws per sample
    assert flags.tolist() == want and 0 < flags.sum() < 10
    assert tb.rng.random() == r.random()
    # probability 0 still draws twice per sample (random_image_roi_flip compares random.random() < 0)
    rng = random.Random(7)
    none = TB.GpuTextureBatch(_opt(input_transforms="none"), rng=rng)
    assert none.draw(5).tolist() == [[0.0, 0.0]] * 5
    r = random.Random(7)
    for _ in range(10):
        r.random()
    assert rng.random() == r.random()
    only_h = TB.GpuTextureBatch(_opt(input_transforms=["hflip"]), rng=random.Random(7))
    assert only_h.draw(5)[:, 0].sum() == 0 and only_h.draw(20)[:, 1].sum() > 0
    assert TB.GpuTextureBatch(_opt(input_transforms="all")).vp == 0.5
    assert tb.crop_bounds == ((4, 4), (68, 68)) and TB.GpuTextureBatch(_opt(load_size=64)).crop_bounds is None
    assert TB.GpuTextureBatch(_opt(load_size=64, crop_bounds="((1, 2), (33, 34))")).crop_bounds == ((1, 2), (33, 34))


def _samples(Hs, cropped):
    compact, _ = model_case(Hs, cropped)
    originals = _originals(Hs)
    return [{"image_u8": compact["textures_u8"][b].numpy(), "labels_u8": compact["cloth_labels_u8"][b].numpy(),
             "rois_raw": compact["rois_raw"][b].numpy(), "original_size": originals[b], "paths": ("c%d" % b, "t%d" % b)} for b in range(2)]


@pytest.mark.parametrize("backend", BACKENDS)
def test_collate_and_expand_give_the_reference_form(backend):
    ctx = _ctx(backend)
    compact, floats = model_case(72, 1)
    tb = TB.GpuTextureBatch(_opt(), ctx=ctx)
    batch = tb.collate(_samples(72, 1), flips=[(1, 1), (0, 1)])
    for k in ("textures_u8", "cloth_labels_u8", "rois_raw", "sample_params"):
        assert torch.equal(batch[k], compact[k]) and batch[k].dtype == compact[k].dtype, k
    assert batch["crop"] == compact["crop"] and batch["cloth_paths"] == ["c0", "c1"] and batch["texture_paths"] == ["t0", "t1"]
    ref = tb.expand(batch)
    for k, want in zip(("input_textures", "rois", "cloths", "target_textures"), floats):
        assert torch.equal(ref[k].cpu(), want), k


@pytest.mark.small_channel_winograd
@pytest.mark.parametrize("backend", BACKENDS)
def test_create_model_trains_on_a_compact_batch_like_on_its_expansion(backend, tmp_path):
    from swapnet_amd.models import create_model
    from tests.test_models_api import make_opt
    compact, floats = model_case(72, 1)
    losses, models = [], []
    for form in ("compact", "reference"):
        opt = make_opt(tmp_path, backend, model="texture", texture_norm_stats=(MEAN, STD), load_size=72, input_transforms=("hflip", "vflip"))
        torch.manual_seed(11)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)         # (seeded-random VGG16 where no pretrained weights are at hand)
            model = create_model(opt)
        model.eval()
        tb = TB.GpuTextureBatch(opt, ctx=model.backend.ctx)
        model.set_input(compact if form == "compact" else tb.expand(compact))
        torch.manual_seed(5)
        model.optimize_parameters()
        losses.append(model.get_current_losses())
        models.append(model)
    assert losses[0] == losses[1] and all(np.isfinite(v) for v in losses[0].values()), losses
    assert torch.equal(models[0].fakes.cpu(), models[1].fakes.cpu())
    m = models[0]
    assert m.get_image_paths() == (("c0", "t0"), ("c1", "t1"))
    assert m._textures is None                                   # nothing was expanded on the training path
    m.compute_visuals()
    vis = m.get_current_visuals()
    assert set(vis) == {"textures_unnormalized", "cloths_decoded", "fakes", "fakes_scaled", "targets_unnormalized"}
    assert torch.equal(m.textures.cpu(), floats[0]) and torch.equal(m.targets.cpu(), floats[3]) and torch.equal(m.cloths.cpu(), floats[2])
    assert torch.equal(vis["cloths_decoded"].cpu(), O.decode_cloth_labels(floats[2]))
    # ... and the float hand-over afterwards is today's path: plain attributes again
    models[0].set_input(tb.expand(compact))
    assert models[0]._compact is None and torch.equal(models[0].textures.cpu(), floats[0])


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    ctx = _ctx(backend)
    c = op_case(11, 13, 1, 19)
    args = (c["img"], c["labels"], c["rois_raw"], c["sample"], MEAN, STD)
    for x_min, y_min, H, W in ((4, 2, 12, 16), (3, 12, 12, 16), (-1, 0, 12, 16), (0, 0, 24, 19)):       # 23 x 19 source
        with pytest.raises(ValueError, match="crop window"):
            engine.op_texture_batch(ctx, *args, x_min, y_min, H, W, 19)
    with pytest.raises(ValueError, match="cloth channels"):
        engine.op_texture_batch(ctx, *args, 3, 2, 12, 16, 65)
    compact, _ = model_case(72, 1)
    warp = backends.get_model(ctx, "warp", 2, 64, is_train=False)
    with pytest.raises(ValueError, match="only the texture model"):
        warp.set_input_texture_batch(compact)
    m = backends.get_model(ctx, "texture", 2, 64, is_train=False)
    with pytest.raises(ValueError, match="num_roi"):
        m.set_input_texture_batch(dict(compact, rois_raw=compact["rois_raw"][:, :5]))
    with pytest.raises(ValueError, match="crop window"):
        m.set_input_texture_batch(dict(compact, crop=(9, 4, 64, 64)))            # 9 + 64 > 72
    with pytest.raises(ValueError, match="batch"):
        m.set_input_texture_batch({k: (v[:1] if torch.is_tensor(v) else v) for k, v in compact.items()})
    samples = _samples(72, 1)
    samples[1] = dict(samples[1], labels_u8=samples[1]["labels_u8"][:-1])
    with pytest.raises(ValueError, match="label maps"):
        TB.GpuTextureBatch(_opt()).collate(samples)
