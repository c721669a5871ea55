"""Texture batches from DECODED images: the `tf.resize(img, load_size)` of the reference's TextureDataset.__getitem__
(datasets/texture_dataset.py:93-95,132-134) -- Pillow's bilinear resize -- as one device launch (csrc/image_resize.hip; the host loop
of engine.cpp on the simulator), and the sources form of the compact texture batch built on it.  The oracle is Pillow itself,
`Image.fromarray(x).resize((Ws, Hs), Image.BILINEAR)`; every comparison is an equality."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from swapnet_amd import engine
from swapnet_amd.datasets import gpu_texture_batch as TB
from tests import backends
from tests.test_texture_batch import BACKENDS, FLIPS, MEAN, ROI_ROWS, STD, _ctx, _opt, _poison, texture_weights


def pillow(x, hs, ws):
    return np.asarray(Image.fromarray(x).resize((ws, hs), Image.BILINEAR))


@functools.lru_cache(maxsize=None)
def pair(h0, w0):
    """The two images of an op case: random bytes with a forced 0 pixel and a forced 255 pixel, and a saturated image."""
    g = np.random.RandomState(1000 * h0 + w0)
    a = g.randint(0, 256, (h0, w0, 3)).astype(np.uint8)
    a[0, 0], a[-1, -1] = 0, 255
    b = ((g.randint(0, 256, (h0, w0, 3)) > 100) * 255).astype(np.uint8)
    return a, b


# (H0, W0) -> (Hs, Ws), one geometry per failure mode
OP_CASES = [((23, 19), (16, 16)),        # non-integer downscale on both axes
            ((19, 23), (32, 40)),        # upscale on both axes
            ((40, 31), (40, 16)),        # horizontal pass only
            ((31, 40), (16, 40)),        # vertical pass only
            ((16, 16), (16, 16)),        # copy
            ((64, 48), (32, 24)),        # exact 2x
            ((5, 7), (16, 16)),          # windows clamped at both edges
            ((1, 9), (4, 4)),            # single-row source
            ((2, 2), (5, 3)),            # 2 x 2 source
            ((75, 141), (37, 70)), ((141, 75), (70, 37)),      # partial tiles on both axes (8 x 32 tiles: 5 x 3 and 9 x 2 of them)
            ((600, 8), (37, 8)), ((8, 600), (8, 37)),          # factor 16.2: 34-tap windows, 130 intermediate rows per tile
            ((310, 62), (10, 2)), ((62, 310), (2, 10))]        # factor 31, the stated bound: 63-tap windows, 280 intermediate rows


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("src,dst", OP_CASES, ids=lambda s: "%dx%d" % s)
def test_op_equals_pillow(backend, src, dst):
    ctx = _ctx(backend)
    imgs = pair(*src)
    got = engine.op_resize_u8(ctx, list(imgs), *dst)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2,) + dst + (3,)
    got = got.cpu().numpy()
    for i, x in enumerate(imgs):
        want = pillow(x, *dst)
        assert np.array_equal(got[i], want), (src, dst, i, int((got[i] != want).sum()))


@pytest.mark.parametrize("backend", BACKENDS)
def test_mixed_sizes_in_one_batch(backend):
    """Three sizes packed back to back (odd offsets: 23 * 19 * 3 = 1311 bytes, then 3720 more), one launch, one output size."""
    ctx = _ctx(backend)
    imgs = [pair(23, 19)[0], pair(40, 31)[0], pair(16, 16)[0]]
    packed, geom = engine.pack_u8_images(imgs)
    assert geom.tolist() == [[0, 23, 19], [1311, 40, 31], [5031, 16, 16]] and packed.numel() == 5031 + 768
    got = engine.op_resize_u8(ctx, imgs, 16, 16).cpu().numpy()
    for i, x in enumerate(imgs):
        assert np.array_equal(got[i], pillow(x, 16, 16)), i


@pytest.mark.parametrize("backend", BACKENDS)
def test_more_samples_than_one_launch_carries(backend):
    """The geometry travels as a kernel argument, 64 samples a launch: 67 samples take two."""
    ctx = _ctx(backend)
    g = np.random.RandomState(67)
    imgs = [g.randint(0, 256, (3 + i % 4, 2 + i % 3, 3)).astype(np.uint8) for i in range(67)]
    got = engine.op_resize_u8(ctx, imgs, 5, 4).cpu().numpy()
    for i, x in enumerate(imgs):
        assert np.array_equal(got[i], pillow(x, 5, 4)), i


def test_a_one_pass_float_resize_is_not_pillow():
    """The tests above have teeth: a float64 one-pass antialiased bilinear, rounded and clamped, is NOT what Pillow computes -- the
    22-bit fixed point and the rounded intermediate image both show."""
    x = pair(75, 141)[0]
    t = torch.from_numpy(x).permute(2, 0, 1)[None].double()
    one_pass = F.interpolate(t, size=(37, 70), mode="bilinear", antialias=True, align_corners=False)
    one_pass = one_pass.round().clamp(0, 255)[0].permute(1, 2, 0).to(torch.uint8).numpy()
    assert int((one_pass != pillow(x, 37, 70)).sum()) >= 1


@pytest.mark.parametrize("w,h,size,want", [(300, 400, 128, (128, 170)), (400, 300, 128, (170, 128)), (256, 256, 128, (128, 128)),
                                           (128, 200, 128, (128, 200)), (38, 46, 19, (19, 23))])
def test_tv_resize_size(w, h, size, want):
    assert TB.tv_resize_size(w, h, size) == want
    assert TB.tv_resize_size(w, h, (7, 9)) == (9, 7)                # a (h, w) pair is taken as is


# ---- hand-over ---------------------------------------------------------------------------------------------------------------------
# (H0, W0) of the sources: the ORIGINALS of tests/test_texture_batch.py as images, with two heights adjusted so that torchvision's
# rule gives ONE resized size at load size 19 -- (25, 19) stays as it is under that rule (its smaller edge already is 19) and
# (40, 38) becomes 20 x 19, so they are (23, 19), which the resize copies, and (47, 38): int(19 * 47 / 38) = 23 like 46 and 69
SOURCE_SIZES = [(46, 38), (69, 57), (23, 19), (47, 38)]


@functools.lru_cache(maxsize=None)
def handover_samples():
    """(sources-form samples, the same with Pillow's resize done on the host) of the B = 4 case."""
    g = np.random.RandomState(19)
    sources, resized = [], []
    for b, (h0, w0) in enumerate(SOURCE_SIZES):
        assert TB.tv_resize_size(w0, h0, 19) == (19, 23)
        img = g.randint(0, 256, (h0, w0, 3)).astype(np.uint8)
        common = {"labels_u8": g.randint(0, 19, (11, 13)).astype(np.uint8), "rois_raw": ROI_ROWS, "paths": ("c%d" % b, "t%d" % b)}
        sources.append(dict(common, source_u8=img))
        resized.append(dict(common, image_u8=pillow(img, 23, 19), original_size=(w0, h0)))
    return sources, resized


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cropped", [1, 0])
def test_expansion_of_sources_equals_that_of_the_resized_images(backend, cropped):
    ctx = _ctx(backend)
    sources, resized = handover_samples()
    tb = TB.GpuTextureBatch(_opt(load_size=19, crop_size=None, crop_bounds="((3, 2), (19, 14))" if cropped else None), ctx=ctx)
    a, b = tb.collate(list(sources), flips=FLIPS), tb.collate(list(resized), flips=FLIPS)
    assert "textures_u8" not in a and a["resized"] == (23, 19) and a["crop"] == b["crop"] == ((3, 2, 16, 12) if cropped else (0, 0, 19, 23))
    assert a["sources_u8"].dim() == 1 and a["sources_u8"].numel() == 3 * sum(h * w for h, w in SOURCE_SIZES)
    assert a["source_geom"][:, 1:].tolist() == [list(s) for s in SOURCE_SIZES]
    assert torch.equal(a["sample_params"], b["sample_params"])       # roi_scale and the flip centres come from the sources' shapes
    ea, eb = tb.expand(a), tb.expand(b)
    for k in ("input_textures", "rois", "cloths", "target_textures"):
        assert torch.equal(ea[k].cpu(), eb[k].cpu()), k
    assert not torch.equal(ea["input_textures"].cpu(), ea["target_textures"].cpu())          # the flips are in it


# B = 2 at the smallest size the U-Net accepts: (load size, sources (H0, W0)); 72 -> resized 108 x 72 with the centred 64 x 64 crop,
# 64 -> resized 64 x 64 (one of them a copy), no crop
MODEL_CASES = [(72, ((150, 100), (225, 150))), (64, ((80, 80), (64, 64)))]


@functools.lru_cache(maxsize=None)
def model_batches(load_size):
    sizes = dict(MODEL_CASES)[load_size]
    g = np.random.RandomState(load_size)
    sources, resized = [], []
    for b, (h0, w0) in enumerate(sizes):
        ws, hs = TB.tv_resize_size(w0, h0, load_size)
        img = g.randint(0, 256, (h0, w0, 3)).astype(np.uint8)
        rois = np.sort(g.randint(0, w0, (12, 2, 2)), axis=1).reshape(12, 4).astype(np.float32)
        common = {"labels_u8": g.randint(0, 19, (10, 11)).repeat(4, 0).repeat(4, 1).astype(np.uint8), "rois_raw": rois, "paths": ("c%d" % b, "t%d" % b)}
        sources.append(dict(common, source_u8=img))
        resized.append(dict(common, image_u8=pillow(img, hs, ws), original_size=(w0, h0)))
    tb = TB.GpuTextureBatch(_opt(load_size=load_size))
    flips = [(1, 1), (0, 1)]
    return tb.collate(sources, flips=flips), tb.collate(resized, flips=flips)


def _run(m, state, batch):
    """Hand `batch` to the poisoned model in its own form: (taps after a forward pass, losses and D gradients after one step)."""
    backends.reset_state(m, state)
    _poison(m)
    if "sources_u8" in batch:
        m.set_input_texture_sources(batch)
    else:
        m.set_input_texture_batch(batch)
    m.forward(False, 0)
    taps = [m.tap(engine.NET_G, "unet_in").cpu(), m.tap(engine.NET_G, "pooled").cpu(), m.output().cpu()]
    m.step([0.9, 0.8, 1.0], training=True, seed=3)
    m.ctx.sync()
    return taps, m.losses(), m.grad_arena(engine.NET_D).cpu().clone()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("load_size", [c[0] for c in MODEL_CASES])
def test_model_handover_of_sources_equals_that_of_the_resized_images(backend, load_size):
    """unet_in holds the cloth slot, pooled is read from the texture and ROI slots, the discriminator's gradients from the target's."""
    ctx = _ctx(backend)
    from_sources, compact = model_batches(load_size)
    assert from_sources["crop"] == compact["crop"] == ((4, 4, 64, 64) if load_size == 72 else (0, 0, 64, 64))
    G, D, vgg, vgg_state_dict = texture_weights()
    m = backends.get_model(ctx, "texture", 2, 64)
    state = {engine.NET_G: G, engine.NET_D: D, engine.NET_VGG: vgg_state_dict(m, vgg)}
    (ta, la, ga), (tb, lb, gb) = _run(m, state, from_sources), _run(m, state, compact)
    for name, a, b in zip(("unet_in", "pooled", "fakes"), ta, tb):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert la == lb, (la, lb)
    assert torch.equal(ga, gb) and float(ga.abs().sum()) > 0
    # an inference model takes the same call
    mi = backends.get_model(ctx, "texture", 2, 64, is_train=False)
    mi.load_state_dict(engine.NET_G, G)
    outs = []
    for batch in (from_sources, compact):
        _poison(mi)
        (mi.set_input_texture_sources if "sources_u8" in batch else mi.set_input_texture_batch)(batch)
        mi.forward(False, 0)
        outs.append(mi.output().cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], ta[2])


@pytest.mark.small_channel_winograd
@pytest.mark.parametrize("backend", BACKENDS)
def test_create_model_trains_on_a_sources_batch_like_on_the_compact_one(backend, tmp_path):
    """TextureModel.set_input routes on the form; its lazily materialised tensors work from either."""
    import warnings
    from swapnet_amd.models import create_model
    from tests.test_models_api import make_opt
    from_sources, compact = model_batches(72)
    losses, models = [], []
    for batch in (from_sources, compact):
        opt = make_opt(tmp_path, backend, model="texture", texture_norm_stats=(MEAN, STD), load_size=72, input_transforms=("hflip", "vflip"))
        torch.manual_seed(11)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)         # (seeded-random VGG16 where no pretrained weights are at hand)
            model = create_model(opt)
        model.eval()
        model.set_input(batch)
        torch.manual_seed(5)
        model.optimize_parameters()
        losses.append(model.get_current_losses())
        models.append(model)
    assert losses[0] == losses[1] and all(np.isfinite(v) for v in losses[0].values()), losses
    a, b = models
    assert torch.equal(a.fakes.cpu(), b.fakes.cpu())
    assert a._compact is from_sources and a._textures is None         # nothing was expanded on the training path
    assert a.get_image_paths() == (("c0", "t0"), ("c1", "t1"))
    for name in ("textures", "cloths", "targets"):
        assert torch.equal(getattr(a, name).cpu(), getattr(b, name).cpu()), name


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    ctx = _ctx(backend)
    imgs = [pair(23, 19)[0], pair(40, 31)[0]]
    packed, geom = engine.pack_u8_images(imgs)

    def still_right():
        got = engine.op_resize_u8(ctx, imgs, 16, 16).cpu().numpy()
        assert all(np.array_equal(got[i], pillow(x, 16, 16)) for i, x in enumerate(imgs))

    with pytest.raises(ValueError, match="sample 1 runs past src_bytes"):
        engine.op_resize_u8_packed(ctx, packed[:-1], geom, 16, 16)
    still_right()
    with pytest.raises(ValueError, match="sample 1 runs past src_bytes"):
        engine.op_resize_u8_packed(ctx, packed, [[0, 23, 19], [-3, 1, 1]], 16, 16)
    with pytest.raises(ValueError, match="sample 1 has an empty or oversized source"):
        engine.op_resize_u8(ctx, [imgs[0], np.zeros((0, 7, 3), dtype=np.uint8)], 16, 16)
    with pytest.raises(ValueError, match="reduction bound.*more than 31 to 1"):
        engine.op_resize_u8(ctx, [pair(8, 600)[0]], 8, 19)                 # 600 > 31 * 19
    with pytest.raises(ValueError, match=r"\(H0, W0, 3\) uint8"):
        engine.op_resize_u8(ctx, [imgs[0][:, :, :2]], 16, 16)
    still_right()
    # the batch forms
    sources, resized = handover_samples()
    tb = TB.GpuTextureBatch(_opt(load_size=19, crop_size=None, crop_bounds="((3, 2), (19, 14))"), ctx=ctx)
    with pytest.raises(ValueError, match="not a mix"):
        tb.collate([sources[0], resized[1]])
    with pytest.raises(ValueError, match="not a mix"):
        tb.collate([dict(sources[0], image_u8=resized[0]["image_u8"])])
    with pytest.raises(ValueError, match="resized sizes"):
        tb.collate([sources[0], dict(sources[1], source_u8=pair(40, 38)[0])])          # (19, 23) and (19, 20)
    with pytest.raises(ValueError, match="label maps"):
        tb.collate([sources[0], dict(sources[1], labels_u8=sources[1]["labels_u8"][:-1])])
    good = tb.collate(list(sources), flips=FLIPS)
    with pytest.raises(ValueError, match="crop window"):
        TB.expand_batch(ctx, dict(good, crop=(4, 2, 16, 12)))                          # 4 + 16 > 19
    want = tb.expand(tb.collate(list(resized), flips=FLIPS))
    assert torch.equal(tb.expand(good)["input_textures"].cpu(), want["input_textures"].cpu())
    # the model: a refused hand-over writes nothing -- the slots still hold what the valid call before it left, and the next valid
    # call is right
    from_sources, compact = model_batches(72)
    warp = backends.get_model(ctx, "warp", 2, 64, is_train=False)
    with pytest.raises(ValueError, match="only the texture model"):
        warp.set_input_texture_sources(from_sources)
    m = backends.get_model(ctx, "texture", 2, 64, is_train=False)
    m.load_state_dict(engine.NET_G, texture_weights()[0])

    def out(batch):
        (m.set_input_texture_sources if "sources_u8" in batch else m.set_input_texture_batch)(batch)
        m.forward(False, 0)
        return m.output().cpu()

    ref = out(compact)
    bad_geom = from_sources["source_geom"].clone()
    bad_geom[1, 1] += 1                                                                 # one row more than the buffer holds
    for bad, msg in ((dict(from_sources, crop=(9, 4, 64, 64)), "crop window"),          # 9 + 64 > 72
                     (dict(from_sources, source_geom=bad_geom), "runs past src_bytes"),
                     (dict(from_sources, rois_raw=from_sources["rois_raw"][:, :5]), "num_roi"),
                     ({k: (v[:1] if k in ("source_geom", "cloth_labels_u8", "rois_raw", "sample_params") else v) for k, v in from_sources.items()}, "batch")):
        _poison(m)
        m.forward(False, 0)
        before = m.output().cpu()
        with pytest.raises(ValueError, match=msg):
            m.set_input_texture_sources(bad)
        m.forward(False, 0)
        assert torch.equal(m.output().cpu(), before), msg
    assert torch.equal(out(from_sources), ref)
