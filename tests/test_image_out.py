"""Saved-image visuals on the device (ops.h image_u8, swn_op_image_u8): bytes against the reference's host chain -- unnormalize /
scale_tensor (swapnet_amd.util, which restate datasets/data_utils.py:41-90), decode_cloth_labels, Pillow's ImageDraw.rectangle and
util.tensor2im's numpy formula -- for EQUALITY: every step is one rounded fp32 operation or integer work.  The same cases run on
the CI host simulator (engine.cpp's plain loops) and, marked gpu, through the HIP kernels of image_out.hip."""
import inspect

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from swapnet_amd import engine
from swapnet_amd.util import util as U
from swapnet_amd.util.decode_labels import decode_cloth_labels
from tests import backends

BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]
# (B, H, W): the issue's 19 x 23; 45 x 67 = 3015 pixels (no multiple of 4 or of a 1024-pixel block, three min/max chunks, images
# after the first at byte offsets that are no multiple of 4); one pixel; a width-3 image (every four-pixel group crosses a row)
SHAPES = [(4, 19, 23), (2, 45, 67), (3, 1, 1), (2, 5, 3)]
MEAN, STD = (0.45, 0.4, 0.5), (0.25, 0.3, 0.2)


def _ctx(backend):
    return backends.gpu_ctx() if backend == "gpu" else backends.hostsim_ctx()


def _img(ctx, *a, **kw):
    return engine.op_image_u8(ctx, *a, **kw).cpu().numpy()


def _hwc(t):
    return np.ascontiguousarray(t.numpy().transpose(0, 2, 3, 1))


def signed_bytes(t):
    """util.tensor2im's formula (util/util.py:27,32) on a whole batch; defined for values in [-1, 1]."""
    return ((_hwc(t) + 1) / 2.0 * 255.0).astype(np.uint8)


def unit_bytes(t):
    return (_hwc(t) * 255.0).astype(np.uint8)


def _tanh(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tanh(1.5 * torch.randn(shape, generator=g))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_float_images_equal_the_reference_chain(backend, shape):
    ctx = _ctx(backend)
    B, H, W = shape
    x = _tanh((B, 3, H, W), 1)
    assert x.dtype == torch.float32 and signed_bytes(x).dtype == np.uint8
    assert np.array_equal(_img(ctx, x), signed_bytes(x))
    x01 = (x + 1) / 2
    assert np.array_equal(_img(ctx, x01, range=engine.RANGE_UNIT), unit_bytes(x01))
    # grayscale: replicated to three channels (util/util.py:24-25)
    g = x[:, :1]
    assert np.array_equal(_img(ctx, g), signed_bytes(g.expand(-1, 3, -1, -1)))
    # unnormalize with its zip over dim 0: images 0..2 get (std[b], mean[b]) and the clamp, image 3 stays as it is (inside [-1, 1])
    rows = engine.image_rows(B, 3, MEAN, STD)
    un = U.unnormalize(x, MEAN, STD)
    if B > 3:
        assert torch.equal(un[3], x[3]) and float(un[3].min()) < 0 and float(un[:3].min()) >= 0
    assert np.array_equal(_img(ctx, x, rows=rows), signed_bytes(un))
    assert np.array_equal(_img(ctx, x, rows=rows, range=engine.RANGE_UNIT)[:3], unit_bytes(un)[:3])
    # reference_quirk = False: the per-channel form on every image
    per = x.clone()
    for c in range(3):
        per[:, c].mul_(STD[c]).add_(MEAN[c]).clamp_(0, 1)
    got = _img(ctx, x, rows=engine.image_rows(B, 3, MEAN, STD, reference_quirk=False))
    assert np.array_equal(got, signed_bytes(per))
    # outside [-1, 1] numpy's cast is undefined: the stated behaviour is saturation, then truncation
    wide = 3 * x
    f = (_hwc(wide) + 1) / 2.0 * 255.0
    assert f.dtype == np.float32 and f.min() < -100 and f.max() > 400
    assert np.array_equal(_img(ctx, wide), np.clip(f, 0, 255).astype(np.uint8))
    f = _hwc(wide) * 255.0
    assert np.array_equal(_img(ctx, wide, range=engine.RANGE_UNIT), np.clip(f, 0, 255).astype(np.uint8))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_scale_each_equals_scale_tensor(backend, shape):
    ctx = _ctx(backend)
    B, H, W = shape
    g = torch.Generator().manual_seed(2)
    cases = {"tanh": _tanh((B, 3, H, W), 3),
             # all positive: a zero pad channel taking part would become the minimum
             "positive": 0.5 + torch.rand((B, 3, H, W), generator=g),
             "constant": torch.full((B, 3, H, W), 0.3125),           # den = 1e-5
             "wide": 40 * torch.randn((B, 3, H, W), generator=g)}
    ends = _tanh((B, 3, H, W), 4)                                     # the maximum is the first element, the minimum the very last
    ends.view(B, -1)[:, 0] = 2.5
    ends.view(B, -1)[:, -1] = -1.75
    cases["ends"] = ends
    for name, x in cases.items():
        ref = U.scale_tensor(x, scale_each=True)
        assert float(ref.min()) >= 0 and float(ref.max()) <= 1, name
        assert np.array_equal(_img(ctx, x, scale_each=True), signed_bytes(ref)), name
        assert np.array_equal(_img(ctx, x, scale_each=True, range=engine.RANGE_UNIT), unit_bytes(ref)), name
    # each image by its own range
    x = cases["tanh"] * torch.arange(1, B + 1).view(B, 1, 1, 1)
    assert np.array_equal(_img(ctx, x, scale_each=True), signed_bytes(U.scale_tensor(x, scale_each=True)))
    with pytest.raises(ValueError, match="exclude each other"):
        _img(ctx, x, scale_each=True, rows=engine.image_rows(B, 3, MEAN, STD))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_palette_sources_equal_decode_cloth_labels(backend, shape):
    ctx = _ctx(backend)
    B, H, W = shape
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(0, 19, (B, H, W), generator=g)
    onehot = torch.nn.functional.one_hot(labels, 19).permute(0, 3, 1, 2).float()
    ref = _hwc(decode_cloth_labels(onehot, ctx=ctx))
    assert np.array_equal(_img(ctx, onehot, source=engine.SRC_ARGMAX), ref)
    assert np.array_equal(_img(ctx, labels=labels), ref)
    # tied logits (small integers, C = 19): the first maximum wins, as argmax does
    tied = torch.randint(0, 3, (B, 19, H, W), generator=g).float()
    got = _img(ctx, tied, source=engine.SRC_ARGMAX)
    assert np.array_equal(got, _hwc(decode_cloth_labels(tied, ctx=ctx)))
    assert np.array_equal(got, _img(ctx, labels=tied.argmax(dim=1)))
    two = torch.zeros((B, 19, H, W))
    two[:, 3] = two[:, 7] = 1.0
    assert (_img(ctx, two, source=engine.SRC_ARGMAX) == np.array([0, 85, 0], dtype=np.uint8)).all()       # colour 3, not 7
    # label 19 and above (and a negative one) give black
    odd = torch.tensor([19, 25, 255, -1, 2 ** 31 - 1])[torch.randint(0, 5, (B, H, W), generator=g)]
    assert not _img(ctx, labels=odd).any()
    many = torch.zeros((B, 24, H, W))
    many[:, 20] = 1.0
    assert not _img(ctx, many, source=engine.SRC_ARGMAX).any()
    many[:, 20] = 0.0
    many[:, 18] = 1.0
    assert (_img(ctx, many, source=engine.SRC_ARGMAX) == np.array([255, 170, 0], dtype=np.uint8)).all()


def pillow_outlines(base, rois, colours, width):
    """The loop of util/draw_rois.py:33-44 on ready bytes."""
    out = []
    for im, boxes in zip(base, rois):
        im = Image.fromarray(im)
        draw = ImageDraw.Draw(im)
        for i, box in enumerate(boxes):
            draw.rectangle(box.numpy(), outline=tuple(int(c) for c in colours[i]), width=width)
        out.append(np.array(im))
    return np.stack(out)


_BOXES = {}


def exhaustive_boxes():
    """Every integer box with -3 <= x0 <= x1 <= 11 and -3 <= y0 <= y1 <= 9 for a 9 x 7 image (10 920 of them), one per image, with
    Pillow's outlines of width 1, 2 and 3 on a random base image -- built once."""
    if not _BOXES:
        rows = [(x0, y0, x1, y1) for x0 in range(-3, 12) for x1 in range(x0, 12) for y0 in range(-3, 10) for y1 in range(y0, 10)]
        rois = torch.tensor(rows, dtype=torch.float32).view(-1, 1, 4)
        assert rois.shape[0] == 10920
        base = _tanh((1, 3, 7, 9), 6).expand(rois.shape[0], -1, -1, -1).contiguous()
        colours = np.array([[255, 1, 128]], dtype=np.uint8)
        bytes_ = signed_bytes(base)
        _BOXES.update(rois=rois, base=base, colours=colours, ref={w: pillow_outlines(bytes_, rois, colours, w) for w in (1, 2, 3)})
    return _BOXES


@pytest.mark.parametrize("backend", BACKENDS)
def test_roi_outlines_equal_pillow_on_every_box(backend):
    ctx = _ctx(backend)
    e = exhaustive_boxes()
    for width, ref in e["ref"].items():
        got = _img(ctx, e["base"], rois=e["rois"], colours=e["colours"], width=width)          # ONE launch, B = number of boxes
        bad = np.nonzero((got != ref).reshape(len(ref), -1).any(axis=1))[0]
        assert bad.size == 0, (width, bad.size, e["rois"][bad[0]].tolist())


@pytest.mark.parametrize("backend", BACKENDS)
def test_roi_outlines_fractional_overlapping_and_degenerate_boxes(backend):
    ctx = _ctx(backend)
    colours = (np.arange(36, dtype=np.uint8).reshape(12, 3) * 7 + 3)
    # fractional coordinates truncate toward zero, positive and negative
    frac = torch.tensor([[2.6, 1.4, 9.5, 8.9], [-0.7, -0.2, 3.9, 4.1], [-2.5, -1.5, 2.5, 3.5], [0.99, 0.99, 10.01, 8.5], [-3.9, 2.2, 20.7, 2.9],
                         [4.5, -7.5, 4.6, 30.25]]).view(-1, 1, 4)
    base = _tanh((frac.shape[0], 3, 10, 12), 7)
    for width in (1, 2, 3):
        got = _img(ctx, base, rois=frac, colours=colours[:1], width=width)
        assert np.array_equal(got, pillow_outlines(signed_bytes(base), frac, colours, width)), width
    one = _img(ctx, base[:1], rois=frac[:1], colours=colours[:1], width=2)[0]
    hit = (one == colours[0]).all(axis=2)
    assert hit[1:3, 2:10].all() and hit[7:9, 2:10].all() and hit[1:9, 2:4].all() and hit[1:9, 8:10].all() and hit.sum() == 48
    # 12 overlapping boxes on one 64 x 48 image: the last outline that covers a pixel wins
    g = torch.Generator().manual_seed(8)
    lo = torch.randint(-4, 40, (2, 12, 2), generator=g).float()
    boxes = torch.cat([lo, lo + torch.randint(0, 30, (2, 12, 2), generator=g).float()], dim=2)
    boxes[1, :, :] = boxes[0].flip(0)                                 # the same boxes in the opposite order: other winners
    img = _tanh((2, 3, 48, 64), 9)
    for width in (1, 3):
        got = _img(ctx, img, rois=boxes, colours=colours, width=width)
        assert np.array_equal(got, pillow_outlines(signed_bytes(img), boxes, colours, width)), width
    assert not np.array_equal(got[0], got[1])
    # the all-zero row (what the reference's rois.csv turns None into): (x 0, y 0) and (x 0, y 1)
    zero = torch.zeros((1, 12, 4))
    got = _img(ctx, img[:1], rois=zero, colours=colours, width=1)
    assert np.array_equal(got, pillow_outlines(signed_bytes(img[:1]), zero, colours, 1))
    changed = (got != signed_bytes(img[:1])).any(axis=3)[0]
    assert changed[0, 0] and changed[1, 0] and changed.sum() == 2 and (got[0, 1, 0] == colours[11]).all()
    # outlines over a palette source as well
    labels = torch.randint(0, 19, (2, 48, 64), generator=g)
    got = _img(ctx, labels=labels, rois=boxes, colours=colours, width=2)
    assert np.array_equal(got, pillow_outlines(_img(ctx, labels=labels), boxes, colours, 2))


def test_reversed_boxes_raise_before_the_library_is_called(monkeypatch):
    ctx = backends.hostsim_ctx()
    calls = []
    real = ctx.lib.call
    monkeypatch.setattr(ctx.lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    img = torch.zeros((1, 3, 7, 9))
    col = np.zeros((1, 3), dtype=np.uint8)
    for box, what in (([5, 1, 4, 3], "x1 must be greater than or equal to x0"), ([1, 5, 4, 3], "y1 must be greater than or equal to y0")):
        with pytest.raises(ValueError, match=what):                    # Pillow's own words
            ImageDraw.Draw(Image.new("RGB", (9, 7))).rectangle(box, outline=(1, 2, 3), width=1)
        with pytest.raises(ValueError, match=what):
            engine.op_image_u8(ctx, img, rois=torch.tensor([[box]], dtype=torch.float32), colours=col, width=1)
    assert "swn_op_image_u8" not in calls
    engine.op_image_u8(ctx, img, rois=torch.tensor([[[1., 1., 4., 3.]]]), colours=col, width=1)
    assert "swn_op_image_u8" in calls
    for bad in (dict(rois=torch.zeros((1, 17, 4)), colours=np.zeros((17, 3), np.uint8)), dict(rois=torch.zeros((1, 1, 4)), colours=col, width=0)):
        with pytest.raises(ValueError):
            engine.op_image_u8(ctx, img, **bad)
    with pytest.raises(ValueError, match="3 channels"):
        engine.op_image_u8(ctx, torch.zeros((1, 2, 7, 9)))


@pytest.mark.parametrize("backend", BACKENDS)
def test_tensor2im_and_draw_rois_on_texture_keep_the_reference_interface(backend):
    from swapnet_amd.util.draw_rois import BODY_COLORS, NUM_BODY_LABELS, draw_rois_on_texture
    ctx = _ctx(backend)
    sig = inspect.signature(U.tensor2im)
    assert list(sig.parameters)[:2] == ["input_image", "imtype"] and sig.parameters["imtype"].default is np.uint8
    assert all(p.kind is p.KEYWORD_ONLY for p in list(sig.parameters.values())[2:])
    x = _tanh((3, 3, 19, 23), 10)
    im = U.tensor2im(x, ctx=ctx)                                       # the first of the batch
    assert im.shape == (19, 23, 3) and im.dtype == np.uint8 and np.array_equal(im, signed_bytes(x)[0])
    assert np.array_equal(U.tensor2im(x[:, :1], ctx=ctx), signed_bytes(x[:, :1].expand(-1, 3, -1, -1))[0])
    assert U.tensor2im(x, np.int32, ctx=ctx).dtype == np.int32
    arr = np.arange(2 * 5 * 4 * 3, dtype=np.uint8).reshape(2, 5, 4, 3)
    assert np.array_equal(U.tensor2im(arr), arr[0]) and np.array_equal(U.tensor2im(arr[1]), arr[1])      # numpy passes through
    assert U.tensor2im("not an image") == "not an image"
    u8 = torch.arange(2 * 3 * 5 * 4, dtype=torch.uint8).view(2, 3, 5, 4)
    assert np.array_equal(U.tensor2im(u8), u8[0].permute(1, 2, 0).numpy())
    # draw_rois_on_texture against the reference's loop (util/draw_rois.py:33-44)
    sig = inspect.signature(draw_rois_on_texture)
    assert list(sig.parameters)[:3] == ["rois", "texture_tensors", "width_factor"] and sig.parameters["width_factor"].default == 0.01
    assert BODY_COLORS.shape == (NUM_BODY_LABELS, 3) == (12, 3) and BODY_COLORS.dtype == np.uint8
    assert BODY_COLORS[0].tolist() == [219, 94, 86] and len({tuple(c) for c in BODY_COLORS.tolist()}) == 12
    g = torch.Generator().manual_seed(11)
    tex = _tanh((2, 3, 64, 128), 12).add(1).div(2)                    # an "unnormalized" texture in [0, 1]
    lo = torch.randint(0, 60, (2, 12, 2), generator=g).float()
    rois = torch.cat([lo, lo + torch.randint(0, 70, (2, 12, 2), generator=g).float()], dim=2)
    rois[0, 5] = 0
    for factor, width in ((0.01, 1), (0.02, 3)):
        assert int(round(factor * 128)) == width
        got = draw_rois_on_texture(rois, tex, factor, ctx=ctx) if factor != 0.01 else draw_rois_on_texture(rois, tex, ctx=ctx)
        assert got.shape == (2, 64, 128, 3) and got.dtype == np.uint8
        assert np.array_equal(got, pillow_outlines(signed_bytes(tex), rois, BODY_COLORS, width))
    # a width that rounds to 0 draws nothing, as ImageDraw.rectangle(width=0) does
    assert np.array_equal(draw_rois_on_texture(rois[:, :, :], tex[:, :, :, :32], ctx=ctx), signed_bytes(tex[:, :, :, :32]))
