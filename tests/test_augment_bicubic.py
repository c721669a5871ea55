"""RandomPerspective resampled BICUBIC (kind 3 of the map table; swn_op_chain_resample, swn_op_warp_batch_ex,
swn_model_set_input_warp_batch_ex).  Oracle = Pillow itself, as in tests/test_augment.py: every channel goes through the SAME
sequence of PIL operations with the SAME parameters, the perspective with Image.BICUBIC on the mode-"F" image that
per_channel_transform hands it, and must come out bit-identical -- floats are compared as uint32 patterns, nothing left out."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

from swapnet_amd import _C, engine
from swapnet_amd.datasets import gpu_augment as A
from swapnet_amd.datasets import gpu_warp_batch as WB
from tests import backends

BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]
K3 = A.KIND_PERSPECTIVE_BICUBIC


def _ctx(kind):
    return backends.gpu_ctx() if kind == "gpu" else backends.hostsim_ctx()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def pil_chain(channel, chain_desc):
    """channel: (H, W) float32; chain_desc: ("hflip",) / ("vflip",) / ("affine", coeffs6) / ("persp", coeffs8) / ("bicubic", coeffs8)."""
    img = Image.fromarray(np.ascontiguousarray(channel, dtype=np.float32))
    assert img.mode == "F"
    for step in chain_desc:
        if step[0] == "hflip":
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        elif step[0] == "vflip":
            img = img.transpose(Image.FLIP_TOP_BOTTOM)
        elif step[0] == "affine":
            img = img.transform(img.size, Image.AFFINE, step[1], Image.NEAREST)
        elif step[0] == "persp":
            img = img.transform(img.size, Image.PERSPECTIVE, step[1], Image.NEAREST)
        elif step[0] == "bicubic":
            img = img.transform(img.size, Image.PERSPECTIVE, step[1], Image.BICUBIC)      # torchvision 0.4.0 F.perspective
    return np.array(img)


def _other(rng, W, H):
    """One non-bicubic row and its PIL description: a flip or an affine (never the identity, so every position of the chain acts)."""
    k = rng.choice(["hflip", "vflip", "affine"])
    if k == "hflip":
        return A.hflip_map(W, H), ("hflip",)
    if k == "vflip":
        return A.vflip_map(W, H), ("vflip",)
    ang, tr, sc, sh = A.random_affine_params(W, H, rng=rng)
    m = A.inverse_affine_matrix((W * 0.5 + 0.5, H * 0.5 + 0.5), ang, tr, sc, sh)
    return A.affine_map(m), ("affine", m)


def _persp(rng, W, H):
    sp, ep = A.random_perspective_points(W, H, rng=rng)
    return A.perspective_coeffs(sp, ep)


def _fill_coeffs(W, H):
    """A perspective whose quad is the image shifted by a third of its size and shrunk: a band of the output maps outside the source."""
    sp = [(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)]
    ep = [(W // 3, H // 3), (W - 1, H // 4), (W - 1 - W // 5, H - 1), (W // 4, H - 1 - H // 5)]
    return A.perspective_coeffs(sp, ep)


def _chains(rng, B, C, W, H):
    """(B, C, 4, 9) table and the PIL descriptions: the kind-3 row at position (b * C + c) % 4 with flips and affines around it; every
    fifth chain is the bicubic alone (identities around it), every seventh pushes part of the output into the fill."""
    maps = np.zeros((B, C, 4, 9))
    desc = {}
    for b in range(B):
        for c in range(C):
            n = b * C + c
            pos = n % 4
            co = _fill_coeffs(W, H) if n % 7 == 3 else _persp(rng, W, H)
            chain, d = [], []
            for k in range(4):
                if k == pos:
                    chain.append([K3] + co); d.append(("bicubic", co))
                elif n % 5 == 4:
                    chain.append(A.IDENTITY)
                else:
                    row, step = _other(rng, W, H)
                    chain.append(row); d.append(step)
            maps[b, c] = np.array(chain)
            desc[(b, c)] = d
    return maps, desc


def _binary_batch(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C, (B, (H + 3) // 4, (W + 3) // 4), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W]
    return torch.nn.functional.one_hot(lab, C).movedim(-1, 1).float().contiguous()


def _call_op(ctx, name, batch, maps):
    B, C, H, W = batch.shape
    src = batch.to(device=ctx.device, dtype=torch.float32).contiguous()
    dst = torch.empty_like(src)
    md = torch.from_numpy(np.ascontiguousarray(maps, dtype=np.float64).reshape(B * C, -1, 9)).to(ctx.device)
    ctx.lib.call(name, ctx.handle, _C.ptr(src), _C.ptr(dst), B, C, H, W, _C.ptr(md), md.shape[1])
    ctx.sync()
    return dst.cpu().numpy()


@pytest.mark.parametrize("backend", BACKENDS)
def test_chain_resample_is_bit_identical_to_pillow(backend):
    ctx = _ctx(backend)
    rng = random.Random(11)
    main = (4, 19, 64, 48) if backend == "gpu" else (2, 5, 24, 20)
    # (B, C, H, W): the main size; 3x2 and 7x5, where every tap clips on every side; W = 33, not a multiple of 4
    shapes = [main, (1, 4, 3, 2), (1, 4, 7, 5), (1, 4, 17, 33)]
    nonbinary = total = 0
    for si, (B, C, H, W) in enumerate(shapes):
        batch = _binary_batch(B, C, H, W, seed=si)
        maps, desc = _chains(rng, B, C, W, H)
        out = A.apply_maps(ctx, batch, maps).cpu().numpy()
        for (b, c), d in desc.items():
            ref = pil_chain(batch[b, c].numpy(), d)
            assert np.array_equal(bits(out[b, c]), bits(ref)), ((B, C, H, W), b, c, d, int((bits(out[b, c]) != bits(ref)).sum()))
        nonbinary += int(((out != 0) & (out != 1)).sum())
        total += out.size
    print("non-binary outputs of the binary-source cases: %d of %d (%.1f %%)" % (nonbinary, total, 100.0 * nonbinary / total))
    assert nonbinary > 0.05 * total                     # the inputs do exercise interpolation (Pillow alone: 29 % on such maps)


@pytest.mark.parametrize("backend", BACKENDS)
def test_chain_resample_reads_float_sources_and_fills(backend):
    """A source that is random float32, not 0/1 (a kernel that assumes binary taps fails; so does one that forms the row cubic's
    coefficients in double: Pillow forms them in fp32), the bicubic alone, and a quad that pushes output into the fill."""
    ctx = _ctx(backend)
    rng = random.Random(12)
    B, C, H, W = 2, 4, 24, 20
    batch = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(5))
    maps, desc = _chains(rng, B, C, W, H)
    alone = _fill_coeffs(W, H)
    maps[0, 0] = np.array([[K3] + alone, A.IDENTITY, A.IDENTITY, A.IDENTITY]); desc[(0, 0)] = [("bicubic", alone)]
    out = A.apply_maps(ctx, batch, maps).cpu().numpy()
    for (b, c), d in desc.items():
        ref = pil_chain(batch[b, c].numpy(), d)
        assert np.array_equal(bits(out[b, c]), bits(ref)), (b, c, d, int((bits(out[b, c]) != bits(ref)).sum()))
    ref = pil_chain(batch[0, 0].numpy(), desc[(0, 0)])
    assert (ref == 0).sum() > 0.1 * ref.size and (ref != 0).sum() > 0.1 * ref.size      # part fill, part image
    # a single-row table that is the bicubic and nothing else
    one = np.array([[[[K3] + _persp(rng, W, H)] for _ in range(C)] for _ in range(B)])
    out = A.apply_maps(ctx, batch, one).cpu().numpy()
    for b in range(B):
        for c in range(C):
            ref = pil_chain(batch[b, c].numpy(), [("bicubic", one[b, c, 0, 1:].tolist())])
            assert np.array_equal(bits(out[b, c]), bits(ref)), (b, c)


@pytest.mark.parametrize("backend", BACKENDS)
def test_chain_resample_without_kind_3_is_affine_gather(backend):
    ctx = _ctx(backend)
    B, C, H, W = 2, 5, 24, 20
    batch = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(6))
    t = A.GpuPerChannelTransform(rng=random.Random(4))
    maps = t.draw_maps(B, C, W, H)
    assert (maps[..., 0] == A.KIND_PERSPECTIVE).any() and not (maps[..., 0] == K3).any()
    want = _call_op(ctx, "swn_op_affine_gather", batch, maps)
    got = _call_op(ctx, "swn_op_chain_resample", batch, maps)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(A.apply_maps(ctx, batch, maps).cpu().numpy()), bits(want))


# ---- the warp batch hand-over ----------------------------------------------------------------------------------------------------
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _warp_case(C, seed):
    """B = 2, labels 23 x 19, body 31 x 27, Ls = 40, crop 32 x 24 at (3, 5), input labels other than the target's (video mode)."""
    g = torch.Generator().manual_seed(seed)
    B, Hl, Wl = 2, 23, 19
    block = lambda: torch.randint(0, C, (B, 6, 5), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :Hl, :Wl].to(torch.uint8).contiguous()
    return dict(body=torch.randint(0, 256, (B, 31, 27, 3), generator=g, dtype=torch.uint8), inp=block(), tgt=block(), B=B, Hl=Hl, Wl=Wl,
                Ls=40, x_min=3, y_min=5, H=24, W=32)


def _warp_call(ctx, c, maps, C, bicubic):
    out = engine.op_warp_batch(ctx, c["body"], c["inp"], c["tgt"], maps, MEAN, STD, c["Ls"], c["x_min"], c["y_min"], c["H"], c["W"], C,
                               bicubic=bicubic)
    ctx.sync()
    return [t.cpu() for t in out]


@pytest.mark.parametrize("channels", [19, 5])
@pytest.mark.parametrize("backend", BACKENDS)
def test_warp_batch_bicubic_is_the_pillow_chain(backend, channels):
    ctx = _ctx(backend)
    C = channels
    c = _warp_case(C, seed=20 + C)
    maps, desc = _chains(random.Random(30 + C), c["B"], C, c["Wl"], c["Hl"])
    bodys, inputs, targets = _warp_call(ctx, c, maps, C, True)
    # one-hot (label 0: all zero) -> the PIL chain per channel at label resolution -> F.interpolate nearest -> crop
    onehot = torch.nn.functional.one_hot(c["inp"].long(), C).movedim(-1, 1).float()
    onehot[:, 0] = 0
    aug = torch.empty_like(onehot)
    for (b, ch), d in desc.items():
        aug[b, ch] = torch.from_numpy(pil_chain(onehot[b, ch].numpy(), d))
    want = torch.nn.functional.interpolate(aug, size=(c["Ls"], c["Ls"]), mode="nearest")
    want = want[:, :, c["y_min"]:c["y_min"] + c["H"], c["x_min"]:c["x_min"] + c["W"]]
    assert np.array_equal(bits(inputs.numpy()), bits(want.numpy())), int((bits(inputs.numpy()) != bits(want.numpy())).sum())
    assert ((want != 0) & (want != 1)).float().mean() > 0.05
    # the body and target outputs do not depend on the flag: the flag-off call's bytes (on a table the old entry point takes)
    nearest = maps.copy()
    nearest[..., 0][nearest[..., 0] == K3] = A.KIND_PERSPECTIVE
    off = _warp_call(ctx, c, nearest, C, False)
    assert np.array_equal(bits(bodys.numpy()), bits(off[0].numpy())) and np.array_equal(bits(targets.numpy()), bits(off[2].numpy()))
    # the flag set and no kind 3 in the table: everything equals the flag-off call
    on = _warp_call(ctx, c, nearest, C, True)
    for got, ref in zip(on, off):
        assert np.array_equal(bits(got.numpy()), bits(ref.numpy()))
    # ... and so without a table at all
    for got, ref in zip(_warp_call(ctx, c, None, C, True), _warp_call(ctx, c, None, C, False)):
        assert np.array_equal(bits(got.numpy()), bits(ref.numpy()))


# ---- the model path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_warp_model_takes_a_bicubic_batch(backend, tmp_path, monkeypatch):
    """64 x 64, batch 2: the compact bicubic batch and its expansion give the same fakes bit for bit, and a training step on the compact
    batch runs clean under the slot audit although the cloth operand now exceeds 1 (its amax slot is measured after the launch)."""
    from swapnet_amd.models import create_model
    from tests.test_models_api import make_opt
    if backend == "sim":
        monkeypatch.setenv("SWN_SIM_PAIR", "1")           # (the simulator always checks its slots; as tests/test_produced_operands.py)
    opt = make_opt(tmp_path, backend, body_norm_stats=(MEAN, STD), load_size=72, perspective_resample="bicubic",
                   input_transforms=("hflip", "vflip", "affine", "perspective"))
    torch.manual_seed(11)
    model = create_model(opt)
    model.eval()
    ctx = model.backend.ctx
    wb = WB.GpuWarpBatch(opt, ctx=ctx, rng=random.Random(3))
    g = np.random.RandomState(8)
    block = lambda: np.repeat(np.repeat(g.randint(0, 19, (10, 8)), 4, 0), 4, 1).astype(np.uint8)            # 40 x 32 label maps
    samples = [{"body_u8": g.randint(0, 256, (50, 44, 3)).astype(np.uint8), "target_labels_u8": block(), "input_labels_u8": block(),
                "paths": ("c%d" % i, "b%d" % i)} for i in range(2)]
    batch = wb.collate(samples)
    assert batch["perspective_resample"] == "bicubic" and (batch["maps"][..., 0] == K3).any()
    ref = wb.expand(batch)
    assert float(ref["input_cloths"].max()) > 1.0 and float(ref["input_cloths"].min()) < 0.0, "no overshoot in the input: a weak case"
    model.set_input(batch)
    model.test()
    compact = model.fakes.cpu().clone()
    assert torch.equal(model.inputs.cpu(), ref["input_cloths"].cpu())
    model.set_input(ref)
    model.test()
    assert np.array_equal(bits(model.fakes.cpu().numpy()), bits(compact.numpy())) and bool(torch.isfinite(compact).all())
    ctx.lib.call("swn_slot_audit", 1)
    try:
        model.set_input(batch)
        model.optimize_parameters()
        ctx.sync()
    finally:
        ctx.lib.call("swn_slot_audit", 0)
    assert all(np.isfinite(v) for v in model.get_current_losses().values())


# ---- parameter draws, the batch, the refusals (no device) ----------------------------------------------------------------------
class _Opt:
    input_transforms = ("hflip", "vflip", "affine", "perspective")
    load_size, crop_size, crop_bounds, cloth_channels, is_train = 40, 32, None, 5, True
    body_norm_stats = (MEAN, STD)


def _samples(n=2):
    g = np.random.RandomState(3)
    return [{"body_u8": g.randint(0, 256, (31, 27, 3)).astype(np.uint8), "target_labels_u8": g.randint(0, 5, (23, 19)).astype(np.uint8),
             "paths": ("c%d" % i, "b%d" % i)} for i in range(n)]


def test_bicubic_draws_are_the_nearest_draws_with_another_kind():
    near = A.GpuPerChannelTransform(rng=random.Random(9)).draw_maps(3, 19, 48, 64)
    cub = A.GpuPerChannelTransform(rng=random.Random(9), perspective_resample="bicubic").draw_maps(3, 19, 48, 64)
    assert A.KIND_PERSPECTIVE_BICUBIC == 3 and np.array_equal(near[..., 1:], cub[..., 1:])
    p = near[..., 0] == A.KIND_PERSPECTIVE
    assert p.any() and np.array_equal(near[..., 0][~p], cub[..., 0][~p]) and (cub[..., 0][p] == K3).all() and not (near[..., 0] == K3).any()
    assert (cub[..., 0] == K3).sum(axis=-1).max() == 1


def test_collate_carries_the_choice():
    opt = _Opt()
    assert "perspective_resample" not in WB.GpuWarpBatch(opt, rng=random.Random(1)).collate(_samples())       # the default form is unchanged
    opt.perspective_resample = "bicubic"
    batch = WB.GpuWarpBatch(opt, rng=random.Random(1)).collate(_samples())
    assert batch["perspective_resample"] == "bicubic" and (batch["maps"][..., 0] == K3).any() and engine.warp_batch_bicubic(batch)
    near = WB.GpuWarpBatch(opt, rng=random.Random(1), perspective_resample="nearest").collate(_samples())      # the keyword overrides
    assert "perspective_resample" not in near and not (near["maps"][..., 0] == K3).any() and not engine.warp_batch_bicubic(near)
    assert torch.equal(near["maps"][..., 1:], batch["maps"][..., 1:])
    opt.perspective_resample = "nearest"
    assert WB.GpuWarpBatch(opt, perspective_resample="bicubic").collate(_samples())["perspective_resample"] == "bicubic"


class _NoLaunch:
    """A context whose library must not be reached: the refusals come before any launch."""
    device = "cpu"
    owns_stream = False

    @property
    def lib(self):
        raise AssertionError("the library was called")


def test_refusals_come_before_any_launch():
    with pytest.raises(ValueError, match="perspective_resample"):
        A.GpuPerChannelTransform(perspective_resample="lanczos")
    opt = _Opt()
    opt.perspective_resample = "cubic"
    with pytest.raises(ValueError, match="perspective_resample"):
        WB.GpuWarpBatch(opt)
    with pytest.raises(ValueError, match="perspective_resample"):
        WB.GpuWarpBatch(_Opt(), perspective_resample="BICUBIC")
    # two kind-3 rows in one chain
    co = _persp(random.Random(2), 19, 23)
    two = np.zeros((2, 5, 4, 9))
    two[1, 3, 0] = two[1, 3, 2] = [K3] + co
    with pytest.raises(ValueError, match="at most one"):
        A.apply_maps(_NoLaunch(), torch.zeros(2, 5, 23, 19), two)
    with pytest.raises(ValueError, match="at most one"):
        WB.GpuWarpBatch(_Opt(), perspective_resample="bicubic").collate(_samples(), maps=two)
    c = _warp_case(5, seed=1)
    with pytest.raises(ValueError, match="at most one"):
        engine.op_warp_batch(_NoLaunch(), c["body"], c["inp"], c["tgt"], two, MEAN, STD, 40, 3, 5, 24, 32, 5, bicubic=True)
    # kind 3 handed to the entry points that resample NEAREST
    one = np.zeros((2, 5, 4, 9))
    one[0, 1, 1] = [K3] + co
    with pytest.raises(ValueError, match="kind 3"):
        engine.op_warp_batch(_NoLaunch(), c["body"], c["inp"], c["tgt"], one, MEAN, STD, 40, 3, 5, 24, 32, 5)
    with pytest.raises(ValueError, match="kind 3"):
        WB.GpuWarpBatch(_Opt()).collate(_samples(), maps=one)
    with pytest.raises(ValueError, match="perspective_resample"):
        engine.warp_batch_bicubic({"perspective_resample": "cubic"})
