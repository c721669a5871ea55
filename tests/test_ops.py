"""Operator-level parity: each C-ABI operator against a plain PyTorch fp32 CPU reference of
the same op (and, on the GPU, the MFMA-tiled convolution against the naive checker kernel).

Every test body runs twice: on the CI host simulator (small shapes, `-m "not gpu"`: checks
the engine-side geometry / packing logic) and on the real MI355X (`-m gpu`: the HIP kernels).
Tolerance: 1e-3 relative (north_star), bit-exact for the integer work.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import swapnet_oracle as O
from swapnet_amd import _C
from tests import backends


pytestmark = pytest.mark.small_channel_winograd      # tests/conftest.py: small shapes on the Winograd forms

K4S2, K3REFL, K4S1, K3ZERO, TAIL = 0, 1, 2, 3, 4


def _ctx(kind):
    return backends.gpu_ctx() if kind == "gpu" else backends.hostsim_ctx()


BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def ref_conv(x, w, b, kind, transposed):
    if transposed:
        return F.conv_transpose2d(x, w, b, stride=2, padding=1)
    if kind == K4S2:
        return F.conv2d(x, w, b, stride=2, padding=1)
    if kind == K3REFL:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)
    if kind == K4S1:
        return F.conv2d(x, w, b, stride=1, padding=1)
    if kind == K3ZERO:
        return F.conv2d(x, w, b, stride=1, padding=1)
    up = F.pad(F.interpolate(x, scale_factor=2), (1, 0, 1, 0))        # swapnet_modules.py:85-88
    return F.conv2d(up, w, b, padding=1)


PRODUCED_OUTPUTS = ("x", "x_slot", "y_slot", "z_slot", "dy", "dy_slot", "kscale")       # optional outputs of swn_op_conv_produced, in argument order


def run_conv(ctx, kind, transposed, what, naive, x, w, b, act, y_shape=None, dy=None, produced=None):
    """produced = None: swn_op_conv (x and dY filled from outside the tape).  produced = a dict: swn_op_conv_produced, the same
    convolution between a `pre` and a `post` stage (keys "pre", "post", default 0 = identity) so that its operands are written by
    kernels of the library; x is then the input of the pre stage, dy the gradient of the post stage's output.  The optional
    outputs named in produced["want"] (PRODUCED_OUTPUTS) come back in the dict as CPU tensors."""
    dev = ctx.device
    xd = x.to(dev).contiguous()
    wd = w.to(dev).contiguous()
    bd = b.to(dev).contiguous() if b is not None else None
    n, ci, h, ww = x.shape
    co = w.shape[1] if transposed else w.shape[0]
    if what == 0:
        yd = torch.empty(y_shape, device=dev)
    else:
        yd = dy.to(dev).contiguous()
    if produced is None:
        ctx.lib.call("swn_op_conv", ctx.handle, kind, int(transposed), what, int(naive), _C.ptr(xd), n, ci, h, ww,
                     _C.ptr(wd), co, _C.ptr(bd), act, _C.ptr(yd))
        ctx.sync()
        return {0: yd, 1: wd, 2: xd}[what].cpu()
    pre, post = produced.get("pre", 0), produced.get("post", 0)
    # n, ci, h, w of the call describe the CONV input: behind an upsampling pre stage it is twice x0, behind a max-pool half
    h, ww = (2 * h, 2 * ww) if pre == 3 else ((h // 2, ww // 2) if pre == 4 else (h, ww))
    if what == 2:
        xd = torch.zeros((n, ci, h, ww), device=dev)          # dX out: the gradient with respect to the conv input
    want = produced.get("want", ())
    assert set(want) <= set(PRODUCED_OUTPUTS), want
    shapes = {"x": ((n, ci, h, ww), torch.float32), "dy": (tuple(yd.shape), torch.float32), "kscale": ((8,), torch.int32)}
    outs = {}
    for k in want:
        shape, dt = shapes.get(k, ((256,), torch.float32))
        outs[k] = torch.full(shape, -(2 ** 30) if k == "kscale" else float("nan"), dtype=dt, device=dev)
    ctx.lib.call("swn_op_conv_produced", ctx.handle, kind, int(transposed), what, int(naive), _C.ptr(xd), n, ci, h, ww,
                 _C.ptr(wd), co, _C.ptr(bd), act, _C.ptr(yd), pre, post, *[_C.ptr(outs.get(k)) for k in PRODUCED_OUTPUTS])
    ctx.sync()
    for k, v in outs.items():
        produced[k] = v.cpu()
    return {0: yd, 1: wd, 2: xd}[what].cpu()


# (kind, transposed, N, Ci, H, Co, bias)   -- sim cases are tiny, gpu cases cover every tile path
CONV_CASES_SIM = [
    (K4S2, 0, 2, 3, 16, 8, False), (K4S2, 0, 1, 32, 8, 36, True), (K3REFL, 0, 2, 8, 6, 8, True),
    (K4S1, 0, 2, 8, 9, 5, True), (K3ZERO, 0, 1, 3, 8, 8, True), (TAIL, 0, 1, 12, 6, 19, True),
    (K4S2, 1, 2, 8, 5, 12, False), (K4S2, 1, 1, 4, 3, 3, True),
    (K3REFL, 0, 2, 32, 6, 32, True), (K3ZERO, 0, 1, 32, 8, 64, True),      # Winograd F(2x2,3x3) / F(4x4,3x3)
    (K3REFL, 0, 1, 32, 8, 32, True),                                       # F(4x4,3x3) + reflect fold (10x10 -> 3x3 tiles)
    (K4S1, 0, 1, 32, 8, 32, True),                                         # F(3x3,4x4): 7x7 outputs, ragged tiles
    (K4S1, 0, 2, 32, 6, 1, True),                                          # 1-channel head: taps on the N axis
    # strided Winograd F(4x4,2x2): k4 s2 conv (8x8 -> 4x4: one tile; 12x12 -> 6x6: ragged 2x2 tiles) and transposed conv
    (K4S2, 0, 2, 32, 8, 32, True), (K4S2, 0, 1, 32, 12, 64, False), (K4S2, 1, 2, 32, 4, 32, True), (K4S2, 1, 1, 48, 3, 32, False),
    (TAIL, 0, 2, 32, 8, 19, True), (TAIL, 0, 1, 64, 6, 19, True),         # tail conv in Winograd form (ragged 6x6 -> 2x2 tiles)
]
CONV_CASES_GPU = CONV_CASES_SIM + [
    (K4S2, 0, 3, 64, 40, 128, False),        # fast path, M = 3*400 (ragged tile), N = 128
    (K4S2, 0, 2, 19, 64, 64, False),         # generic path (Ci=19 -> 20), N = 64 tile
    (K4S2, 0, 2, 512, 8, 1024, False),       # split-K (M = 32, K = 8192)
    (K4S2, 0, 1, 22, 64, 64, True),
    (K3REFL, 0, 2, 256, 16, 256, True),      # reflect pad, K = 2304
    (K4S1, 0, 2, 256, 32, 512, True),        # PatchGAN model.8 shape (31x31 out, ragged M)
    (K4S1, 0, 2, 512, 31, 1, True),          # PatchGAN model.11: N = 1
    (K3ZERO, 0, 1, 64, 64, 64, True),        # VGG
    (TAIL, 0, 1, 192, 32, 19, True),         # upsample_and_pad, N = 19
    (K4S2, 1, 2, 1024, 4, 512, False),       # convT, split-K per phase
    (K4S2, 1, 2, 384, 32, 64, False),        # dual_up3
    (K4S2, 1, 1, 128, 64, 3, True),          # texture outermost up conv (round 5: four phases in one launch, tail_fwd4_kernel<1, true>)
    (K4S2, 1, 2, 64, 16, 19, True), (K4S2, 1, 1, 32, 8, 8, False), (K4S2, 1, 1, 48, 6, 16, True), (K4S2, 1, 2, 16, 5, 12, True),   # the same for 20 / 8 / 16 / 12 columns, ragged 256-pixel tiles
    # LDS-DMA ring kernel corner cases: Ci % 16 == 0 but not % 32, N = 64 (256x64 tile), N = 96 / 80 / 48 (columns of
    # the 128-wide tile past Npad are fetched out of range), ragged M, zero / reflect padding rows out of range
    (K4S2, 0, 2, 48, 24, 96, True), (K4S2, 0, 1, 16, 32, 64, True), (K3ZERO, 0, 2, 48, 12, 80, True),
    (K3REFL, 0, 1, 16, 10, 48, True), (K4S1, 0, 3, 48, 9, 40, True), (K4S2, 1, 1, 48, 6, 72, True),
    # Cin % 16 != 0 next to the ring kernel's shapes (register-staged generic loader: per-lane (tap, channel) decode)
    (K4S2, 0, 2, 12, 32, 48, True), (K3REFL, 0, 1, 20, 10, 80, True), (K4S1, 0, 2, 36, 9, 40, True),
    (K4S2, 1, 1, 24, 6, 72, True), (K3ZERO, 0, 2, 3, 32, 64, True), (K4S2, 0, 1, 55, 64, 64, True),
    (K3ZERO, 0, 1, 7, 12, 160, False),
]


@pytest.mark.parametrize("backend", BACKENDS)
def test_conv_forward(backend):
    ctx = _ctx(backend)
    cases = CONV_CASES_GPU if backend == "gpu" else CONV_CASES_SIM
    g = torch.Generator().manual_seed(0)
    for kind, tr, n, ci, h, co, bias in cases:
        k = 3 if kind in (K3REFL, K3ZERO) else 4
        x = torch.randn(n, ci, h, h, generator=g)
        w = torch.randn((ci, co, k, k) if tr else (co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5
        b = torch.randn(co, generator=g) * 0.1 if bias else None
        ref = ref_conv(x, w, b, kind, tr)
        for act, fn in ((0, lambda t: t), (1, lambda t: F.leaky_relu(t, 0.2)), (3, torch.tanh)):
            if tr and act != 0:
                continue            # ConvTranspose2d is always followed by IN in the reference
            out = run_conv(ctx, kind, tr, 0, False, x, w, b, act, ref.shape)
            assert rel(out, fn(ref)) < 1e-4, (backend, kind, tr, n, ci, h, co, act, rel(out, fn(ref)))
            if act != 0:
                continue
            if backend == "gpu":       # tiled MFMA kernel vs the one-thread-per-output checker
                chk = run_conv(ctx, kind, tr, 0, True, x, w, b, act, ref.shape)
                assert rel(out, chk) < 1e-5, ("tiled vs naive", kind, tr, n, ci, h, co)


@pytest.mark.small_channel_winograd
@pytest.mark.parametrize("backend", [pytest.param("sim", id="hostsim"),
                                     pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)])
def test_winograd_layers_of_129_to_192_channels(backend):
    """Stride-1 Winograd layers whose output (or, for the input gradient, input) width falls in (128, 192]: conv_precut_tile answers
    192 there -- the tile of the tail conv's input gradient -- but the 6-point filter transform writes tiles of 64 / 128 only, and
    planning used to fail at the first operand refresh ("wino_filter_transform_pc: ... tile 64 or 128"; advisor, round 3).  Such a
    layer now keeps its fp32 filter planes (engine.cpp wino_precut_tile).  No network of the reference has one; swn_op_conv does."""
    ctx = _ctx(backend)
    g = torch.Generator().manual_seed(3)
    for kind, k, ci, co, h in ((K3REFL, 3, 32, 160, 8), (K3ZERO, 3, 160, 32, 8), (K3REFL, 3, 176, 176, 12), (K4S1, 4, 48, 176, 9)):
        x = torch.randn(2, ci, h, h, generator=g)
        w = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        b = torch.randn(co, generator=g) * 0.1
        ref = ref_conv(x.double(), w.double(), b.double(), kind, 0)
        out = run_conv(ctx, kind, 0, 0, False, x, w, b, 0, ref.shape)
        dy = torch.randn(ref.shape, generator=g)
        xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
        ref_conv(xr, wr, None, kind, 0).backward(dy.double())
        dx = run_conv(ctx, kind, 0, 2, False, torch.zeros_like(x), w, None, 0, dy=dy)
        dw = run_conv(ctx, kind, 0, 1, False, x, torch.zeros_like(w), None, 0, dy=dy)
        for what, a, r in (("fwd", out, ref), ("dgrad", dx, xr.grad), ("wgrad", dw, wr.grad)):
            assert rel(a, r) < 1e-5, (kind, ci, co, what, rel(a, r))


@pytest.mark.parametrize("backend", BACKENDS)
def test_conv_backward(backend):
    ctx = _ctx(backend)
    cases = CONV_CASES_GPU if backend == "gpu" else CONV_CASES_SIM
    g = torch.Generator().manual_seed(1)
    for kind, tr, n, ci, h, co, bias in cases:
        k = 3 if kind in (K3REFL, K3ZERO) else 4
        x = torch.randn(n, ci, h, h, generator=g, requires_grad=True)
        w = (torch.randn((ci, co, k, k) if tr else (co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5).requires_grad_(True)
        ref = ref_conv(x, w, None, kind, tr)
        dy = torch.randn(ref.shape, generator=g)
        gx, gw = torch.autograd.grad(ref, (x, w), dy)
        dw = run_conv(ctx, kind, tr, 1, False, x.detach(), torch.zeros_like(w), None, 0, dy=dy)
        assert rel(dw, gw) < 2e-4, ("wgrad", backend, kind, tr, n, ci, h, co, rel(dw, gw))
        dx = run_conv(ctx, kind, tr, 2, False, torch.zeros_like(x), w.detach(), None, 0, dy=dy)
        assert rel(dx, gx) < 2e-4, ("dgrad", backend, kind, tr, n, ci, h, co, rel(dx, gx))


@pytest.mark.parametrize("backend", BACKENDS)
def test_instance_norm_act(backend):
    ctx = _ctx(backend)
    g = torch.Generator().manual_seed(2)
    shapes = [(2, 8, 5, 7), (3, 36, 4, 4), (1, 1024, 2, 2)] + ([(4, 64, 128, 128), (2, 512, 31, 31), (2, 64, 8, 8), (2, 96, 16, 16), (2, 64, 20, 20), (2, 32, 32, 32), (1, 64, 33, 32)]
                                                          if backend == "gpu" else [])      # <= 1024 pixels, C % 32 == 0: the register-resident kernels
    for n, c, h, w in shapes:
        x = (torch.randn(n, c, h, w, generator=g) * 3 + 1.5).requires_grad_(True)
        for act, fn in ((0, lambda t: t), (1, lambda t: F.leaky_relu(t, 0.2)), (2, F.relu)):
            ref = fn(F.instance_norm(x, eps=1e-5))
            xd = x.detach().to(ctx.device).contiguous()
            yd = torch.empty_like(xd)
            ctx.lib.call("swn_op_instance_norm_act", ctx.handle, _C.ptr(xd), n, c, h, w, act, _C.ptr(yd))
            assert rel(yd.cpu(), ref.detach()) < 1e-5
            dy = torch.randn(ref.shape, generator=g)
            gx, = torch.autograd.grad(ref, x, dy)
            dyd = dy.to(ctx.device).contiguous()
            dxd = torch.empty_like(xd)
            ctx.lib.call("swn_op_instance_norm_act_bwd", ctx.handle, _C.ptr(xd), _C.ptr(dyd), n, c, h, w, act, _C.ptr(dxd))
            assert rel(dxd.cpu(), gx) < 1e-4, (n, c, h, w, act, rel(dxd.cpu(), gx))


@pytest.mark.parametrize("backend", BACKENDS)
def test_adamw_matches_torch(backend):
    ctx = _ctx(backend)
    g = torch.Generator().manual_seed(3)
    n = 4096 + 8
    p = torch.randn(n, generator=g)
    ref_p = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref_p], lr=4e-4, betas=(0.9, 0.999), weight_decay=0.01)
    pd = p.to(ctx.device).contiguous()
    md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g) * 10 ** float(torch.randint(-6, 1, (1,), generator=g))
        ref_p.grad = grad.clone()
        opt.step()
        gd = grad.to(ctx.device).contiguous()
        ctx.lib.call("swn_op_adamw", ctx.handle, _C.ptr(pd), _C.ptr(gd), _C.ptr(md), _C.ptr(vd), C.c_size_t(n),
                     C.c_float(4e-4), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-8), C.c_float(0.01), step)
        assert torch.allclose(pd.cpu(), ref_p.detach(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("backend", BACKENDS)
def test_roi_align_bit_exact_indices_and_values(backend, golden_dir):
    """Integer work must be bit-exact: corner indices + validity of every sample, and (since
    the bilinear arithmetic is evaluated unfused in the published order) the values too."""
    import os
    ctx = _ctx(backend)
    rois = torch.from_numpy(np.load(os.path.join(golden_dir, "notebook_rois.npz"))["rois"])     # (4,12,4), degenerate boxes
    H = W = 256
    PH = PW = 128 if backend == "gpu" else 16
    extra = torch.tensor([[[0, 0, 255, 255], [255, 0, 255, 0], [10.5, 3.25, 200.75, 77.5], [254, 254, 255, 255]]])
    for r in (rois, extra):
        B, R = r.shape[0], r.shape[1]
        flat = O.reshape_rois(r)
        I = O.roi_align_indices(flat.numpy(), H, W, (PH, PW))
        rd = r.to(ctx.device).contiguous()
        idx = torch.empty((B * R, PH, PW, 4), dtype=torch.int32, device=ctx.device)
        valid = torch.empty((B * R, PH, PW), dtype=torch.uint8, device=ctx.device)
        ctx.lib.call("swn_op_roi_align_indices", ctx.handle, _C.ptr(rd), B * R, H, W, PH, PW, _C.ptr(idx), _C.ptr(valid))
        idx, valid = idx.cpu().numpy(), valid.cpu().numpy().astype(bool)
        assert np.array_equal(valid, I["valid"])
        for j, k in enumerate(("yl", "yh", "xl", "xh")):
            assert np.array_equal(idx[..., j], I[k]), k
        x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(5))
        ref = O.roi_align(x, flat, (PH, PW), 1.0, 1).view(B, R * 3, PH, PW)
        xd = x.to(ctx.device).contiguous()
        out = torch.empty((B, R * 3, PH, PW), device=ctx.device)
        ctx.lib.call("swn_op_roi_align", ctx.handle, _C.ptr(xd), B, 3, H, W, _C.ptr(rd), R, PH, PW, _C.ptr(out))
        assert torch.equal(out.cpu(), ref)


@pytest.mark.gpu
def test_wavefront_gather_roi_align_is_bit_identical(golden_dir, monkeypatch):
    """roi_align_wave_kernel (SWN_ROI_WAVE=1; gather.hip): one wavefront per output row segment, the texel run of the row loaded
    coalesced and the four corners of every lane taken from its neighbours' registers with ds_bpermute -- against the scalar
    one-thread-per-sample kernel and the oracle, bit for bit: the notebook's ROIs (degenerate boxes), full-image and sub-pixel
    boxes, 1-pixel boxes at the border, ROIs wider than 64 / 128 source pixels (several 64-texel segments per row), a pooled
    width that is not a multiple of 64, and a non-square image.  (First run on the MI355X in round 5: green; the wave kernel is the default.)"""
    ctx = _ctx("gpu")
    rois = torch.from_numpy(np.load(os.path.join(golden_dir, "notebook_rois.npz"))["rois"])
    extra = torch.tensor([[[0, 0, 255, 255], [255, 0, 255, 0], [10.5, 3.25, 200.75, 77.5], [254, 254, 255, 255],
                           [3, 200, 250, 201], [100, 0, 101, 255], [0, 0, 63, 63], [-5, -7, 40, 300]]])
    g = torch.Generator().manual_seed(9)
    for r, H, W, PH, PW in ((rois, 256, 256, 128, 128), (extra, 256, 256, 128, 128), (extra, 256, 256, 32, 96), (extra[:, :4] * 0.5, 128, 192, 128, 128)):
        B, R = r.shape[0], r.shape[1]
        x = torch.randn(B, 3, H, W, generator=g)
        ref = O.roi_align(x, O.reshape_rois(r), (PH, PW), 1.0, 1).view(B, R * 3, PH, PW)
        xd, rd = x.to(ctx.device).contiguous(), r.to(ctx.device).contiguous()
        got = {}
        for wave in ("0", "1"):
            monkeypatch.setenv("SWN_ROI_WAVE", wave)
            out = torch.full((B, R * 3, PH, PW), float("nan"), device=ctx.device)
            ctx.lib.call("swn_op_roi_align", ctx.handle, _C.ptr(xd), B, 3, H, W, _C.ptr(rd), R, PH, PW, _C.ptr(out))
            got[wave] = out.cpu()
        assert torch.equal(got["0"], ref), ("scalar kernel", H, W, PH, PW)
        assert torch.equal(got["1"], got["0"]), ("wave kernel", H, W, PH, PW, int((got["1"] != got["0"]).sum()))


@pytest.mark.parametrize("backend", BACKENDS)
def test_label_decode_and_onehot_bit_exact(backend):
    ctx = _ctx(backend)
    g = torch.Generator().manual_seed(6)
    B, Cn, H = (4, 19, 256) if backend == "gpu" else (2, 19, 12)
    x = torch.tanh(torch.randn(B, Cn, H, H, generator=g))
    x[:, :, :3, :3] = 0.0                      # ties -> first index
    xd = x.to(ctx.device).contiguous()
    rgb = torch.empty((B, 3, H, H), dtype=torch.uint8, device=ctx.device)
    ctx.lib.call("swn_op_decode_labels", ctx.handle, _C.ptr(xd), B, Cn, H, H, _C.ptr(rgb))
    assert torch.equal(rgb.cpu(), O.decode_cloth_labels(x))
    lab = torch.empty((B, H, H), dtype=torch.int32, device=ctx.device)
    ctx.lib.call("swn_op_argmax_labels", ctx.handle, _C.ptr(xd), B, Cn, H, H, _C.ptr(lab))
    assert torch.equal(lab.cpu().long(), O.onehot_to_labels(x))
    oh = torch.empty((B, Cn, H, H), device=ctx.device)
    ctx.lib.call("swn_op_labels_to_onehot", ctx.handle, _C.ptr(lab), B, Cn, H, H, _C.ptr(oh))
    assert torch.equal(oh.cpu(), O.labels_to_onehot(lab.cpu().long(), Cn))


@pytest.mark.gpu
def test_conv_wide_ring_tile(monkeypatch):
    """The 128 x 256 (8-wave) instantiation of the LDS-DMA ring kernel, forced (SWN_DMA_WIDE=2; by default it is
    chosen by the launch cost model only where it quantises better): forward, input gradient and the hybrid split-K
    tail, ragged M, N = 256 / 512, against torch."""
    ctx = _ctx("gpu")
    monkeypatch.setenv("SWN_DMA_WIDE", "2")
    g = torch.Generator().manual_seed(3)
    for kind, tr, n, ci, h, co, bias in ((K3REFL, 0, 2, 64, 10, 256, True), (K4S2, 0, 3, 32, 36, 512, False),
                                         (K4S1, 0, 1, 48, 13, 256, True), (K4S2, 1, 2, 64, 9, 256, False),
                                         (K3ZERO, 0, 2, 256, 16, 256, True)):
        k = 3 if kind in (K3REFL, K3ZERO) else 4
        x = torch.randn(n, ci, h, h, generator=g)
        w = torch.randn((ci, co, k, k) if tr else (co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5
        b = torch.randn(co, generator=g) * 0.1 if bias else None
        ref = ref_conv(x, w, b, kind, tr)
        out = run_conv(ctx, kind, tr, 0, False, x, w, b, 0, ref.shape)
        assert rel(out, ref) < 1e-4, (kind, tr, n, ci, h, co, rel(out, ref))
        dy = torch.randn(ref.shape, generator=g)
        xr = x.clone().requires_grad_(True)
        ref_conv(xr, w, b, kind, tr).backward(dy)
        dx = run_conv(ctx, kind, tr, 2, False, torch.zeros_like(x), w, None, 0, dy=dy)
        assert rel(dx, xr.grad) < 1e-4, ("dgrad", kind, tr, n, ci, h, co, rel(dx, xr.grad))


@pytest.mark.gpu
def test_split_main_loop_is_as_accurate_as_the_f32_mfma(monkeypatch):
    """The ring kernels form fp32 products on the 16-bit matrix pipe from two amax-scaled fp16 planes per operand (h h + h l + l h:
    3 fp16 MFMA products, fp32 accumulate; conv_gemm.h / conv_ring.hip -- the three-plane bf16 form of rounds 2-3 left the library in round 5).
    Against a float64 convolution the result must be at least as close as the v_mfma_f32_32x32x2_f32 form (SWN_SPLIT=0) --
    forward, input gradient and weight gradient -- and the two forms must agree to fp32 round-off.  Inputs carry full 24-bit
    mantissas (randn)."""
    ctx = _ctx("gpu")
    g = torch.Generator().manual_seed(11)
    for kind, n, ci, h, co in ((K4S2, 4, 128, 64, 256), (K3REFL, 2, 256, 32, 256), (K4S2, 2, 512, 16, 512)):
        k = 3 if kind == K3REFL else 4
        x = torch.randn(n, ci, h, h, generator=g)
        w = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        y64 = ref_conv(xd, wd, None, kind, 0)
        dy = torch.randn(y64.shape, generator=g)
        gx64, gw64 = torch.autograd.grad(y64, (xd, wd), dy.double())
        res = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("SWN_SPLIT", mode)
            monkeypatch.setenv("SWN_WINOGRAD", "0")
            res[mode] = (run_conv(ctx, kind, 0, 0, False, x, w, None, 0, y64.shape),
                         run_conv(ctx, kind, 0, 2, False, torch.zeros_like(x), w, None, 0, dy=dy),
                         run_conv(ctx, kind, 0, 1, False, x, torch.zeros_like(w), None, 0, dy=dy))
        for what, i, ref in (("fwd", 0, y64), ("dgrad", 1, gx64), ("wgrad", 2, gw64)):
            e_split, e_f32 = rel(res["1"][i], ref), rel(res["0"][i], ref)
            assert e_split <= 1.15 * e_f32 + 2e-8, (what, kind, ci, co, "split %.3e" % e_split, "f32 mfma %.3e" % e_f32)
            assert e_split < 2e-6 and rel(res["1"][i], res["0"][i]) < 2e-6


@pytest.mark.parametrize("backend", BACKENDS)
def test_two_plane_form_on_heavy_tailed_operands(backend, monkeypatch):
    """The two-fp16-plane form scales an operand by ONE power of two per tensor, taken from its amax: an element keeps 22
    mantissa bits only while it lies within 2^-14 of the tensor's largest, below that the low plane runs into fp16's subnormal
    range and the element's error becomes ABSOLUTE, amax * 2^-37 (conv_gemm.h).  A single outlier 2^18 x the bulk -- gradient
    tensors do this -- therefore costs every bulk element 4 bits.  This test pins that price at product level, element-wise
    and not only in rel-L2: forward (outlier in the activations), input gradient (outlier in dY) and weight gradient (outliers
    in both operands) against float64,
        |err| <= 2^-20 conv(|a|, |b|)  +  2^-35 (amax_a conv(1, |b|) + amax_b conv(|a|, 1))  per output element
    (twice the analytic bound: dropped l*l term and per-element representation errors of both operands); the bulk outputs stay
    within 1e-5 relative, two digits inside north_star's 1e-3; and the f32-MFMA form (SWN_SPLIT=0) of the same launch is held
    to the same element-wise bound so that the bound itself is checked against a kernel that has no scaling at all.
    On the host simulator the same launches run through its rounding model of the operand formats (SWN_SIM_PAIR=1: the engine's
    scales, software fp16 cuts, exact products) -- the bound is a property of the FORMAT and must hold there too."""
    ctx = _ctx(backend)
    if backend == "sim":
        monkeypatch.setenv("SWN_SIM_PAIR", "1")
    g = torch.Generator().manual_seed(21)
    monkeypatch.setenv("SWN_WINOGRAD", "0")
    n, ci, h, co, k = 3, 64, 64, 128, 4
    x = torch.randn(n, ci, h, h, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
    big = float(2 ** 18)
    xo = x.clone(); xo[1, 7, 33, 21] = big                       # one activation 2^18 x the bulk (rms 1)
    y_shape = ref_conv(x, w, None, K4S2, 0).shape
    dy = torch.randn(y_shape, generator=g)
    dyo = dy.clone(); dyo[2, 100, 5, 9] = -big                   # one output-gradient element 2^18 x the bulk

    def conv64(a, b):
        return F.conv2d(a.double(), b.double(), None, stride=2, padding=1)

    def bound(absA, amaxA, onesA, absB, amaxB, onesB, f):
        return 2.0 ** -20 * f(absA, absB) + 2.0 ** -35 * (amaxA * f(onesA, absB) + amaxB * f(absA, onesB))

    cases = {}
    # forward: A = x (outlier), B = w
    cases["fwd"] = (lambda: run_conv(ctx, K4S2, 0, 0, False, xo, w, None, 0, y_shape), conv64(xo, w), conv64(x, w),
                    bound(xo.abs(), float(xo.abs().max()), torch.ones_like(xo), w.abs(), float(w.abs().max()), torch.ones_like(w), conv64))
    # input gradient: A = dY (outlier), B = w^T
    def dgrad64(a, b):
        return F.conv_transpose2d(a.double(), b.double(), None, stride=2, padding=1)
    cases["dgrad"] = (lambda: run_conv(ctx, K4S2, 0, 2, False, torch.zeros_like(x), w, None, 0, dy=dyo), dgrad64(dyo, w), dgrad64(dy, w),
                      bound(dyo.abs(), float(dyo.abs().max()), torch.ones_like(dyo), w.abs(), float(w.abs().max()), torch.ones_like(w), dgrad64))
    # weight gradient: both operands are activations, both heavy-tailed
    def wgrad64(a, d):
        a = a.double().requires_grad_(False)
        wz = torch.zeros(co, ci, k, k, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(F.conv2d(a, wz, None, stride=2, padding=1), wz, d.double())[0]
    cases["wgrad"] = (lambda: run_conv(ctx, K4S2, 0, 1, False, xo, torch.zeros_like(w), None, 0, dy=dyo), wgrad64(xo, dyo), wgrad64(x, dy),
                      bound(xo.abs(), float(xo.abs().max()), torch.ones_like(xo), dyo.abs(), float(dyo.abs().max()), torch.ones_like(dyo), wgrad64))
    for what, (run, ref, clean, tol) in cases.items():
        # the outputs no outlier reaches (equal, in float64, to the result without the outliers): their relative error is the
        # price of the shared scale
        far = ref == clean
        assert 0.5 < float(far.double().mean()) < 1.0, (what, float(far.double().mean()))
        for mode in (("1", "0") if backend == "gpu" else ("1",)):
            monkeypatch.setenv("SWN_SPLIT", mode)
            got = run().double()
            err = (got - ref).abs()
            worst = float((err / tol).max())
            rel_far = float((got - ref)[far].norm() / ref[far].norm())
            print("heavy tail %s SWN_SPLIT=%s: worst |err| / bound %.3f   rel-L2 of the bulk outputs %.2e" % (what, mode, worst, rel_far))
            assert worst <= 1.0, (what, mode, worst)
            assert rel_far < 1e-5, (what, mode, rel_far)


@pytest.mark.gpu
def test_split_main_loop_on_one_signed_operands(monkeypatch):
    """The cut of the split main loop is by TRUNCATION, so the three dropped terms (mid*lo, lo*mid, lo*lo, each below
    2^-24 |a||b|) all carry the sign of a*b: with zero-mean operands they average out, with one-signed operands -- post-ReLU
    activations against a positive filter, the image Gram -- they add up to a BIAS.  K = 9216 (the resblock conv run
    direct), non-negative activations, positive weights: the relative error against float64 must stay at the f32 MFMA
    form's level and the signed mean error (the bias) below one fp32 ulp of the result."""
    ctx = _ctx("gpu")
    g = torch.Generator().manual_seed(12)
    monkeypatch.setenv("SWN_WINOGRAD", "0")
    for kind, n, ci, h, co in ((K3REFL, 2, 1024, 16, 256), (K4S2, 2, 256, 32, 128)):
        k = 3 if kind == K3REFL else 4
        x = torch.relu(torch.randn(n, ci, h, h, generator=g)) + 0.01
        w = torch.randn(co, ci, k, k, generator=g).abs() * (2.0 / (ci * k * k)) ** 0.5
        y64 = ref_conv(x.double(), w.double(), None, kind, 0)
        dy = torch.rand(y64.shape, generator=g) + 0.1
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        gx64, gw64 = torch.autograd.grad(ref_conv(xd, wd, None, kind, 0), (xd, wd), dy.double())
        res = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("SWN_SPLIT", mode)
            res[mode] = (run_conv(ctx, kind, 0, 0, False, x, w, None, 0, y64.shape),
                         run_conv(ctx, kind, 0, 2, False, torch.zeros_like(x), w, None, 0, dy=dy),
                         run_conv(ctx, kind, 0, 1, False, x, torch.zeros_like(w), None, 0, dy=dy))
        for what, i, ref in (("fwd", 0, y64), ("dgrad", 1, gx64), ("wgrad", 2, gw64)):
            e_split, e_f32 = rel(res["1"][i], ref), rel(res["0"][i], ref)
            bias = float(((res["1"][i].double() - ref) / ref).mean())
            bias32 = float(((res["0"][i].double() - ref) / ref).mean())
            print("one-signed K=%d %s: split %.2e (bias %+.2e)  f32 mfma %.2e (bias %+.2e)" % (ci * k * k, what, e_split, bias, e_f32, bias32))
            assert e_split <= 1.25 * e_f32 + 6e-8, (what, kind, "split %.3e" % e_split, "f32 mfma %.3e" % e_f32)
            assert abs(bias) < 1.2e-7, (what, kind, "relative bias of the split form", bias)
