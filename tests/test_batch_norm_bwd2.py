"""batch_norm.hip batch_norm_bwd2 -- the second-order (reverse over reverse) step through y = act(BatchNorm2d(x)) in training mode --
through the model-free entry point swn_op_batch_norm_act_bwd2, against torch's float64 double backward

    y  = act(F.batch_norm(x, None, None, gamma, beta, True))
    gx = autograd.grad(y, x, gy, create_graph=True)
    (ax, uy, dgamma) = autograd.grad((gx * u).sum(), (x, gy, gamma))

gamma is drawn with both signs and beta != 0, so the branch of the activation (taken from z = gamma xh + beta) differs from the sign
of xh.  LeakyReLU's slope is float32(0.2) on both sides, the constant the fp32 module computes with.

Inputs stay off the kink in z (_off_the_kink_bn, the scheme of tests/test_norm_act_ops.py::_off_the_kink): the kernels form z as
x * scale + shift in fp32, scale = fl(gamma rstd), shift = fl(beta - mean scale), which is off the float64 z by a few U a with
a = |gamma| (2 |mean| rstd + |xh|) + |beta| (one U per rounding of x scale, mean scale, the shift and the sum).  Every element with
|z| < 16 U a is moved away from the kink by 64 U a / (|gamma| rstd) until none is left, so both sides take the same branch
everywhere and no element is excluded from a comparison.

Bar (that of test_norm_act_bwd2_vs_float64): 4 x the distance of torch's own fp32 CPU double backward to float64 on the same
inputs, at least 2^-23 -- element-wise over the channel's max|ref| (the vector's, for dgamma) and as rel-L2 -- for uy, ax, dgamma.

Worst figures on the MI355X over all cases (the BN2 lines the test prints): share of the bar uy 0.15, ax 0.19, dgamma 0.12; worst
element-wise error over the channel's max|ref| 2.5e-7 (ax), worst rel-L2 9.0e-8 (ax).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from swapnet_amd import engine
from tests import backends
from tests.test_batch_norm import CASES, plan_chunks

U = 2.0 ** -24
EPS = 1e-5
SLOPE = float(np.float32(0.2))
NONE, LRELU = 0, 1
ACT_NAMES = ("none", "lrelu")

# (N, H, W): 63 pixels per image (below one chunk) and an odd image count across the reduction
SHAPES = [(2, 7, 9), (3, 31, 31)]
# C 8: several pixel rows per block; 320: more than one 16-channel finalize block with 80 float4 lanes per row (3 rows, 16 idle
# lanes); 512
CHANNELS = [8, 320, 512]
# H*W one row above a multiple of the pixel chunk (tests/test_batch_norm.py's chunk case, here as one group)
CHUNK_CASE = (CASES["chunk+1"][0], CASES["chunk+1"][2], CASES["chunk+1"][3], CASES["chunk+1"][4])
ALL_CASES = [(n, c, h, w) for c in CHANNELS for n, h, w in SHAPES] + [(CHUNK_CASE[0], CHUNK_CASE[3], CHUNK_CASE[1], CHUNK_CASE[2])]


def _cm(v):
    return v.mean(axis=(0, 2, 3), keepdims=True)


def _stats64(x64):
    mean = _cm(x64)
    return mean, 1.0 / np.sqrt(_cm((x64 - mean) ** 2) + EPS)


def _margin(x, gamma, beta):
    """(z, a, |gamma| rstd, sign(gamma)) in float64: the pre-activation, the scale of its fp32 round-off (module docstring) and
    dz/dx."""
    x64 = x.astype(np.float64)
    g, b = gamma.astype(np.float64)[None, :, None, None], beta.astype(np.float64)[None, :, None, None]
    mean, rstd = _stats64(x64)
    xh = (x64 - mean) * rstd
    return g * xh + b, np.abs(g) * (2 * np.abs(mean) * rstd + np.abs(xh)) + np.abs(b), np.abs(g) * rstd, np.sign(g)


def _off_the_kink_bn(x, gamma, beta):
    for _ in range(9):
        z, a, slope, sg = _margin(x, gamma, beta)
        near = np.abs(z) < 16 * U * a
        if not near.any():
            return x
        step = 64 * U * a / slope * sg
        x = np.where(near, x.astype(np.float64) + np.where(z >= 0, step, -step), x.astype(np.float64)).astype(np.float32)
    raise AssertionError("elements within 16 U a of the kink are left after 8 rounds")


@functools.lru_cache(maxsize=None)
def _inputs(N, C, H, W):
    rng = np.random.default_rng(7000 + C + H)
    x = (rng.standard_normal((N, C, H, W)) * 3 + 1.5).astype(np.float32)
    gamma = ((1.0 + 0.3 * rng.standard_normal(C)) * np.where(rng.random(C) < 0.5, -1.0, 1.0)).astype(np.float32)
    gamma = np.where(np.abs(gamma) < 0.1, np.float32(0.5), gamma).astype(np.float32)
    beta = (0.5 * rng.standard_normal(C)).astype(np.float32)
    beta = np.where(beta == 0, np.float32(0.25), beta).astype(np.float32)
    assert (gamma > 0).any() and (gamma < 0).any()
    x = _off_the_kink_bn(x, gamma, beta)
    gy, u = rng.standard_normal(x.shape).astype(np.float32), rng.standard_normal(x.shape).astype(np.float32)
    return x, gy, u, gamma, beta


def _double_backward(x, gy, u, gamma, beta, act, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    gt = torch.from_numpy(gy).to(dtype).requires_grad_(True)
    wt = torch.from_numpy(gamma).to(dtype).requires_grad_(True)
    bt = torch.from_numpy(beta).to(dtype)
    ut = torch.from_numpy(u).to(dtype)
    z = F.batch_norm(xt, None, None, wt, bt, True, 0.1, EPS)
    y = F.leaky_relu(z, SLOPE) if act == LRELU else z
    gx, = torch.autograd.grad(y, xt, gt, create_graph=True)
    ax, uy, dg = torch.autograd.grad((gx * ut).sum(), (xt, gt, wt))
    return tuple(t.detach().double().numpy() for t in (uy, ax, dg))


@functools.lru_cache(maxsize=None)
def _reference(N, C, H, W, act):
    """(float64, fp32) double backward of torch on the CPU: computed once per case and shared."""
    a = _inputs(N, C, H, W)
    return _double_backward(*a, act, torch.float64), _double_backward(*a, act, torch.float32)


def _figs(got, ref):
    if ref.ndim == 4:
        pm = np.abs(ref).max(axis=(0, 2, 3), keepdims=True)
    else:
        pm = np.abs(ref).max()
    assert bool((pm > 0).all())
    return float((np.abs(got - ref) / pm).max()), float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_the_shapes_cover_what_they_claim():
    n, c, h, w = ALL_CASES[-1]
    nchunk, chunk = plan_chunks(h * w, n, c)
    assert nchunk > 1 and h * w == (nchunk - 1) * chunk + 1                # the last block of every image sees ONE pixel row
    assert plan_chunks(7 * 9, 2, 8)[0] == 1 and 256 // (8 // 4) > 1        # 63 pixels: one chunk, 128 pixel rows per block
    assert -(-320 // 16) > 1 and 256 // (320 // 4) == 3 and 256 % (320 // 4)   # 20 finalize blocks; 3 rows of 80 lanes, 16 idle
    assert plan_chunks(31 * 31, 3, 512)[0] > 1                             # several chunks per image, three images


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: "N%d-C%d-%dx%d" % c)
def test_no_input_is_left_inside_the_margin_of_the_kink(case):
    x, _, _, gamma, beta = _inputs(*case)
    z, a, _, _ = _margin(x, gamma, beta)
    assert bool((np.abs(z) >= 16 * U * a).all())
    x64 = x.astype(np.float64)
    assert bool((np.sign(z) != np.sign(x64 - _cm(x64))).any())             # the branch of z is not that of xh


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: "N%d-C%d-%dx%d" % c)
def test_batch_norm_bwd2_vs_float64(case):
    ctx = backends.gpu_ctx()
    N, C, H, W = case
    x, gy, u, gamma, beta = _inputs(*case)
    t = [torch.from_numpy(a) for a in (x, gy, u, gamma, beta)]
    for act in (NONE, LRELU):
        outs = [engine.op_batch_norm_act_bwd2(ctx, *t, act=act) for _ in range(2)]
        ctx.sync()
        for a, b in zip(*outs):
            assert torch.equal(_bits(a), _bits(b)), "two runs differ"
        ref, t32 = _reference(N, C, H, W, act)
        bad = []
        for which, got, r64, r32 in zip(("uy", "ax", "dgamma"), outs[0], ref, t32):
            dmax, drel = _figs(got.cpu().numpy().astype(np.float64), r64)
            tmax, trel = _figs(r32, r64)
            bmax, brel = 4 * max(tmax, 2.0 ** -23), 4 * max(trel, 2.0 ** -23)
            print("BN2 N%d C%d %dx%d %-5s %-6s dev_max %.3g torch32_max %.3g dev_rel %.3g torch32_rel %.3g share_max %.3g share_rel %.3g"
                  % (N, C, H, W, ACT_NAMES[act], which, dmax, tmax, drel, trel, dmax / bmax, drel / brel))
            if dmax > bmax or drel > brel:
                bad.append((which, ACT_NAMES[act], "max %.3g bar %.3g" % (dmax, bmax), "rel-L2 %.3g bar %.3g" % (drel, brel)))
        assert not bad, (case, bad)


def test_the_host_simulator_refuses_by_name():
    x = torch.randn(2, 8, 4, 4)
    with pytest.raises(NotImplementedError, match="simulator"):
        engine.op_batch_norm_act_bwd2(backends.hostsim_ctx(), x, x, x, torch.ones(8), torch.zeros(8), act=LRELU)
