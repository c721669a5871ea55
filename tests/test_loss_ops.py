"""Operator-level float64 parity of the loss kernels (csrc/losses.hip) and of bias_grad (norm_act.hip).

Every kernel is called alone through swn_op_gan_loss / swn_op_loss / swn_op_bias_grad and compared with a plain float64
formula on the same fp32 operands.  Each body runs on the CI host simulator (tiny shapes) and on the MI355X.

What holds in every loss test (`_call`): the same call twice gives bit-equal loss and gradient (the fixed-order sums of
losses.hip); da = NULL gives the same loss bits; with `accumulate` the incoming gradient is randn and the result is old +
reference; pad channels of the gradient buffer at or above round-up-4(C) keep the sentinel bit pattern, those in
[C, round-up-4(C)) hold zeros after a non-accumulating ce_argmax_loss and the sentinel after every other call (ops.h).

Tolerances.  Bit-exact: the L1 gradient, b == a for the Gram, the CE label position, run-to-run equality, pads.
Loss values of BCE / LSGAN / WGAN / CE / normalised MSE: partials are fp64 sums of fp32 per-element terms, so the error of the
mean is at most the mean per-term error.  The figure is  |loss - loss64| / mean|term64| ; the same inputs go through a torch
fp32 CPU evaluation of the terms, whose figure is  mean|term32 - term64| / mean|term64| , at least 2^-24 (half an ulp of a
term: the torch figure is a small sample at 1 pixel, and exactly 0 for WGAN); the bar is 4 x that (another libm,
FMA contraction) plus 2^-24 |loss64| / mean|term64| for the one rounding of the fp32 result, which the term-wise figure does
not contain.  Gradients of those kernels: max|err| in units of gscale * 2^-24 and rel-L2, each at most 4 x the torch-fp32
figure.  The torch figure is a sample (a maximum over nine distinct values in the "edges" map, one element at 1x1x1x1, exact
for WGAN), so it is floored at what ANY fp32 evaluation may be off: element-wise max(1 unit, 2^-24 |g|) -- half an ulp of an O(1)
intermediate (sigmoid, softmax) times gscale, and half an ulp of the element itself; rel-L2 2^-24, or one element off by one unit.  With accumulate one more rounding of old + g is allowed:
2^-24 |old + g| per element.  L1 loss: 2^-23 relative (one rounded subtraction per term, one rounding of the result).
Gram: analytic bound from the fp32 chain length of the path (see _gram_ref_and_bound), |err| <= 2 x bound.  bias_grad: fp64
partials and one rounding, |db - ref| <= 2^-23 |ref| + 2^-45 sum|dy|.
"""
import numpy as np
import pytest
import torch

from swapnet_amd import engine
from tests import backends

BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]
U = 2.0 ** -24
SENT = engine.PAD_SENTINEL


def _ctx(kind):
    return backends.gpu_ctx() if kind == "gpu" else backends.hostsim_ctx()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ru4(c):
    return (c + 3) // 4 * 4


def _pads(c):
    r = _ru4(c) - c
    return [0, 4] if r == 0 else [r, r + 4]


def _f32(x):
    return float(np.float32(x))


def _record(kernel, case, **figs):
    print("LOSSOPS %-10s %-44s %s" % (kernel, case, "  ".join("%s %.3g" % kv for kv in figs.items())))


def _call(ctx, kind, a, b, pad_c, scale, acc, n0=0, nloc=-1, seed=0):
    """The call under test three times (see the module docstring).  Returns (loss as float, gradient, incoming gradient)."""
    ng = a.shape[0] if nloc < 0 else nloc
    old = torch.randn((ng,) + tuple(a.shape[1:]), generator=_gen(1000 + seed)) if acc else None
    l1, d1, p1 = engine.op_loss(ctx, kind, a, b, pad_c, scale, acc, n0, nloc, grad=old)
    l2, d2, p2 = engine.op_loss(ctx, kind, a, b, pad_c, scale, acc, n0, nloc, grad=old)
    l3, _, _ = engine.op_loss(ctx, kind, a, b, pad_c, scale, acc, n0, nloc, want_grad=False)
    ctx.sync()
    assert torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(d1), _bits(d2)), "two runs differ"
    assert torch.equal(_bits(l1), _bits(l3)), "loss differs without a gradient view"
    if pad_c:
        c, pb = a.shape[1], _bits(p1)
        assert torch.equal(pb, _bits(p2))
        soft = pb[:, :_ru4(c) - c]
        assert bool((pb[:, _ru4(c) - c:] == SENT).all()), "a pad channel at or above round-up-4(C) was written"
        # ops.h: ce_argmax_loss moves whole float4 groups and writes zeros there (adds zero when it accumulates); every other kernel
        # writes the C logical channels only
        want = 0 if kind == engine.LOSS_CE and not acc else SENT
        assert bool((soft == want).all()), "pad channels in [C, round-up-4(C)): expected %s" % ("zeros" if want == 0 else "the sentinel")
    return float(l1.cpu().double()), d1.cpu(), old


def _check_loss(kernel, case, loss, term64, term32):
    """The 4 x torch-fp32 bar on a loss value (module docstring).  term64 / term32: per-element terms."""
    ref = float(term64.mean())
    mt = float(term64.abs().mean())
    dev = abs(loss - ref) / max(mt, 1e-300)
    t32 = float((term32.double() - term64).abs().mean()) / max(mt, 1e-300)
    bar = 4.0 * max(t32, U) + U * abs(ref) / max(mt, 1e-300)
    _record(kernel, case + " loss", dev=dev, torch32=t32, bar=bar)
    assert dev <= bar, (kernel, case, "loss %.9g ref %.9g: %.3g of mean|term| > bar %.3g" % (loss, ref, dev, bar))


def _check_grad(kernel, case, d, g64, g32, unit, old=None):
    """Element-wise and rel-L2 bars on a gradient.  unit: gscale * 2^-24 (a scalar, or per element)."""
    ref = g64 if old is None else old.double() + g64
    slack = 0.0 if old is None else U * ref.abs()            # the one extra rounding of old + g
    err = (d.double() - ref).abs()
    e32 = (g32.double() - g64).abs()
    floor = torch.maximum(U * g64.abs() / unit, torch.ones_like(g64))     # half an ulp of the element, and of an O(1) intermediate
    t_max = max(float((e32 / unit).max()), float(floor.max()))
    dev_max = float(((err - slack).clamp(min=0) / unit).max())
    _record(kernel, case + (" grad+acc" if old is not None else " grad"), dev_max=dev_max, torch32_max=t_max)
    assert dev_max <= 4.0 * t_max, (kernel, case, "max|err| %.3g units > 4 x %.3g" % (dev_max, t_max))
    if old is None:
        n64 = float(g64.norm()) + 1e-300
        dev_rel, t_rel = float(err.norm()) / n64, max(float(e32.norm()) / n64, U, float((unit * torch.ones_like(g64)).max()) / n64)
        _record(kernel, case + " grad", dev_rel=dev_rel, torch32_rel=t_rel)
        assert dev_rel <= 4.0 * t_rel, (kernel, case, "rel-L2 %.3g > 4 x %.3g" % (dev_rel, t_rel))


# ---- GAN losses (swn_op_gan_loss) -------------------------------------------------------------------------------------------
def _gan_map(family, shape, seed):
    n = int(np.prod(shape))
    if family == "randn":
        return torch.randn(shape, generator=_gen(seed))
    vals = torch.tensor([0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0])
    return vals[torch.arange(n) % len(vals)].reshape(shape).clone()


GAN_SHAPES = [(1, 1, 1, 1), (1, 1, 15, 17), (1, 1, 16, 16), (1, 1, 1, 257), (1, 1, 520, 512)]       # 1, 255, 256, 257, > 256 * 1024 elements


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["bce", "lsgan", "wgan"])
@pytest.mark.parametrize("family", ["randn", "edges"])
def test_gan_loss_vs_float64(backend, mode, family):
    """All three GAN modes, smoothed labels 0.9 / 0.1, one block / a ragged second block / a wrapped grid-stride loop; the BCE
    reference is max(x,0) - x t + log1p(exp(-|x|)) in float64.  257 elements = 2 partials for finalize_kernel."""
    ctx = _ctx(backend)
    for shape in GAN_SHAPES:
        for label, real in ((0.9, True), (0.1, False)):
            x = _gan_map(family, shape, 3)
            numel = x.numel()
            scale = 0.5
            t = _f32(label) if mode < 2 else (-1.0 if real else 1.0)
            gs = _f32(np.float32(scale) / np.float32(numel))
            outs = [engine.op_gan_loss(ctx, x, mode, label, real, scale) for _ in range(2)]
            l3, _ = engine.op_gan_loss(ctx, x, mode, label, real, scale, want_grad=False)
            ctx.sync()
            assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
            assert torch.equal(_bits(outs[0][0]), _bits(l3))
            loss, d = float(outs[0][0].cpu().double()), outs[0][1].cpu()

            def terms(v, tt, g):
                if mode == 0:
                    return v.clamp(min=0) - v * tt + torch.log1p(torch.exp(-v.abs())), (torch.sigmoid(v) - tt) * g
                if mode == 1:
                    return (v - tt) ** 2, 2 * (v - tt) * g
                return tt * v, torch.full_like(v, tt) * g
            t64, g64 = terms(x.double(), t, gs)
            t32, g32 = terms(x, torch.tensor(t, dtype=torch.float32), torch.tensor(gs, dtype=torch.float32))
            case = "mode%d %s %s t=%.1f" % (mode, family, "x".join(map(str, shape)), label)
            _check_loss("gan", case, loss, t64, t32)
            _check_grad("gan", case, d, g64, g32, gs * U)


# ---- cross entropy vs argmax(target) -------------------------------------------------------------------------------------------
def _ce_inputs(C, shape, family, seed):
    g = _gen(seed)
    n, h, w = shape
    if family == "tanh":
        lg = torch.tanh(torch.randn((n, C, h, w), generator=g))
    elif family == "wide":
        lg = torch.randn((n, C, h, w), generator=g) * 30
    else:                                       # one +80 among -80s: the softmax saturates, lmax must be subtracted
        lg = torch.full((n, C, h, w), -80.0)
        hot = torch.randint(0, C, (n, 1, h, w), generator=g)
        lg.scatter_(1, hot, 80.0)
    tg = torch.rand((n, C, h, w), generator=g)
    # exact ties, by pixel index mod 4: all-equal row; two equal maxima; the maximum in the last channel; untouched
    P = tg.permute(0, 2, 3, 1).reshape(-1, C)
    idx = torch.arange(P.shape[0])
    P[idx % 4 == 0] = 0.5
    if C > 1:
        two = idx % 4 == 1
        first = torch.randint(0, C - 1, (P.shape[0],), generator=g)
        second = (first + 1 + (torch.rand(P.shape[0], generator=g) * (C - 1 - first).float()).long()).clamp(max=C - 1)
        rows = torch.nonzero(two).flatten()
        P[rows, first[rows]] = 2.0
        P[rows, second[rows]] = 2.0
        P[idx % 4 == 2, C - 1] = 3.0
    tg = P.reshape(n, h, w, C).permute(0, 3, 1, 2).contiguous()
    return lg, tg


def _ce_ref(lg, tg, gs, dtype):
    n, C, h, w = lg.shape
    L = lg.permute(0, 2, 3, 1).reshape(-1, C).to(dtype)
    label = torch.from_numpy(np.argmax(tg.permute(0, 2, 3, 1).reshape(-1, C).numpy(), axis=1))     # numpy: the FIRST maximal index
    d = L - L.max(dim=1, keepdim=True).values
    e = torch.exp(d)
    se = e.sum(dim=1, keepdim=True)
    term = torch.log(se).squeeze(1) - d.gather(1, label[:, None]).squeeze(1)
    onehot = torch.zeros_like(L).scatter_(1, label[:, None], 1.0)
    g = (e / se - onehot) * torch.tensor(gs, dtype=dtype)
    return term, g.reshape(n, h, w, C).permute(0, 3, 1, 2).contiguous(), label


CE_SHAPES = [(1, 1, 1), (1, 15, 17), (1, 1, 257)]          # 1, 255, 257 pixels (257 pixels = 2 partials)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("C", [1, 3, 4, 19, 20, 31, 32])
def test_ce_vs_float64(backend, C):
    """ce_kernel at every C around the float4 groups, with strided views; saturating logits; exact ties in the target (the
    label is the first maximal index: the only negative entry of a pixel's gradient row)."""
    ctx = _ctx(backend)
    shapes = CE_SHAPES + ([(1, 513, 512)] if backend == "gpu" and C in (3, 19, 32) else [])          # > 262144 pixels: the loop wraps
    for shape in shapes:
        big = shape[1] * shape[2] > 1000
        for family in (("tanh",) if big else ("tanh", "wide", "sat")):
            lg, tg = _ce_inputs(C, shape, family, 7 + C)
            pixels = shape[0] * shape[1] * shape[2]
            scale = 3.0
            gs = _f32(np.float32(scale) / np.float32(pixels))
            t64, g64, label = _ce_ref(lg, tg, gs, torch.float64)
            t32, g32, _ = _ce_ref(lg, tg, gs, torch.float32)
            for pad_c in (_pads(C)[:1] if big else _pads(C)):
                for acc in (0, 1):
                    case = "C%d pad%d %s %s" % (C, pad_c, family, "x".join(map(str, shape)))
                    loss, d, old = _call(ctx, engine.LOSS_CE, lg, tg, pad_c, scale, acc, seed=C)
                    _check_loss("ce", case, loss, t64, t32)
                    _check_grad("ce", case, d, g64, g32, gs * U, old)
                    if not acc and family == "tanh" and C > 1:
                        D = d.permute(0, 2, 3, 1).reshape(-1, C)
                        assert bool(((D < 0).sum(dim=1) == 1).all())
                        assert torch.equal(D.argmin(dim=1), label), "the label is not the first maximal target channel"


@pytest.mark.parametrize("backend", BACKENDS)
def test_ce_rejects_33_channels(backend):
    ctx = _ctx(backend)
    x = torch.zeros(1, 33, 2, 2)
    with pytest.raises(ValueError):
        engine.op_loss(ctx, engine.LOSS_CE, x, x, 3)


# ---- L1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("C", [1, 3, 4, 19])
def test_l1_vs_float64(backend, C):
    """l1_kernel: the loss to 2^-23 relative; the gradient takes the three values {-g, 0, +g}, g = fp32(scale / numel), bit for bit,
    and exactly 0 where a == b.  Operands in [-1, 1] and equal or >= 2^-24 apart: no subnormal difference, so the sign of the fp32
    difference is that of the float64 one."""
    ctx = _ctx(backend)
    for shape in ((1, 1, 1), (1, 15, 17), (1, 1, 257), (2, 300, 301)):          # numel C * 180600 > 262144 for every C but 1
        if shape[0] == 2 and C == 1:
            shape = (2, 400, 401)                                                 # 320800 elements
        n, h, w = shape
        a = torch.rand((n, C, h, w), generator=_gen(11 + C)) * 2 - 1
        b = torch.rand((n, C, h, w), generator=_gen(12 + C)) * 2 - 1
        if h * w > 1:
            b[:, :, : max(1, h // 3)] = a[:, :, : max(1, h // 3)]                  # a block of exactly equal elements
        numel = a.numel()
        scale = 0.7
        g = np.float32(scale) / np.float32(numel)
        diff = a.double() - b.double()
        assert bool(((diff == 0) | (diff.abs() >= 2.0 ** -30)).all())
        ref = float(diff.abs().mean())
        sign = torch.sign(diff).float()
        gref = sign * torch.tensor(g)
        for pad_c in _pads(C):
            for acc in (0, 1):
                loss, d, old = _call(ctx, engine.LOSS_L1, a, b, pad_c, scale, acc, seed=C)
                dev = abs(loss - ref) / max(ref, 1e-300)
                _record("l1", "C%d pad%d %s acc%d" % (C, pad_c, "x".join(map(str, shape)), acc), dev=dev, bar=2.0 ** -23)
                assert dev <= 2.0 ** -23, (loss, ref)
                want = gref if not acc else old + gref                              # fp32 old + g
                assert torch.equal(d, want), "L1 gradient is not {-g, 0, +g} (+ old)"
                if not acc:
                    assert bool((d[diff == 0] == 0).all())


# ---- normalised MSE (content term) --------------------------------------------------------------------------------------------------
EPS32 = _f32(1e-8)


def _nmse_ref(f, t, gs, dtype):
    """Closed form of losses.hip: y = x / (s + eps), dx = g / (s + eps) - x (x.g) / (s (s + eps)^2), the second term dropped at
    s == 0 (the kernel's convention: g / eps there, where autograd through sqrt gives NaN)."""
    n, C, h, w = f.shape
    F_ = f.permute(0, 2, 3, 1).reshape(-1, C).to(dtype)
    T_ = t.permute(0, 2, 3, 1).reshape(-1, C).to(dtype)
    eps = torch.tensor(EPS32, dtype=dtype)
    sf = (F_ * F_).sum(dim=1, keepdim=True).sqrt()
    st = (T_ * T_).sum(dim=1, keepdim=True).sqrt()
    inf = 1 / (sf + eps)
    diff = F_ * inf - T_ / (st + eps)
    g = diff * torch.tensor(gs, dtype=dtype)
    dot = (F_ * g).sum(dim=1, keepdim=True)
    k2 = torch.where(sf > 0, dot * inf * inf / torch.where(sf > 0, sf, torch.ones_like(sf)), torch.zeros_like(sf))
    dx = g * inf - F_ * k2
    back = lambda v: v.reshape(n, h, w, C).permute(0, 3, 1, 2).contiguous()
    return back(diff * diff), back(dx), sf.squeeze(1)


def _nmse_inputs(C, shape, kinds, seed):
    """Post-ReLU features; pixel p (row-major) gets the special type kinds[p] where given."""
    n, h, w = shape
    g = _gen(seed)
    f = torch.relu(torch.randn((n, C, h, w), generator=g))
    t = torch.relu(torch.randn((n, C, h, w), generator=g))
    F_, T_ = f.permute(0, 2, 3, 1).reshape(-1, C), t.permute(0, 2, 3, 1).reshape(-1, C)
    for p, k in enumerate(kinds):
        if F_[p].norm() == 0:
            F_[p, 0] = 1.0
        if k in ("f0", "both0"):
            F_[p] = 0
        if k in ("t0", "both0"):
            T_[p] = 0
        if k == "tiny":
            F_[p] = F_[p] / F_[p].norm() * 1e-6
        if k == "huge":
            F_[p] = F_[p] / F_[p].norm() * 1e4
    back = lambda v: v.reshape(n, h, w, C).permute(0, 3, 1, 2).contiguous()
    return back(F_), back(T_)


NMSE_KINDS = ("f0", "t0", "both0", "tiny", "huge")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("C", [4, 64, 252, 256, 260, 512])
def test_normed_mse_vs_float64(backend, C):
    """normed_mse_kernel (one wave per pixel; C = 260 puts one lane into the second float4 group) at 1, 3, 5 pixels and above the
    2048 x 4 grid, on post-ReLU features with pixels that are all-zero in f, in t, in both, of norm 1e-6 and of norm 1e4.
    CONVENTION (asserted here, stated in ops.h): at a pixel with |f| == 0 the gradient is g / eps = (0 - t/(|t|+eps)) * gscale * 1e8,
    finite, where the reference program's autograd (sqrt'(0) * 0) gives NaN.  The element-wise bar at the zero-norm and norm-1e-6
    pixels is scaled by that pixel's 1 / (s + eps): the error is relative to the pixel's own gradient magnitude."""
    ctx = _ctx(backend)
    cases = [((1, 1, 1), (k,)) for k in (None,) + NMSE_KINDS] + [((1, 1, 3), NMSE_KINDS[:3]), ((1, 5, 1), NMSE_KINDS)]
    if backend == "gpu" or C <= 64:
        cases.append(((1, 96, 96), (None, None, None) + NMSE_KINDS))
    for shape, kinds in cases:
        f, t = _nmse_inputs(C, shape, [k for k in kinds], 21 + C)
        numel = f.numel()
        scale = 1.5
        gs = _f32(np.float32(2.0) * np.float32(scale) / np.float32(numel))
        t64, g64, sf = _nmse_ref(f, t, gs, torch.float64)
        t32, g32, _ = _nmse_ref(f, t, gs, torch.float32)
        assert bool(torch.isfinite(g64).all())
        small = sf <= 1e-5                                                  # the zero-norm and the norm-1e-6 pixels
        unit = torch.where(small, 1.0 / (sf + EPS32), torch.ones_like(sf)) * gs * U
        unit = unit.reshape(shape[0], shape[1], shape[2], 1).permute(0, 3, 1, 2)
        for pad_c in (0, 4):
            for acc in (0, 1):
                case = "C%d pad%d %s %s" % (C, pad_c, "x".join(map(str, shape)), kinds[0] if len(kinds) == 1 else "mixed")
                loss, d, old = _call(ctx, engine.LOSS_NORMED_MSE, f, t, pad_c, scale, acc, seed=C)
                assert bool(torch.isfinite(d).all()), "the zero-norm convention: finite gradient"
                _check_loss("nmse", case, loss, t64, t32)
                _check_grad("nmse", case, d, g64, g32, unit, old)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("C", [6, 516])
def test_normed_mse_rejects_bad_channels(backend, C):
    ctx = _ctx(backend)
    x = torch.ones(1, C, 2, 2)
    with pytest.raises(ValueError):
        engine.op_loss(ctx, engine.LOSS_NORMED_MSE, x, x, (-C) % 4)


# ---- image Gram (style term) ----------------------------------------------------------------------------------------------------------
def _gram_chain(R, HW, whole):
    """fp32 chain length of the path gram_style_loss takes (the launcher's rule): 64-pixel chunks on the LDS path, per_split pixels
    per block on the tiled one."""
    if R <= 128 and whole:
        return 64
    nsplit = max(1, min(64, HW // 256))
    per = (HW + nsplit - 1) // nsplit
    return (per + 63) // 64 * 64


def _gram_ref_and_bound(a, b, scale, n0, nloc, L):
    """float64 loss and gradient of scale * mse(Gram(a), Gram(b)) w.r.t. a (rows [n0*C, (n0+nloc)*C)), and the propagated fp32 bound:
    every Gram entry is a sum of fp32 fmaf chains of length <= L, partials added in fp64: |dGa| <= L u |A||A|^T (same for B); through
    d = Ga - Gb, loss = mean d^2 (+ one rounding of the result), dG = fp32(2 d) * fp32(scale / R^2) (3 roundings), the symmetrisation
    (1 rounding) and da = (dG + dG^T) A with its own R-long fp32 chain."""
    N, C, H, W = a.shape
    R, HW = N * C, H * W
    A, B = a.double().reshape(R, HW), b.double().reshape(R, HW)
    Ga, Gb = A @ A.T, B @ B.T
    Ed = L * U * (A.abs() @ A.abs().T + B.abs() @ B.abs().T)
    d = Ga - Gb
    loss = float((d * d).mean())
    loss_bound = float((2 * d.abs() * Ed + Ed * Ed).mean()) + U * loss
    gs = _f32(np.float32(scale) / np.float32(R * R))
    dG = 2 * d * gs
    EdG = 2 * gs * Ed + 3 * U * dG.abs()
    g = dG + dG.T
    Eg = EdG + EdG.T + U * g.abs()
    rows = slice(n0 * C, (n0 + nloc) * C)
    da = g[rows] @ A
    bound = Eg[rows] @ A.abs() + R * U * (g[rows].abs() @ A.abs())
    return loss, loss_bound, da.reshape(nloc, C, H, W), bound.reshape(nloc, C, H, W)


def _gram_operands(N, H, W, family, seed):
    a = torch.rand((N, 3, H, W), generator=_gen(seed)) * 2 - 1
    if family == "indep":
        b = torch.rand((N, 3, H, W), generator=_gen(seed + 1)) * 2 - 1
    elif family == "near":
        b = (a + 1e-2 * torch.randn((N, 3, H, W), generator=_gen(seed + 1))).clamp(-1, 1)
    else:
        b = a.clone()
    return a, b


def _gram_case(ctx, backend, N, H, W, n0=0, nloc=-1, families=("indep", "near", "equal"), pads=(1, 5), operands=None):
    R, HW = 3 * N, H * W
    whole = nloc < 0
    L = _gram_chain(R, HW, whole)
    nl = N if whole else nloc
    worst = 0.0
    for fi, family in enumerate(families):
        a, b = operands if operands is not None else _gram_operands(N, H, W, family, 31 + N)
        scale = 5.0
        ref, lbound, gref, gbound = _gram_ref_and_bound(a, b, scale, n0, nl, L)
        for acc in (0, 1):
            pad_c = pads[(fi + acc) % len(pads)]
            loss, d, old = _call(ctx, engine.LOSS_GRAM, a, b, pad_c, scale, acc, n0, nloc, seed=N)
            case = "N%d %dx%d n0=%d nloc=%d L%d %s acc%d" % (N, H, W, n0, nloc, L, family, acc)
            if family == "equal":
                assert loss == 0.0, "b == a: the loss must be exactly 0"
                assert torch.equal(d, old if acc else torch.zeros_like(d)), "b == a: the gradient must be exactly 0"
                continue
            want = gref if not acc else old.double() + gref
            extra = 0.0 if not acc else U * want.abs()
            rl = abs(loss - ref) / max(lbound, 1e-300)
            rg = float(((d.double() - want).abs() / (gbound + extra)).max())
            worst = max(worst, rl, rg)
            figs = dict(loss_err_over_bound=rl, grad_err_over_bound=rg, grad_rel_l2=float((d.double() - want).norm() / want.norm()))
            if family == "near":
                figs["loss_rel_err"] = abs(loss - ref) / ref
            _record("gram", case, **figs)
            assert rl <= 2.0, (case, "loss %.9g ref %.9g bound %.3g" % (loss, ref, lbound))
            assert rg <= 2.0, (case, "gradient: worst |err| / bound %.3g" % rg)
    return worst


@pytest.mark.parametrize("backend", BACKENDS)
def test_gram_lds_path_vs_float64(backend):
    """R = N * 3 <= 128, whole batch: gram_partial_kernel (64-pixel chunks, HW % 64 != 0, fewer pixels than one chunk),
    gram_final_kernel (R^2 / 16 partials: 1 at N = 1, 3 at N = 2 -- no multiple of 64 -- 993 at N = 42) and gram_bwd_kernel (the grid wraps at
    74 x 74 with N >= 16).  Operands: independent, b = a + 1e-2 randn (Ga - Gb cancels), b == a (exactly 0)."""
    ctx = _ctx(backend)
    if backend == "sim":
        cases = [(1, 4, 4), (2, 7, 9), (5, 4, 4)]
    else:
        cases = [(1, 4, 4), (2, 7, 9), (1, 64, 64), (16, 74, 74), (16, 40, 52), (42, 64, 64), (42, 7, 9)]
    for N, H, W in cases:
        _gram_case(ctx, backend, N, H, W)


@pytest.mark.parametrize("backend", BACKENDS)
def test_gram_tiled_path_vs_float64(backend):
    """R > 128 (129 = the first tiled case; 132, 162: ragged 32-tiles) and the n0 / nloc form of data parallelism, which takes the
    tiled kernels at any R; 40 x 52 leaves a ragged last split."""
    ctx = _ctx(backend)
    if backend == "sim":
        cases = [(4, 4, 4, 0, 2), (4, 7, 9, 1, 3), (43, 4, 4, 0, -1)]
    else:
        cases = [(43, 7, 9, 0, -1), (43, 64, 64, 0, -1), (44, 40, 52, 0, -1), (54, 74, 74, 0, -1), (54, 4, 4, 0, -1),
                 (4, 7, 9, 0, 2), (4, 40, 52, 1, 3), (4, 64, 64, 1, 3), (48, 64, 64, 0, 2), (48, 40, 52, 1, 3), (48, 74, 74, 47, 1)]
    for N, H, W, n0, nloc in cases:
        _gram_case(ctx, backend, N, H, W, n0, nloc)


@pytest.mark.gpu
def test_gram_256_tiled_vs_lds_digits():
    """256 x 256: the tiled path (N = 44, chains of per_split = 1024) against the same bound, and for the record the rel-L2 error
    of the style gradient of both paths on the same first 42 images (N = 42 takes the LDS path, chains of 64)."""
    ctx = _ctx("gpu")
    a, b = _gram_operands(44, 256, 256, "near", 77)
    _gram_case(ctx, "gpu", 44, 256, 256, families=("near",), pads=(1,), operands=(a, b))
    _gram_case(ctx, "gpu", 42, 256, 256, families=("near",), pads=(1,), operands=(a[:42].contiguous(), b[:42].contiguous()))


@pytest.mark.parametrize("backend", BACKENDS)
def test_gram_rejects_more_than_1024_rows(backend):
    ctx = _ctx(backend)
    x = torch.zeros(342, 3, 2, 2)               # R = 1026
    with pytest.raises(ValueError):
        engine.op_loss(ctx, engine.LOSS_GRAM, x, x, 1)


# ---- bias gradient ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("C", [4, 12, 20, 32, 76, 256, 1024])
def test_bias_grad_vs_float64(backend, C):
    """colsum_partial_kernel / colsum_final_kernel: C/4 that does not divide 256 (idle thread rows, ragged LDS fold), rows = 1 at
    C = 1024, fewer pixels than thread rows (1 and 4 pixels), chunk counts that are no multiple of 16 (170 chunks at C = 256,
    2883 pixels), strided views.  fp64 partials, one rounding: |db - ref| <= 2^-23 |ref| + 2^-45 sum|dy| per channel."""
    ctx = _ctx(backend)
    for n, h, w in ((1, 1, 1), (1, 2, 2), (1, 7, 9), (1, 32, 32), (3, 31, 31)):
        dy = torch.randn((n, C, h, w), generator=_gen(41 + C)) + 3
        ref = dy.double().sum(dim=(0, 2, 3))
        tot = dy.double().abs().sum(dim=(0, 2, 3))
        for pad_c in (0, 4):
            db = engine.op_bias_grad(ctx, dy, pad_c)
            db2 = engine.op_bias_grad(ctx, dy, pad_c)
            ctx.sync()
            assert torch.equal(_bits(db), _bits(db2)), "two runs differ"
            err = (db.cpu().double() - ref).abs()
            bar = 2.0 ** -23 * ref.abs() + 2.0 ** -45 * tot
            _record("bias_grad", "C%d pad%d %dx%dx%d" % (C, pad_c, n, h, w), err_over_bar=float((err / bar).max()))
            assert bool((err <= bar).all()), (C, n, h, w, pad_c, float((err / bar).max()))
