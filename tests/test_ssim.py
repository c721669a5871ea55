"""SSIM and L1_Charbonnier_loss of modules.losses (reference modules/losses/__init__.py:14-35,128-259): the fused kernels of
csrc/ssim.hip and their host form (engine.cpp, the expressions of csrc/ssim_math.h) against float64, on the host simulator and on
the MI355X, and the module's torch branch on the CPU.

Bars (the project's existing ones against float64): rel-L2 <= 1e-5 for the loss map and for 'mean' / 'sum', <= 1e-4 for each
gradient, under a non-uniform upstream map (linspace(0.5, 1.5)) and under a scalar.  The float64 reference is (a) the module's own
torch branch in float64 and (b) the REAL reference's float64 arrays in tests/golden/ssim_reference.npz (tools/make_ssim_golden.py),
whose float32 arrays must sit inside the same bars themselves.  Inputs, shapes and seeds come from that file; every seed keeps the
float64 SSIM index 1e-4 away from the clamp points S = 0 and S = 1, where the gradient is discontinuous (asserted below)."""
import os

import numpy as np
import pytest
import torch

from tests import backends

BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]
MAP_BAR, GRAD_BAR = 1e-5, 1e-4
G_SCALAR = 0.7
_GOLD = np.load(os.path.join(backends.REPO, "tests", "golden", "ssim_reference.npz"))
CASES = [str(c) for c in _GOLD["meta/cases"]]
CHARB = [str(c) for c in _GOLD["meta/charb"]]


def _ctx(backend):
    return backends.gpu_ctx() if backend == "gpu" else backends.hostsim_ctx()


def _case(name):
    g = _GOLD
    return dict(x=torch.from_numpy(g[name + "/x"]), y=torch.from_numpy(g[name + "/y"]), window=int(g[name + "/window"]),
                max_val=float(g[name + "/max_val"]))


def _gmap(shape):
    return torch.linspace(0.5, 1.5, int(np.prod(shape)), dtype=torch.float64).reshape(shape)


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))


_ref = {}


def reference64(name):
    """The module's torch branch in float64 (computed once per case): loss map, mean, sum, the gradients under the upstream map and
    under the scalar G_SCALAR on the mean."""
    if name not in _ref:
        from swapnet_amd.modules.losses import SSIM
        c = _case(name)
        a, b = c["x"].double().requires_grad_(True), c["y"].double().requires_grad_(True)
        loss = SSIM(c["window"], "none", c["max_val"])(a, b)
        d1m, d2m = torch.autograd.grad((loss * _gmap(loss.shape)).sum(), (a, b), retain_graph=True)
        d1s, d2s = torch.autograd.grad(G_SCALAR * loss.mean(), (a, b))
        _ref[name] = dict(loss=loss.detach(), mean=loss.detach().mean(), sum=loss.detach().sum(), d1m=d1m, d2m=d2m, d1s=d1s, d2s=d2s)
    return _ref[name]


_native = {}


def native(backend, name):
    """The kernel (or its host form) on one case, computed once per backend: everything reference64 holds."""
    from swapnet_amd import engine
    key = (backend, name)
    if key not in _native:
        ctx, c = _ctx(backend), _case(name)
        n = c["x"].numel()
        total, lmap, d1m, d2m = engine.op_ssim(ctx, c["x"], c["y"], c["window"], c["max_val"], want_map=True, grad=_gmap(c["x"].shape).float(),
                                               want_grad=(True, True))
        total2, none, d1s, d2s = engine.op_ssim(ctx, c["x"], c["y"], c["window"], c["max_val"], grad=G_SCALAR / n, want_grad=(True, True))
        assert none is None and torch.equal(total.cpu(), total2.cpu())
        _native[key] = dict(loss=lmap.cpu(), sum=total.cpu()[0], mean=total.cpu()[0].double() / n, d1m=d1m.cpu(), d2m=d2m.cpu(), d1s=d1s.cpu(),
                            d2s=d2s.cpu())
    return _native[key]


def _assert_bars(got, ref, what):
    rows = [(k, _rel(got[k], ref[k]), MAP_BAR if k in ("loss", "mean", "sum") else GRAD_BAR) for k in ("loss", "mean", "sum", "d1m", "d2m", "d1s", "d2s")]
    print(what + "  " + "  ".join("%s %.2e" % (k, e) for k, e, _ in rows))
    bad = [(k, "%.2e > %.0e" % (e, bar)) for k, e, bar in rows if not e <= bar]
    assert not bad, (what, bad)


@pytest.mark.parametrize("name", CASES)
def test_inputs_stay_away_from_the_clamp_points(name):
    """Precondition of every gradient comparison below: no element of the float64 SSIM index within 1e-4 of 0 or of 1."""
    from swapnet_amd.modules.losses import SSIM
    c = _case(name)
    m = SSIM(c["window"], "none", c["max_val"])
    x, y, ch = c["x"].double(), c["y"].double(), c["x"].shape[1]
    k = m.window.double().repeat(ch, 1, 1, 1)
    mu1, mu2 = m.filter2D(x, k, ch), m.filter2D(y, k, ch)
    s1, s2, s12 = m.filter2D(x * x, k, ch) - mu1 * mu1, m.filter2D(y * y, k, ch) - mu2 * mu2, m.filter2D(x * y, k, ch) - mu1 * mu2
    S = ((2 * mu1 * mu2 + m.C1) * (2 * s12 + m.C2)) / ((mu1 * mu1 + mu2 * mu2 + m.C1) * (s1 + s2 + m.C2))
    assert float(S.abs().min()) >= 1e-4 and float((1 - S).abs().min()) >= 1e-4
    assert torch.allclose(torch.clamp(1 - S, 0, 1) / 2, reference64(name)["loss"], rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", CASES)
def test_the_reference_itself_sits_inside_the_bars(name):
    """The golden's float32 arrays against its float64 arrays, and the module's float64 torch branch against the golden's float64:
    the fixture cannot hide a failure, and the torch branch IS the reference's formula."""
    g, ref = _GOLD, reference64(name)
    assert _rel(g[name + "/loss32"], g[name + "/loss64"]) <= MAP_BAR
    assert _rel(g[name + "/d1_32"], g[name + "/d1_64"]) <= GRAD_BAR and _rel(g[name + "/d2_32"], g[name + "/d2_64"]) <= GRAD_BAR
    assert _rel(ref["loss"], g[name + "/loss64"]) <= 1e-12 and _rel(ref["mean"], g[name + "/mean64"]) <= 1e-12 and _rel(ref["sum"], g[name + "/sum64"]) <= 1e-12
    assert _rel(ref["d1m"], g[name + "/d1_64"]) <= 1e-10 and _rel(ref["d2m"], g[name + "/d2_64"]) <= 1e-10


@pytest.mark.parametrize("name", CASES)
def test_torch_branch_in_float32(name):
    """CPU float32 tensors take the module's torch branch: inside the bars too."""
    from swapnet_amd.modules.losses import ssim
    c, ref = _case(name), reference64(name)
    a, b = c["x"].clone().requires_grad_(True), c["y"].clone().requires_grad_(True)
    loss = ssim(a, b, c["window"], "none", c["max_val"])
    d1m, d2m = torch.autograd.grad((loss * _gmap(loss.shape).float()).sum(), (a, b), retain_graph=True)
    d1s, d2s = torch.autograd.grad(G_SCALAR * loss.mean(), (a, b))
    got = dict(loss=loss.detach(), mean=ssim(a, b, c["window"], "mean", c["max_val"]).detach(), sum=ssim(a, b, c["window"], "sum", c["max_val"]).detach(),
               d1m=d1m, d2m=d2m, d1s=d1s, d2s=d2s)
    _assert_bars(got, ref, "torch fp32 %s" % name)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_native_against_float64(backend, name):
    _assert_bars(native(backend, name), reference64(name), "%s %s" % (backend, name))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_native_against_the_golden(backend, name):
    g, got = _GOLD, native(backend, name)
    ref = dict(loss=g[name + "/loss64"], mean=g[name + "/mean64"], sum=g[name + "/sum64"], d1m=g[name + "/d1_64"], d2m=g[name + "/d2_64"])
    rows = [(k, _rel(got[k], ref[k]), MAP_BAR if k in ("loss", "mean", "sum") else GRAD_BAR) for k in ref]
    print("%s %s vs golden  " % (backend, name) + "  ".join("%s %.2e" % (k, e) for k, e, _ in rows))
    assert all(e <= bar for _, e, bar in rows), rows


@pytest.mark.parametrize("backend", BACKENDS)
def test_two_calls_are_bitwise_equal(backend):
    from swapnet_amd import engine
    ctx, c = _ctx(backend), _case("ragged")
    runs = [engine.op_ssim(ctx, c["x"], c["y"], c["window"], c["max_val"], want_map=True, grad=_gmap(c["x"].shape).float(), want_grad=(True, True))
            for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a.cpu(), b.cpu())
    for k, t in zip(("sum", "loss", "d1m", "d2m"), runs[0]):
        assert torch.equal(t.cpu().reshape(-1), torch.as_tensor(native(backend, "ragged")[k]).reshape(-1))


@pytest.mark.parametrize("backend", BACKENDS)
def test_saturated_and_identical_images(backend):
    """y = -x pins the saturated branch: loss exactly 0.5, gradient exactly 0.  With y = -x, S = (C1 - 2 mu^2)(C2 - 2 s) / ((C1 + 2 mu^2)
    (C2 + 2 s)) is negative only where exactly one factor is: the image is a +-0.2 checkerboard, whose local mean all but vanishes
    under the Gaussian (mu^2 < C1 / 2 even in the zero-padded corners) while its local variance does not (s > C2 / 2) -- asserted in
    float64 first.  y = x: loss <= 1e-6 (value only)."""
    from swapnet_amd import engine
    from swapnet_amd.modules.losses import SSIM
    ctx, c = _ctx(backend), _case("ragged")
    ii = torch.arange(37).view(1, 1, 37, 1) + torch.arange(45).view(1, 1, 1, 45) + torch.arange(3).view(1, 3, 1, 1)
    x = (0.2 * (1 - 2 * (ii % 2)).float()).expand(2, 3, 37, 45).contiguous()
    assert torch.equal(SSIM(11)(x.double(), -x.double()), torch.full(x.shape, 0.5, dtype=torch.float64))
    total, lmap, d1, d2 = engine.op_ssim(ctx, x, -x, 11, 1.0, want_map=True, grad=_gmap(x.shape).float(), want_grad=(True, True))
    assert torch.equal(lmap.cpu(), torch.full_like(x, 0.5)) and float(total.cpu()[0]) == 0.5 * x.numel()
    assert not d1.cpu().any() and not d2.cpu().any()
    x = c["x"]
    total, lmap, _, _ = engine.op_ssim(ctx, x, x.clone(), 11, 1.0, want_map=True)
    assert float(lmap.cpu().max()) <= 1e-6 and float(lmap.cpu().min()) >= 0.0 and float(total.cpu()[0]) / x.numel() <= 1e-6


@pytest.mark.parametrize("backend", BACKENDS)
def test_one_gradient_alone_and_unaligned_views(backend):
    """d1 without d2 (and the reverse) equals the pair; non-contiguous inputs are made contiguous."""
    from swapnet_amd import engine
    ctx, c, ref = _ctx(backend), _case("flat_wide"), native(backend, "flat_wide")
    g = _gmap(c["x"].shape).float()
    _, _, d1, none = engine.op_ssim(ctx, c["x"], c["y"], c["window"], c["max_val"], grad=g, want_grad=(True, False))
    assert none is None and torch.equal(d1.cpu(), ref["d1m"])
    xt = c["x"].transpose(2, 3).contiguous().transpose(2, 3)
    assert not xt.is_contiguous()
    _, _, none, d2 = engine.op_ssim(ctx, xt, c["y"], c["window"], c["max_val"], grad=g, want_grad=(False, True))
    assert none is None and torch.equal(d2.cpu(), ref["d2m"])


def test_errors_are_the_references():
    from swapnet_amd.modules.losses import SSIM, get_gaussian_kernel1d, get_gaussian_kernel2d
    x = torch.zeros(1, 2, 8, 8)
    with pytest.raises(TypeError, match="kernel_size must be an odd positive integer. Got 4"):
        SSIM(4)
    with pytest.raises(TypeError, match="odd positive integer"):
        SSIM(5.0)
    with pytest.raises(TypeError, match="odd positive integer"):
        get_gaussian_kernel1d(0, 1.5)
    with pytest.raises(TypeError, match="tuple of length two"):
        get_gaussian_kernel2d(5, (1.5, 1.5))
    with pytest.raises(TypeError, match="Input img1 type is not a torch.Tensor"):
        SSIM(5)(x.numpy(), x)
    with pytest.raises(TypeError, match="Input img2 type is not a torch.Tensor"):
        SSIM(5)(x, [1.0])
    with pytest.raises(ValueError, match="Invalid img1 shape, we expect BxCxHxW"):
        SSIM(5)(x[0], x)
    with pytest.raises(ValueError, match="Invalid img2 shape, we expect BxCxHxW"):
        SSIM(5)(x, x[0])
    with pytest.raises(ValueError, match="shapes must be the same"):
        SSIM(5)(x, x[:, :1])
    with pytest.raises(ValueError, match="same dtype"):
        SSIM(5)(x, x.double())


def test_module_surface():
    """The reference's constructor and attributes, and its exports."""
    from swapnet_amd.modules import losses
    for n in ("PerceptualLoss", "SSIM", "ssim", "L1_Charbonnier_loss", "gaussian", "get_gaussian_kernel1d", "get_gaussian_kernel2d"):
        assert hasattr(losses, n), n
    m = losses.SSIM(5, reduction="none", max_val=2.0)
    assert isinstance(m, torch.nn.Module) and m.window.shape == (5, 5) and m.window.dtype == torch.float32 and m.padding == 2
    assert m.C1 == (0.01 * 2.0) ** 2 and m.C2 == (0.03 * 2.0) ** 2 and (m.window_size, m.reduction, m.max_val) == (5, "none", 2.0)
    assert torch.allclose(losses.get_gaussian_kernel1d(5, 1.5), torch.tensor([0.1201, 0.2339, 0.2921, 0.2339, 0.1201]), atol=5e-5)
    assert abs(float(m.window.sum()) - 1.0) < 1e-6 and losses.L1_Charbonnier_loss().eps == 1e-6
    assert losses.ssim(torch.rand(1, 4, 5, 5), torch.rand(1, 4, 5, 5), 5).shape == (1, 4, 5, 5)


@pytest.mark.parametrize("backend", BACKENDS)
def test_window_sizes_and_the_cap(backend):
    """Every odd window from 1 to the cap has a kernel (value against float64 on a two-tile image); the next odd size and an even
    one are refused by name."""
    from swapnet_amd import engine
    from swapnet_amd.modules.losses import SSIM
    ctx = _ctx(backend)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 2, 12, 35, generator=g) * 2 - 1
    y = x + 0.25 * torch.randn(x.shape, generator=g)
    assert engine.SSIM_MAX_WINDOW == 15
    for ws in range(1, engine.SSIM_MAX_WINDOW + 1, 2):
        total, lmap, _, _ = engine.op_ssim(ctx, x, y, ws, 1.0, want_map=True)
        ref = SSIM(ws)(x.double(), y.double())
        assert _rel(lmap, ref) <= MAP_BAR and _rel(total.cpu()[0], ref.sum()) <= MAP_BAR, ws
    with pytest.raises(NotImplementedError, match="larger than 15"):
        engine.op_ssim(ctx, x, y, 17)
    with pytest.raises(ValueError, match="odd positive integer. Got 4"):
        engine.op_ssim(ctx, x, y, 4)
    with pytest.raises(ValueError, match="one shape"):
        engine.op_ssim(ctx, x, y[:, :1], 5)


# ---- Charbonnier ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CHARB)
def test_charbonnier(backend, name):
    from swapnet_amd import engine
    ctx, g = _ctx(backend), _GOLD
    x, y = torch.from_numpy(g["charb/%s/x" % name]), torch.from_numpy(g["charb/%s/y" % name])
    total, dx, dy = engine.op_charbonnier(ctx, x, y, 1e-6, grad=G_SCALAR, want_grad=(True, True))
    e = (_rel(total.cpu()[0], g["charb/%s/value64" % name]), _rel(dx, G_SCALAR * g["charb/%s/dx64" % name]), _rel(dy, G_SCALAR * g["charb/%s/dy64" % name]))
    print("%s charbonnier %s  value %.2e  dx %.2e  dy %.2e" % (backend, name, *e))
    assert e[0] <= MAP_BAR and e[1] <= GRAD_BAR and e[2] <= GRAD_BAR
    assert _rel(g["charb/%s/value32" % name], g["charb/%s/value64" % name]) <= MAP_BAR
    total2, none, dy2 = engine.op_charbonnier(ctx, x, y, 1e-6, grad=G_SCALAR, want_grad=(False, True))
    assert none is None and torch.equal(total.cpu(), total2.cpu()) and torch.equal(dy.cpu(), dy2.cpu())


@pytest.mark.parametrize("backend", BACKENDS)
def test_charbonnier_at_zero_difference(backend):
    """d = 0: sqrt(eps) per element, gradient exactly 0."""
    from swapnet_amd import engine
    ctx = _ctx(backend)
    x = torch.linspace(-1, 1, 2 * 3 * 7 * 9).reshape(2, 3, 7, 9)
    total, dx, dy = engine.op_charbonnier(ctx, x, x.clone(), 1e-6, grad=1.0, want_grad=(True, True))
    assert _rel(total.cpu()[0], x.numel() * 1e-3) <= MAP_BAR and not dx.cpu().any() and not dy.cpu().any()
    with pytest.raises(ValueError, match="equal numel"):
        engine.op_charbonnier(ctx, x, x[:1])


def test_charbonnier_module_on_the_cpu():
    from swapnet_amd.modules.losses import L1_Charbonnier_loss
    g = _GOLD
    x, y = torch.from_numpy(g["charb/small/x"]).double().requires_grad_(True), torch.from_numpy(g["charb/small/y"]).double().requires_grad_(True)
    v = L1_Charbonnier_loss()(x, y)
    v.backward()
    assert _rel(v.detach(), g["charb/small/value64"]) <= 1e-12 and _rel(x.grad, g["charb/small/dx64"]) <= 1e-12 and _rel(y.grad, g["charb/small/dy64"]) <= 1e-12


# ---- the autograd.Function path (CUDA float32 tensors), GPU only ----------------------------------------------------------------------
@pytest.mark.gpu
def test_module_on_the_device_end_to_end():
    from swapnet_amd.modules.losses import SSIM, L1_Charbonnier_loss
    backends.gpu_ctx()
    c, ref, got = _case("ragged"), reference64("ragged"), native("gpu", "ragged")
    a, b = c["x"].cuda().requires_grad_(True), c["y"].cuda().requires_grad_(True)
    loss = SSIM(11, "mean")(a, b)
    (G_SCALAR * loss).backward()
    assert loss.is_cuda and loss.dim() == 0 and a.grad is not None and b.grad is not None
    assert _rel(loss.detach(), ref["mean"]) <= MAP_BAR and _rel(a.grad, ref["d1s"]) <= GRAD_BAR and _rel(b.grad, ref["d2s"]) <= GRAD_BAR
    # reduction 'none' under a map; a non-contiguous input; only one side asks for a gradient
    a2 = c["x"].cuda().transpose(2, 3).contiguous().transpose(2, 3).requires_grad_(True)
    lmap = SSIM(11)(a2, c["y"].cuda())
    (lmap * _gmap(lmap.shape).float().cuda()).sum().backward()
    assert torch.equal(lmap.detach().cpu(), got["loss"]) and torch.equal(a2.grad.cpu(), got["d1m"])
    s = SSIM(11, "sum")(c["x"].cuda(), c["y"].cuda())
    assert torch.equal(s.cpu(), got["sum"])
    # float64 on the device takes the torch branch
    l64 = SSIM(11, "mean")(c["x"].cuda().double(), c["y"].cuda().double())
    assert l64.dtype == torch.float64 and _rel(l64, ref["mean"]) <= 1e-10
    g = _GOLD
    x, y = torch.from_numpy(g["charb/small/x"]).cuda().requires_grad_(True), torch.from_numpy(g["charb/small/y"]).cuda().requires_grad_(True)
    v = L1_Charbonnier_loss()(x, y)
    (G_SCALAR * v).backward()
    assert _rel(v.detach(), g["charb/small/value64"]) <= MAP_BAR and _rel(x.grad, G_SCALAR * g["charb/small/dx64"]) <= GRAD_BAR
    assert _rel(y.grad, G_SCALAR * g["charb/small/dy64"]) <= GRAD_BAR
