"""Operator-level float64 parity of norm_act.hip's InstanceNorm + activation + dropout + residual: forward, backward, second order.

Every launch goes through swn_op_norm_act (norm_act_fwd + norm_act_bwd called directly, no Net) or swn_op_norm_act_bwd2.  Each
operand lives in an NHWC buffer of lead_c + C + pad_c channels filled with the byte 0x7f, the kernel gets buffer.slice(lead_c, C).
Each body runs on the CI host simulator and on the MI355X.

Reference: plain float64 formulas on the fp32 operands, eps = float32(1e-5), LeakyReLU slope = float32(0.2), the mask the device
used (the dropout_mask export), the activation branch taken from the float64 xh.

Inputs stay off the kink (_off_the_kink): with a = |mean| rstd + |xh|, every element with |xh| < 16 U a is moved away from zero by
64 U a / rstd until none is left, so the fp32 xh of the kernels (off by at most ~2 U a) selects the branch the float64 xh selects
and no element is excluded from a comparison.  Exactly constant planes (0.75) are the exception: xh is exactly 0 on both sides and
the branch is the `v > 0` false one.

Bars (U = 2^-24; <.> = the plane mean; one term per rounding of the kernels: fp64 sums, mean / rstd rounded to fp32, the fp32
(x - mean) * rstd, the fp64 combination rounded once):
  forward   |y - y64|   <= U (a |act'| mask + 3 |y64|)
  backward  |dx - dx64| <= U rstd (2|g| + 2<|g|> + |xh| (2<|g||xh|> + <|g| a>) + a |m2|) + 3 U |dx64|,  g = dy act' mask, m2 = <g xh>
test_bars_hold_for_an_emulation_of_the_kernels checks these against a numpy emulation of that arithmetic alone (no library call).
With a residual (activation none, as Net::norm_act requires) the residual carries the sign of the normalised term: the forward bar
is relative to y64, and a residual that cancels the term would leave the term's own roundings without cover.
norm = 0: forward and backward are single fp32 operations and must equal numpy's fp32 result bit for bit.
tanh: |y - y64| <= k ulp(y64) + U a |act'| with k = 4 x the worst figure of torch's fp32 CPU tanh on the same inputs (at least 1 ulp);
the backward bar adds what that uncertainty of y and of xh does to g = dy (1 - y^2), pushed through the backward formula.
Second order: 4 x the figure of a torch fp32 CPU double backward on the same inputs, at least 2^-23 (tests/test_loss_ops.py).

Asserted in every call (_launch): two runs are bit-equal; the non-logical channels of the y and dx buffers keep the sentinel;
max(amax slot) equals the amax of the returned tensor bit for bit (a sentinel in a neighbouring channel would show as 3.39e38);
the statistics are within U relative of the float64 mean and rstd; y == 0 exactly where the mask is 0; the seed_base form (s, salt)
gives the bits of the host seed s * 0x9E3779B1 + salt; where column sums were emitted |colsum - sum64(dx returned)| <= 2^-45 sum|dx|
and db is within one fp32 rounding of their sum over the batch.
"""
import numpy as np
import pytest
import torch

from swapnet_amd import engine
from tests import backends

BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]
U = 2.0 ** -24
SENT = engine.PAD_SENTINEL
EPS = float(np.float32(1e-5))
SLOPE = float(np.float32(0.2))
NONE, LRELU, RELU, TANH = 0, 1, 2, 3
ACT_NAMES = ("none", "lrelu", "relu", "tanh")
SALT = 1                                      # the salt of the mask export (swn_op_norm_act_dropout: first op of its net)


def _ctx(kind):
    return backends.gpu_ctx() if kind == "gpu" else backends.hostsim_ctx()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _raw(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def _np(t):
    return t.detach().cpu().numpy()


def _record(kernel, case, **figs):
    print("NORMOPS %-14s %-52s %s" % (kernel, case, "  ".join("%s %.3g" % kv for kv in figs.items())))


def _pm(v):
    return v.mean(axis=(2, 3), keepdims=True)


def _stats64(x64):
    mean = _pm(x64)
    return mean, 1.0 / np.sqrt(_pm((x64 - mean) ** 2) + EPS)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _off_the_kink(x, const):
    """See the module docstring.  x (N,C,H,W) fp32, const (N,C) marks the exactly constant planes.  Returns (x, rounds)."""
    free = ~const[:, :, None, None]
    for rounds in range(9):
        x64 = x.astype(np.float64)
        mean, rstd = _stats64(x64)
        xh = (x64 - mean) * rstd
        a = np.abs(mean) * rstd + np.abs(xh)
        near = (np.abs(xh) < 16 * U * a) & free
        if not near.any():
            assert bool((xh[np.broadcast_to(~free, xh.shape)] == 0).all()), "a constant plane is not exactly constant"
            return x, rounds
        step = 64 * U * a / rstd
        x = np.where(near, x64 + np.where(xh >= 0, step, -step), x64).astype(np.float32)
    raise AssertionError("elements within 16 U a of the kink are left after 8 rounds")


def _make_x(N, C, H, W, seed, families=True):
    """randn * 3 + 1.5; with `families`, by channel mod 8: 1 = mean 100 / std 0.01, 2 = constant 0.75, 3 and 5 = scale e^U(-6,3)
    with an offset of a few scales.  families = "mild": without the mean-100 planes."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, C, H, W)) * 3 + 1.5).astype(np.float32)
    const = np.zeros((N, C), dtype=bool)
    if families:
        for c in range(C):
            k = c % 8
            if k == 1 and families != "mild":
                x[:, c] = 100 + 0.01 * rng.standard_normal((N, H, W))
            elif k == 2:
                x[:, c] = 0.75
                const[:, c] = True
            elif k in (3, 5):
                s = np.exp(rng.uniform(-6, 3))
                x[:, c] = s * (rng.standard_normal((N, H, W)) + 2 * rng.standard_normal())
    return _off_the_kink(x, const)[0]


_masks = {}


def _mask(ctx, backend, shape, s):
    """The keep/scale factors (0 or 2) of a p = 0.5 site of this shape under step seed s: the library's dropout_mask export."""
    key = (backend, tuple(shape), s)
    if key not in _masks:
        _, m, _ = engine.op_norm_act_dropout(ctx, torch.zeros(shape), None, norm=False, act=NONE, p=0.5, seed=s)
        ctx.sync()
        m = _np(m).astype(np.float64)
        assert bool(((m == 0) | (m == 2)).all())
        assert m.size < 256 or 0.3 < float((m == 0).mean()) < 0.7
        _masks[key] = m
    return _masks[key]


# ---- the float64 reference and its bars -----------------------------------------------------------------------------------------------
def _act64(xh, act):
    if act == LRELU:
        return np.where(xh > 0, xh, SLOPE * xh), np.where(xh > 0, 1.0, SLOPE)
    if act == RELU:
        return np.where(xh > 0, xh, 0.0), np.where(xh > 0, 1.0, 0.0)
    if act == TANH:
        t = np.tanh(xh)
        return t, 1.0 - t * t
    return xh, np.ones_like(xh)


def _reference(x, dy, mask, res, act):
    """norm = 1.  Returns a dict of float64 arrays: mean, rstd, xh, a, ad, y, ybar and, with dy, g, dx, dxbar."""
    x64 = x.astype(np.float64)
    mean, rstd = _stats64(x64)
    xh = (x64 - mean) * rstd
    a = np.abs(mean) * rstd + np.abs(xh)
    f, ad = _act64(xh, act)
    m = 1.0 if mask is None else mask
    y = f * m + (0.0 if res is None else res.astype(np.float64))
    r = dict(mean=mean, rstd=rstd, xh=xh, a=a, ad=ad, m=m, y=y, ybar=U * (a * np.abs(ad) * m + 3 * np.abs(y)))
    if dy is not None:
        g = dy.astype(np.float64) * ad * m
        m2 = _pm(g * xh)
        dx = rstd * (g - _pm(g) - xh * m2)
        ag = np.abs(g)
        r.update(g=g, dx=dx, dxbar=U * rstd * (2 * ag + 2 * _pm(ag) + np.abs(xh) * (2 * _pm(ag * np.abs(xh)) + _pm(ag * a)) + a * np.abs(m2))
                 + 3 * U * np.abs(dx))
    return r


def _share(err, bar):
    """max err / bar; an element whose bar is 0 must be exact."""
    assert bool((err[bar == 0] == 0).all()), "an element whose bar is 0 (exactly representable result) is off"
    nz = bar > 0
    return float((err[nz] / bar[nz]).max()) if nz.any() else 0.0


# ---- one launch with everything that holds in every call ----------------------------------------------------------------------------
VIEW_BITS = (0b0000, 0b1111, 0b0101, 0b1010, 0b0011, 0b1100, 0b0110, 0b1001)         # (y lead, y pad, dx lead, dx pad) x 4 channels


def _views(i):
    b = VIEW_BITS[i % len(VIEW_BITS)]
    j = (i * 5 + 3) % 16                                                               # x, dy and the residual take other combinations
    return {"y": (4 * (b & 1), 4 * (b >> 1 & 1)), "dx": (4 * (b >> 2 & 1), 4 * (b >> 3 & 1)),
            "x": (4 * (j & 1), 4 * (j >> 1 & 1)), "dy": (4 * (j >> 2 & 1), 4 * (j >> 3 & 1)), "residual": (4 * (j >> 1 & 1), 4 * (j & 1))}


def _check_buffer(buf, out, lead, what):
    c = out.shape[1]
    b = _bits(buf)
    assert torch.equal(b[:, lead:lead + c], _bits(out)), what + ": the buffer's logical channels are not the returned tensor"
    assert bool((b[:, :lead] == SENT).all()) and bool((b[:, lead + c:] == SENT).all()), what + ": a non-logical channel was written"


def _check_slot(slot, out, what):
    assert torch.equal(_bits(slot.max()), _bits(out.abs().max())), \
        (what, "max(slot) %.9g != amax %.9g" % (float(slot.max()), float(out.abs().max())))


def _launch(ctx, x, dy, res, norm, act, drop, s, views, **kw):
    """The call twice (+ once in the seed_base form when it drops), with the assertions of the module docstring that need no
    reference.  Returns the first result."""
    host_seed = (s * 0x9E3779B1 + SALT) % 2 ** 64
    tx, tdy, tres = torch.from_numpy(x), None if dy is None else torch.from_numpy(dy), None if res is None else torch.from_numpy(res)
    args = dict(residual=tres, norm=norm, act=act, drop_p=0.5 if drop else 0.0, views=views, **kw)
    runs = [engine.op_norm_act(ctx, tx, tdy, seed=host_seed, **args) for _ in range(2)]
    if drop:
        runs.append(engine.op_norm_act(ctx, tx, tdy, seed=s, seed_on_device=True, salt=SALT, **args))
    ctx.sync()
    r = runs[0]
    for o in runs[1:]:
        for k in ("y", "stats", "dx", "colsum", "db", "y_buf", "dx_buf"):
            assert (r[k] is None) == (o[k] is None) and (r[k] is None or torch.equal(_raw(r[k]), _raw(o[k]))), \
                "%s differs between two runs / between the host seed and the seed_base form" % k
    _check_buffer(r["y_buf"], r["y"], views["y"][0], "y")
    _check_slot(r["y_slot"], r["y"], "y")
    if dy is not None:
        _check_buffer(r["dx_buf"], r["dx"], views["dx"][0], "dx")
        _check_slot(r["dx_slot"], r["dx"], "dx")
    return r


def _check_colsum(ctx, r, case):
    """Where the launch emitted column sums; returns whether it did."""
    if not r["colsum_emitted"]:
        return False
    dx = _np(r["dx"]).astype(np.float64)
    cs = _np(r["colsum"])
    ref, tot = dx.sum(axis=(2, 3)), np.abs(dx).sum(axis=(2, 3))
    fig = _share(np.abs(cs - ref), 2.0 ** -45 * tot)
    dbref = cs.sum(axis=0)
    dfig = _share(np.abs(_np(r["db"]).astype(np.float64) - dbref), U * np.abs(dbref))
    _record("colsum", case, err_over_bar=fig, db_over_one_rounding=dfig)
    assert fig <= 1.0 and dfig <= 1.0, (case, fig, dfig)
    return True


def _check_case(ctx, backend, name, x, dy, act, drop, residual, vi, s=11, **kw):
    """norm = 1: one configuration of one case against the float64 reference."""
    mask = _mask(ctx, backend, x.shape, s) if drop else None
    res = None
    if residual:
        mean, rstd = _stats64(x.astype(np.float64))
        sign = np.where((x.astype(np.float64) - mean) >= 0, 1.0, -1.0)
        res = (sign * np.abs(np.random.default_rng(5).standard_normal(x.shape))).astype(np.float32)
    views = _views(vi)
    r = _launch(ctx, x, dy, res, True, act, drop, s, views, **kw)
    ref = _reference(x, dy, mask, res, act)
    case = "%s %s drop%d res%d y%s dx%s" % (name, ACT_NAMES[act], drop, residual, "%d+%d" % views["y"], "%d+%d" % views["dx"])
    st = _np(r["stats"]).astype(np.float64)
    smean = _share(np.abs(st[..., 0] - ref["mean"][:, :, 0, 0]), U * np.abs(ref["mean"][:, :, 0, 0]))
    srstd = _share(np.abs(st[..., 1] - ref["rstd"][:, :, 0, 0]), U * ref["rstd"][:, :, 0, 0])
    y = _np(r["y"]).astype(np.float64)
    fy = _share(np.abs(y - ref["y"]), ref["ybar"])
    figs = dict(mean_over_U=smean, rstd_over_U=srstd, fwd_share=fy)
    if mask is not None and res is None:
        assert bool((y[mask == 0] == 0).all()), "y is not exactly 0 where the mask is 0"
    fdx = 0.0
    if dy is not None:
        fdx = _share(np.abs(_np(r["dx"]).astype(np.float64) - ref["dx"]), ref["dxbar"])
        figs["bwd_share"] = fdx
    _record("norm_act", case, **figs)
    assert smean <= 1.0 and srstd <= 1.0, (case, "statistics off by more than U relative", smean, srstd)
    assert fy <= 1.0, (case, "forward: worst |err| / bar %.3g" % fy)
    assert fdx <= 1.0, (case, "backward: worst |err| / bar %.3g" % fdx)
    if dy is not None:
        emitted = _check_colsum(ctx, r, case)
        assert emitted == (backend == "gpu" and x.shape[2] * x.shape[3] <= 1024 and x.shape[1] % 32 == 0)
    return r


CONFIGS = [(NONE, 0, 0), (LRELU, 0, 0), (RELU, 0, 0), (NONE, 1, 0), (LRELU, 1, 0), (RELU, 1, 0), (NONE, 0, 1), (NONE, 1, 1)]    # (act, dropout, residual)

# the smallest shapes that reach each code path of norm_act_fwd / norm_act_bwd: (id, N, C, H, W)
CASES = [
    ("fused<32,2> HW2", 1, 32, 1, 2), ("fused<32,2> HW33", 2, 32, 3, 11), ("fused<32,2> HW64", 1, 32, 8, 8),
    ("fused<32,8> HW65", 1, 32, 5, 13), ("fused<32,8> HW256", 2, 32, 16, 16),
    ("fused<32,16> HW257", 1, 32, 1, 257), ("fused<32,16> HW512", 1, 32, 16, 32),
    ("fused<16,16> HW513", 1, 32, 19, 27), ("fused<16,16> HW1024", 1, 32, 32, 32), ("fused<16,16> C256 HW529", 1, 256, 23, 23),
    ("chunked C8 HW4", 2, 8, 2, 2), ("chunked C36 HW16", 1, 36, 4, 4), ("chunked C12 HW2500", 1, 12, 50, 50),
    ("chunked C32 HW1025", 1, 32, 25, 41), ("chunked C1024 HW1056", 1, 1024, 33, 32),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_norm_act_vs_float64(backend, case):
    """Every path of the table with activation none / LeakyReLU / ReLU x dropout 0 / 0.5, a residual, and lead_c / pad_c in {0, 4}
    chosen independently for y and dx (VIEW_BITS: every value of each of the four in every case)."""
    ctx = _ctx(backend)
    name, N, C, H, W = case
    x = _make_x(N, C, H, W, seed=100 + C + H * W)
    dy = np.random.default_rng(7 + H * W).standard_normal(x.shape).astype(np.float32)
    for i, (act, drop, residual) in enumerate(CONFIGS):
        _check_case(ctx, backend, name, x, dy, act, drop, residual, vi=i + len(name))


@pytest.mark.parametrize("backend", BACKENDS)
def test_norm_act_statistics_from_partial_sums(backend):
    """partial_in: in_finalize_kernel<0> + apply without a statistics pass, C 32, HW 2048, 16 chunks.  float64 partials of random
    planes: the bars of the statistics pass.  On a grid of multiples of 2^-10 every fp64 sum is exact in any order, so the partials
    ARE the statistics pass's own sums: the statistics then equal that pass's bit for bit.
    No mean-100 / std-0.01 plane here: the interface carries (sum x, sum x^2), and rounding those to fp64 alone costs (mean / std)^2 2^-53 =
    1e-8 of the variance per rounding -- with the roundings of 16 partials and their sum that is the whole U the statistics are held to."""
    ctx = _ctx(backend)
    N, C, H, W, chunks = 1, 32, 32, 64, 16
    x = _make_x(N, C, H, W, seed=9, families="mild")
    dy = np.random.default_rng(8).standard_normal(x.shape).astype(np.float32)

    def partials(v):
        p = v.astype(np.float64).reshape(N, C, chunks, H * W // chunks)
        return torch.from_numpy(np.stack([p.sum(axis=3), (p * p).sum(axis=3)], axis=-1).transpose(0, 2, 1, 3).copy())      # (N, chunks, C, 2)
    for i, (act, drop, residual) in enumerate(CONFIGS):
        _check_case(ctx, backend, "partial_in HW2048", x, dy, act, drop, residual, vi=i, partial_in=partials(x))
    grid = (np.random.default_rng(3).integers(-4096, 4097, size=x.shape) / 1024.0).astype(np.float32)
    tg = torch.from_numpy(grid)
    own = engine.op_norm_act(ctx, tg, act=LRELU)
    fed = engine.op_norm_act(ctx, tg, act=LRELU, partial_in=partials(grid))
    ctx.sync()
    assert torch.equal(_bits(own["stats"]), _bits(fed["stats"])), "statistics from the pass's own sums differ from the pass"
    assert torch.equal(_bits(own["y"]), _bits(fed["y"]))
    with pytest.raises(ValueError, match="partial_chunks"):
        engine.op_norm_act(ctx, tg, act=LRELU, partial_in=partials(grid)[:, :15].contiguous())       # 2048 % 15 != 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_norm_act_without_norm_is_bit_exact(backend):
    """norm = 0 (the apply kernels alone): y = act(x) * mask + residual and dx = dy * act'(x) * mask are single fp32 operations --
    equal to numpy's fp32 result bit for bit, at a fused-size and a chunked-size shape."""
    ctx = _ctx(backend)
    for name, N, C, H, W in (("C32 HW33", 2, 32, 3, 11), ("C12 HW2500", 1, 12, 50, 50)):
        x = _make_x(N, C, H, W, seed=21, families=False)
        dy = np.random.default_rng(22).standard_normal(x.shape).astype(np.float32)
        res0 = np.random.default_rng(23).standard_normal(x.shape).astype(np.float32)
        for i, (act, drop, residual) in enumerate(CONFIGS):
            mask = _mask(ctx, backend, x.shape, 11).astype(np.float32) if drop else np.float32(1)
            res = res0 if residual else None
            r = _launch(ctx, x, dy, res, False, act, drop, 11, _views(i))
            slope = np.float32(0.2)
            f = x if act == NONE else np.where(x > 0, x, slope * x if act == LRELU else np.float32(0))
            ad = np.float32(1) if act == NONE else np.where(x > 0, np.float32(1), slope if act == LRELU else np.float32(0))
            y = f * mask if drop else f
            if residual:
                y = y + res
            g = dy * ad
            g = (g * mask if drop else g).astype(np.float32)
            case = "%s %s drop%d res%d" % (name, ACT_NAMES[act], drop, residual)
            _record("norm_act", "norm0 " + case, y_bits_equal=float(np.array_equal(_np(r["y"]).view(np.int32), y.astype(np.float32).view(np.int32))))
            assert np.array_equal(_np(r["y"]).view(np.int32), y.astype(np.float32).view(np.int32)), case
            assert np.array_equal(_np(r["dx"]).view(np.int32), g.view(np.int32)), case
            assert not r["colsum_emitted"]


def _tanh_bar(v):
    """k of the module docstring for the tanh arguments v (float64 array of fp32 values), and the measured torch figure."""
    y64 = np.tanh(v)
    t32 = torch.tanh(torch.from_numpy(v.astype(np.float32))).numpy().astype(np.float64)
    ulp = np.spacing(np.abs(y64).astype(np.float32)).astype(np.float64)
    fig = float((np.abs(t32 - y64) / ulp).max())
    return 4.0 * max(fig, 1.0), fig


def _tanh_sweep(shape, seed):
    """Magnitudes 2^-30 .. 2^5, both signs, log-uniform."""
    rng = np.random.default_rng(seed)
    return (np.exp2(rng.uniform(-30, 5, size=shape)) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


@pytest.mark.parametrize("backend", BACKENDS)
def test_norm_act_tanh(backend):
    """tanh through norm_act.  norm = 0 on the magnitude sweep: the forward to k ulp, and the backward differentiates through the
    INPUT: dx = dy (1 - tanh(x)^2) with x the raw pre-activation NormActBwdArgs::x holds -- handing it the output y instead would give
    dy (1 - tanh(tanh(x))^2), off by O(1) for |x| ~ 1.  norm = 1 at a fused and a chunked shape: the a term is added (module
    docstring)."""
    ctx = _ctx(backend)
    x = _tanh_sweep((2, 32, 3, 11), 31)
    dy = np.random.default_rng(32).standard_normal(x.shape).astype(np.float32)
    r = _launch(ctx, x, dy, None, False, TANH, 0, 11, _views(3))
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    k, tfig = _tanh_bar(x64)
    t = np.tanh(x64)
    ulp = np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)
    fy = float((np.abs(_np(r["y"]).astype(np.float64) - t) / ulp).max())
    # 1 - th^2 in fp32 from a th that is k ulp off: 2 |th| k ulp(th) + one rounding each of th^2, of the difference and of the product
    dx64 = dy64 * (1 - t * t)
    bar = np.abs(dy64) * (2 * np.abs(t) * k * ulp + U * t * t + U * np.abs(1 - t * t)) + U * np.abs(dx64)
    fdx = _share(np.abs(_np(r["dx"]).astype(np.float64) - dx64), bar)
    wrong = float(np.abs(dy64 * (1 - np.tanh(t) ** 2) - dx64).max())
    _record("norm_act", "norm0 tanh sweep", fwd_ulps=fy, torch32_ulps=tfig, bar_ulps=k, bwd_share=fdx, through_y_would_be_off_by=wrong)
    assert fy <= k, ("tanh forward %.3g ulp > %.3g" % (fy, k))
    assert fdx <= 1.0, ("tanh backward through the input: worst |err| / bar %.3g" % fdx)
    assert wrong > 0.1                                        # the two readings of ops.h differ where the test looks
    for name, N, C, H, W in (("fused C32 HW65", 1, 32, 5, 13), ("chunked C12 HW2500", 1, 12, 50, 50)):
        x = _make_x(N, C, H, W, seed=33)
        dy = np.random.default_rng(34).standard_normal(x.shape).astype(np.float32)
        r = _launch(ctx, x, dy, None, True, TANH, 0, 11, _views(5))
        ref = _reference(x, dy, None, None, TANH)
        k, tfig = _tanh_bar(ref["xh"].astype(np.float32).astype(np.float64))
        ulp = np.spacing(np.abs(ref["y"]).astype(np.float32)).astype(np.float64)
        ybar = k * ulp + U * ref["a"] * np.abs(ref["ad"])
        fy = _share(np.abs(_np(r["y"]).astype(np.float64) - ref["y"]), ybar)
        # g = dy (1 - y^2): y is uncertain by ybar, plus the roundings of y^2, of 1 - y^2 and of the product
        dg = np.abs(dy.astype(np.float64)) * (2 * np.abs(ref["y"]) * ybar + U * ref["y"] ** 2 + U * np.abs(ref["ad"])) + U * np.abs(ref["g"])
        axh = np.abs(ref["xh"])
        dxbar = ref["dxbar"] + ref["rstd"] * (dg + _pm(dg) + axh * _pm(dg * axh))
        fdx = _share(np.abs(_np(r["dx"]).astype(np.float64) - ref["dx"]), dxbar)
        _record("norm_act", "tanh " + name, fwd_share=fy, torch32_ulps=tfig, bar_ulps=k, bwd_share=fdx)
        assert fy <= 1.0 and fdx <= 1.0, (name, fy, fdx)


@pytest.mark.parametrize("backend", BACKENDS)
def test_norm_act_refusals(backend):
    """norm_act_bwd refuses C > 1024 like the forward (its chunked path would run with 256 / (C / 4) = 0 pixel rows); column sums
    requested where the launch cannot emit them are refused, not dropped."""
    ctx = _ctx(backend)
    x = torch.ones(1, 1028, 2, 2)
    with pytest.raises(ValueError, match="C > 1024"):
        engine.op_norm_act(ctx, x, act=LRELU)
    stats = torch.stack([torch.zeros(1, 1028), torch.ones(1, 1028)], dim=-1)
    for norm in (True, False):
        with pytest.raises(ValueError, match="C > 1024"):
            engine.op_norm_act(ctx, x, x, norm=norm, act=LRELU, stats_in=stats)          # the backward pass alone
    small = torch.randn(2, 8, 2, 2, generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match="colsum"):
        engine.op_norm_act(ctx, small, small, act=LRELU, want_colsum=2)                  # C % 32 != 0: the chunked path
    with pytest.raises(ValueError, match="colsum"):
        engine.op_norm_act(ctx, torch.randn(1, 32, 2, 2), torch.randn(1, 32, 2, 2), norm=False, act=LRELU, want_colsum=2)


def test_backward_alone_matches_the_pair():
    """swn_op_norm_act with stats_in (the backward pass alone on the caller's statistics) gives the bits of the forward + backward
    call when handed that call's statistics -- host simulator."""
    ctx = _ctx("sim")
    x = _make_x(1, 8, 3, 5, seed=2)
    dy = np.random.default_rng(4).standard_normal(x.shape).astype(np.float32)
    both = engine.op_norm_act(ctx, torch.from_numpy(x), torch.from_numpy(dy), act=LRELU)
    alone = engine.op_norm_act(ctx, torch.from_numpy(x), torch.from_numpy(dy), act=LRELU, stats_in=both["stats"])
    assert torch.equal(_bits(both["dx"]), _bits(alone["dx"]))


# ---- the bars against the kernels' arithmetic alone ---------------------------------------------------------------------------------
def _emulate(x, dy, mask, act):
    """numpy emulation of norm_act.hip: fp64 sums (of x - x0), mean / rstd rounded to fp32, fp32 (x - mean) * rstd, the fp64 combination of the
    backward rounded once."""
    f32 = np.float32
    x64 = x.astype(np.float64)
    d = x64 - x64[:, :, :1, :1]                                # sums of x - x0, x0 = the plane's first pixel
    md = _pm(d)
    var = np.maximum(_pm(d * d) - md * md, 0.0)
    mean, rstd = (x64[:, :, :1, :1] + md).astype(f32), (1.0 / np.sqrt(var + EPS)).astype(f32)
    xh = ((x - mean).astype(f32) * rstd).astype(f32)
    if act == LRELU:
        y, ad = np.where(xh > 0, xh, (f32(0.2) * xh).astype(f32)), np.where(xh > 0, f32(1), f32(0.2))
    elif act == RELU:
        y, ad = np.where(xh > 0, xh, f32(0)), np.where(xh > 0, f32(1), f32(0))
    else:
        y, ad = xh, np.ones_like(xh)
    mk = f32(1) if mask is None else mask.astype(f32)
    y = (y * mk).astype(f32)
    g = ((dy * ad).astype(f32) * mk).astype(f32)
    xhd = (x64 - mean.astype(np.float64)) * rstd.astype(np.float64)
    m1, m2 = _pm(g.astype(np.float64)), _pm(g.astype(np.float64) * xhd)
    dx = (rstd.astype(np.float64) * (g.astype(np.float64) - m1 - xhd * m2)).astype(f32)
    return y, dx


def test_bars_hold_for_an_emulation_of_the_kernels():
    """CPU only, no library call: the two analytic bars against a numpy emulation of the kernels' arithmetic over randn * 3 + 1.5, the
    mean-100 / std-0.01 plane, per-plane scales e^U(-6,3) with offsets and constant planes, at HW 4 / 65 / 257 / 1024 / 1025 / 2500,
    with activation none / LeakyReLU / ReLU + dropout 0.5.  The bar is thereby checked against the reference alone; the off-the-kink
    builder needs at most 2 rounds."""
    worst_f = worst_b = 0.0
    worst_rounds = 0
    for hw_i, (H, W) in enumerate(((2, 2), (5, 13), (1, 257), (32, 32), (25, 41), (50, 50))):
        rng = np.random.default_rng(50 + hw_i)
        C = 16
        x = (rng.standard_normal((1, C, H, W)) * 3 + 1.5).astype(np.float32)
        const = np.zeros((1, C), dtype=bool)
        x[:, 1] = 100 + 0.01 * rng.standard_normal((1, H, W))
        x[:, 9] = 100 + 0.01 * rng.standard_normal((1, H, W))
        x[:, 2] = 0.75
        const[:, 2] = True
        for c in (3, 5, 7, 11, 13):
            s = np.exp(rng.uniform(-6, 3))
            x[:, c] = s * (rng.standard_normal((1, H, W)) + 2 * rng.standard_normal())
        x, rounds = _off_the_kink(x, const)
        worst_rounds = max(worst_rounds, rounds)
        dy = rng.standard_normal(x.shape).astype(np.float32)
        for act, drop in ((NONE, 0), (LRELU, 0), (RELU, 1)):
            mask = (rng.random(x.shape) >= 0.5) * 2.0 if drop else None
            y, dx = _emulate(x, dy, mask, act)
            ref = _reference(x, dy, mask, None, act)
            ff = _share(np.abs(y.astype(np.float64) - ref["y"]), ref["ybar"])
            fb = _share(np.abs(dx.astype(np.float64) - ref["dx"]), ref["dxbar"])
            _record("emulation", "HW%d %s drop%d" % (H * W, ACT_NAMES[act], drop), fwd_share=ff, bwd_share=fb)
            worst_f, worst_b = max(worst_f, ff), max(worst_b, fb)
    _record("emulation", "worst", fwd_share=worst_f, bwd_share=worst_b, kink_rounds=worst_rounds)
    assert worst_f <= 1.0 and worst_b <= 1.0, (worst_f, worst_b)
    assert worst_rounds <= 2


# ---- second order ---------------------------------------------------------------------------------------------------------------------
def _double_backward(x, gy, u, act, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    gt = torch.from_numpy(gy).to(dtype).requires_grad_(True)
    ut = torch.from_numpy(u).to(dtype)
    mean = xt.mean(dim=(2, 3), keepdim=True)
    xh = (xt - mean) / torch.sqrt(((xt - mean) ** 2).mean(dim=(2, 3), keepdim=True) + EPS)
    y = torch.nn.functional.leaky_relu(xh, SLOPE) if act == LRELU else xh
    gx, = torch.autograd.grad(y, xt, gt, create_graph=True)
    uy, ax = torch.autograd.grad(gx, (gt, xt), ut)
    return uy.detach().double().numpy(), ax.detach().double().numpy()


def _figs(got, ref):
    pm = np.abs(ref).max(axis=(2, 3), keepdims=True)
    assert bool((pm > 0).all())
    return float((np.abs(got - ref) / pm).max()), float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("C", [8, 12, 320, 512])
def test_norm_act_bwd2_vs_float64(backend, C):
    """in2_partial_kernel / in2_finalize_kernel / in2_apply_kernel: C 8 and 12 (several pixel rows per block), 320 (two `cb` passes,
    64 live lanes in the second) and 512, at HW 63 and 31 x 31, activation none and LeakyReLU, against torch's float64 double
    backward.  Bar: 4 x what torch's fp32 CPU double backward is off on the same inputs -- element-wise over the plane's max|ref| and
    rel-L2 -- at least 2^-23."""
    ctx = _ctx(backend)
    for H, W in ((7, 9), (31, 31)):
        N = 2 if C <= 12 else 1
        x = _make_x(N, C, H, W, seed=60 + C, families=False)
        rng = np.random.default_rng(61 + C)
        gy, u = rng.standard_normal(x.shape).astype(np.float32), rng.standard_normal(x.shape).astype(np.float32)
        for act in (NONE, LRELU):
            outs = [engine.op_norm_act_bwd2(ctx, torch.from_numpy(x), torch.from_numpy(gy), torch.from_numpy(u), act=act) for _ in range(2)]
            ctx.sync()
            assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1])), "two runs differ"
            ref, t32 = _double_backward(x, gy, u, act, torch.float64), _double_backward(x, gy, u, act, torch.float32)
            for which, got, r64, r32 in zip(("uy", "ax"), outs[0], ref, t32):
                dmax, drel = _figs(_np(got).astype(np.float64), r64)
                tmax, trel = _figs(r32, r64)
                bmax, brel = 4 * max(tmax, 2.0 ** -23), 4 * max(trel, 2.0 ** -23)
                _record("norm_act_bwd2", "C%d %dx%d %s %s" % (C, H, W, ACT_NAMES[act], which), dev_max=dmax, torch32_max=tmax, dev_rel=drel,
                        torch32_rel=trel, share_max=dmax / bmax, share_rel=drel / brel)
                assert dmax <= bmax, (C, H, W, act, which, "max %.3g > bar %.3g" % (dmax, bmax))
                assert drel <= brel, (C, H, W, act, which, "rel-L2 %.3g > bar %.3g" % (drel, brel))
