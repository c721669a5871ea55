"""Operator-level tests of the element-wise kernels of norm_act.hip (act_fwd, act_bwd, axpy, reflect_fold) and of the resampling
half of gather.hip (upsample_nearest_fwd / bwd, maxpool2_fwd / bwd, act_pattern, pool_pattern).

Every launcher is called alone through swn_op_elementwise / swn_op_resample on channel-slice views: each operand lives in an NHWC
buffer of lead_c + C + pad_c channels (lead_c, pad_c in {0, 4}) filled with the byte 0x7f, the kernel gets buffer.slice(lead_c, C).
Each body runs on the CI host simulator and on the MI355X.  Shapes: C in {4, 8, 36}, H != W, N 1 or 2; the largest launch has 17
blocks.

Held in every call (_ew / _rs): two runs are bit-equal; the non-logical channels of the destination buffer keep the sentinel;
max(amax slot) equals the amax of the returned tensor bit for bit (a sentinel read from a neighbouring channel shows as 3.39e38).

Bit-exact against numpy fp32: act_fwd (none / LeakyReLU / ReLU), act_bwd (LeakyReLU / ReLU, accumulate 0 / 1), axpy with alpha = 1,
shift = 0, upsample_nearest_fwd (factors 1, 2, 4), maxpool2_fwd, maxpool2_bwd (the gradient goes to the first maximum in (kh, kw)
scan order, a NaN wins; reference written out in numpy), act_pattern (== y > 0) and pool_pattern (the window position that
received the gradient).
Bounded by roundings against float64 (U = 2^-24):
  axpy, general alpha / shift (the device may contract to an FMA)   2 U |result|, + U |old + result| when accumulating; the inputs
                                                                    keep alpha * x and shift from cancelling, the bar being relative
  upsample_nearest_bwd, a sum of f^2 terms                          (f^2 + accumulate) U (sum|terms| + |old|)
  reflect_fold, a sum of up to 4 terms                              (4 + accumulate) U (sum|terms| + |old|)
  act_bwd with tanh, dy (1 - y^2) through the OUTPUT y              U |dy| (y^2 + |1 - y^2|) + U |dx64| (+ U |old + dx64|)
tanh forward: the error in ulps of the float64 result, at most 4 x the worst figure of torch's fp32 CPU tanh on the same inputs
(magnitudes 2^-30 .. 2^5, both signs), at least 1 ulp.
"""
import numpy as np
import pytest
import torch

from swapnet_amd import engine
from tests import backends

BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]
U = 2.0 ** -24
SENT = engine.PAD_SENTINEL
NONE, LRELU, RELU, TANH = 0, 1, 2, 3
ACT_NAMES = ("none", "lrelu", "relu", "tanh")
F32 = np.float32
SHAPES = [(2, 4, 6, 10), (1, 8, 3, 5), (1, 36, 7, 9), (2, 36, 12, 20)]          # (N, C, H, W); the last one: 17 blocks of 256 threads


def _ctx(kind):
    return backends.gpu_ctx() if kind == "gpu" else backends.hostsim_ctx()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want, dtype=F32).view(np.int32))


def _record(kernel, case, **figs):
    print("NORMOPS %-14s %-52s %s" % (kernel, case, "  ".join("%s %.3g" % kv for kv in figs.items())))


def _views(i):
    """lead_c / pad_c in {0, 4} for the three operands, another combination for every i; all 64 over 64 consecutive i."""
    j = (i * 37 + 11) % 64
    return {"a": (4 * (j & 1), 4 * (j >> 1 & 1)), "b": (4 * (j >> 2 & 1), 4 * (j >> 3 & 1)), "out": (4 * (j >> 4 & 1), 4 * (j >> 5 & 1))}


def _check_buffer(buf, out, lead):
    c = out.shape[1]
    b = _bits(buf)
    assert torch.equal(b[:, lead:lead + c], _bits(out)), "the buffer's logical channels are not the returned tensor"
    assert bool((b[:, :lead] == SENT).all()) and bool((b[:, lead + c:] == SENT).all()), "a non-logical channel was written"


def _check_slot(slot, out):
    assert torch.equal(_bits(slot.max()), _bits(out.abs().max())), "max(slot) %.9g != amax %.9g" % (float(slot.max()), float(out.abs().max()))


def _ew(ctx, op, a, b=None, vi=0, old=None, **kw):
    """swn_op_elementwise twice with what holds in every call; returns the result as numpy."""
    views = _views(vi)
    runs = [engine.op_elementwise(ctx, op, _t(a), _t(b), old=_t(old), accumulate=old is not None, views=views, **kw) for _ in range(2)]
    ctx.sync()
    (out, slot, buf), (out2, slot2, buf2) = runs
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(buf), _bits(buf2)), "two runs differ"
    _check_buffer(buf, out, views["out"][0])
    _check_slot(slot, out)
    return _np(out)


def _rs(ctx, op, a, b=None, vi=0, old=None, slot_exact=True, **kw):
    """swn_op_resample twice with what holds in every call; returns (out, pattern) as numpy."""
    views = _views(vi)
    runs = [engine.op_resample(ctx, op, _t(a), _t(b), old=_t(old), accumulate=old is not None, views=views, **kw) for _ in range(2)]
    ctx.sync()
    (out, slot, pat, buf), (out2, _, pat2, buf2) = runs
    if out is not None:
        assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(buf), _bits(buf2)), "two runs differ"
        _check_buffer(buf, out, views["out"][0])
    if pat is not None:
        assert torch.equal(pat.cpu(), pat2.cpu())
    if slot is not None and slot_exact:
        _check_slot(slot, out)
    return (None if out is None else _np(out)), (None if pat is None else _np(pat))


def _randn(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


def _with_edges(x):
    """Zeros of both signs and large values among the first elements of every plane."""
    x = x.copy()
    edge = np.array([0.0, -0.0, 3e38, -3e38], dtype=F32)
    flat = x.reshape(x.shape[0], x.shape[1], -1)
    k = min(len(edge), flat.shape[2])
    flat[:, :, :k] = edge[:k]
    return flat.reshape(x.shape)


# ---- act_fwd / act_bwd / axpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_act_fwd_act_bwd_axpy_bit_exact(backend):
    ctx = _ctx(backend)
    slope = F32(0.2)
    vi = 0
    for si, shape in enumerate(SHAPES):
        x, dy, old = _with_edges(_randn(shape, 1 + si)), _randn(shape, 11 + si), _randn(shape, 21 + si)
        for act in (NONE, LRELU, RELU):
            y = _ew(ctx, engine.EW_ACT_FWD, x, act=act, vi=(vi := vi + 1))
            want = x if act == NONE else np.where(x > 0, x, slope * x if act == LRELU else F32(0))
            assert _same_bits(y, want), ("act_fwd", ACT_NAMES[act], shape)
            pat = _rs(ctx, engine.RS_ACT_PATTERN, y, vi=(vi := vi + 1))[1]
            assert np.array_equal(pat, (y > 0).astype(np.uint8)), "act_pattern is not y > 0 of the returned y"
            if act == NONE:
                continue
            ad = np.where(y > 0, F32(1), slope if act == LRELU else F32(0))
            for acc in (0, 1):
                dx = _ew(ctx, engine.EW_ACT_BWD, dy, y, act=act, old=old if acc else None, vi=(vi := vi + 1))
                want = (dy * ad).astype(F32)
                assert _same_bits(dx, want + old if acc else want), ("act_bwd", ACT_NAMES[act], shape, acc)
        for acc in (0, 1):
            got = _ew(ctx, engine.EW_AXPY, x, alpha=1.0, shift=0.0, old=old if acc else None, vi=(vi := vi + 1))
            want = (x * F32(1) + F32(0)).astype(F32)
            assert _same_bits(got, want + old if acc else want), ("axpy alpha 1 shift 0", shape, acc)
        _record("elementwise", "act_fwd/act_bwd/axpy(1,0) %s" % "x".join(map(str, shape)), bit_exact=1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_axpy_general_vs_float64(backend):
    """alpha * x + shift may be one FMA or two roundings: 2 U |result| covers both.  x >= 0 with alpha and shift of one sign, and
    shift = 0 with x of both signs: nothing cancels."""
    ctx = _ctx(backend)
    worst = 0.0
    vi = 100
    for si, shape in enumerate(SHAPES):
        old = _randn(shape, 31 + si)
        for alpha, shift, positive in ((1.7, 0.3, True), (-0.37, -2.5, True), (0.001953125, 0.0, False), (-3.3, 0.0, False), (1.0, 0.625, True)):
            x = _randn(shape, 41 + si)
            x = np.abs(x) if positive else x
            res = float(F32(alpha)) * x.astype(np.float64) + float(F32(shift))
            for acc in (0, 1):
                got = _ew(ctx, engine.EW_AXPY, x, alpha=alpha, shift=shift, old=old if acc else None, vi=(vi := vi + 1)).astype(np.float64)
                want = res + old if acc else res
                bar = 2 * U * np.abs(res) + (U * np.abs(want) if acc else 0.0)
                fig = float((np.abs(got - want) / bar).max())
                worst = max(worst, fig)
                assert fig <= 1.0, ("axpy", shape, alpha, shift, acc, fig)
    _record("axpy", "general alpha / shift", err_over_bar=worst)


def _tanh_sweep(shape, seed):
    rng = np.random.default_rng(seed)
    return (np.exp2(rng.uniform(-30, 5, size=shape)) * rng.choice([-1.0, 1.0], size=shape)).astype(F32)


@pytest.mark.parametrize("backend", BACKENDS)
def test_tanh_forward_and_backward_through_the_output(backend):
    ctx = _ctx(backend)
    shape = (2, 36, 12, 20)
    x = _tanh_sweep(shape, 51)
    y64 = np.tanh(x.astype(np.float64))
    ulp = np.spacing(np.abs(y64).astype(F32)).astype(np.float64)
    tfig = float((np.abs(torch.tanh(_t(x)).numpy().astype(np.float64) - y64) / ulp).max())
    k = 4.0 * max(tfig, 1.0)
    y = _ew(ctx, engine.EW_ACT_FWD, x, act=TANH, vi=7)
    fig = float((np.abs(y.astype(np.float64) - y64) / ulp).max())
    _record("act_fwd", "tanh 2^-30..2^5", dev_ulps=fig, torch32_ulps=tfig, bar_ulps=k)
    assert fig <= k, "tanh: %.3g ulp > %.3g" % (fig, k)
    # backward through the OUTPUT: any y in [-1, 1] will do, the kernel never sees x
    dy, old = _randn(shape, 52), _randn(shape, 53)
    yy = y.astype(np.float64)
    dx64 = dy.astype(np.float64) * (1 - yy * yy)
    for acc in (0, 1):
        got = _ew(ctx, engine.EW_ACT_BWD, dy, y, act=TANH, old=old if acc else None, vi=8 + acc).astype(np.float64)
        want = dx64 + old if acc else dx64
        bar = U * np.abs(dy) * (yy * yy + np.abs(1 - yy * yy)) + U * np.abs(dx64) + (U * np.abs(want) if acc else 0.0)
        ok = bar > 0
        assert bool((got[~ok] == want[~ok]).all())
        fig = float((np.abs(got - want)[ok] / bar[ok]).max())
        _record("act_bwd", "tanh through y acc%d" % acc, err_over_bar=fig)
        assert fig <= 1.0, ("act_bwd tanh", acc, fig)


# ---- nearest upsampling ------------------------------------------------------------------------------------------------------------
UP_SHAPES = [(2, 4, 6, 10), (1, 8, 3, 5), (1, 36, 3, 5), (2, 36, 5, 3)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("f", [1, 2, 4])
def test_upsample_nearest(backend, f):
    """Forward: a copy, bit for bit (6 x 10 -> 12 x 20, 3 x 5 -> 12 x 20).  Backward: the f^2 gradients of a source pixel added in fp32."""
    ctx = _ctx(backend)
    worst = 0.0
    for si, shape in enumerate(UP_SHAPES):
        n, c, h, w = shape
        x = _with_edges(_randn(shape, 61 + si))
        y = _rs(ctx, engine.RS_UPSAMPLE_FWD, x, factor=f, vi=si + 10 * f)[0]
        assert y.shape == (n, c, h * f, w * f)
        assert _same_bits(y, x.repeat(f, axis=2).repeat(f, axis=3)), ("upsample_nearest_fwd", shape, f)
        dy, old = _randn((n, c, h * f, w * f), 71 + si), _randn(shape, 81 + si)
        terms = dy.astype(np.float64).reshape(n, c, h, f, w, f)
        ref, tot = terms.sum(axis=(3, 5)), np.abs(terms).sum(axis=(3, 5))
        for acc in (0, 1):
            got = _rs(ctx, engine.RS_UPSAMPLE_BWD, dy, factor=f, old=old if acc else None, vi=si + 10 * f + 3 + acc)[0].astype(np.float64)
            want = ref + old if acc else ref
            bar = (f * f + acc) * U * (tot + (np.abs(old) if acc else 0.0))
            fig = float((np.abs(got - want) / bar).max())
            worst = max(worst, fig)
            assert fig <= 1.0, ("upsample_nearest_bwd", shape, f, acc, fig)
            if f == 1 and not acc:
                assert _same_bits(got.astype(F32), dy)
    _record("upsample_bwd", "f%d" % f, err_over_bar=worst)


# ---- MaxPool2d(2, 2) --------------------------------------------------------------------------------------------------------------------
def _pool_input(shape, seed, special):
    """randn rounded to multiples of 1/4 (exact ties are common); with `special`, the first windows of every plane are: all equal,
    a tie of the two maxima at positions 1 and 2, a tie at 2 and 3, one NaN (at position 2), all -inf, -inf with one finite value."""
    x = (np.round(_randn(shape, seed) * 4) / 4).astype(F32)
    if special:
        wins = [[1.5, 1.5, 1.5, 1.5], [0.0, 2.0, 2.0, -1.0], [-3.0, -5.0, -2.0, -2.0], [1.0, 9.0, np.nan, 3.0],
                [-np.inf] * 4, [-np.inf, -np.inf, -np.inf, -7.0]]
        for i, wv in enumerate(wins[: shape[3] // 2]):
            x[:, :, 0:2, 2 * i:2 * i + 2] = np.array(wv, dtype=F32).reshape(2, 2)
    return x


def _pool_ref(x):
    """Scan (kh, kw) with a strict '>', a NaN replaces the running maximum: (max, window position), written out."""
    n, c, h, w = x.shape
    win = x.reshape(n, c, h // 2, 2, w // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    m, am = win[..., 0].copy(), np.zeros(win.shape[:-1], dtype=np.uint8)
    for t in range(1, 4):
        v = win[..., t]
        with np.errstate(invalid="ignore"):
            take = (v > m) | np.isnan(v)
        m = np.where(take, v, m)
        am = np.where(take, np.uint8(t), am)
    return m, am


@pytest.mark.parametrize("backend", BACKENDS)
def test_maxpool2(backend):
    ctx = _ctx(backend)
    vi = 200
    for si, shape in enumerate([(2, 4, 6, 10), (1, 8, 4, 12), (1, 36, 6, 14), (2, 36, 12, 20)]):
        n, c, h, w = shape
        for special in (False, True):
            x = _pool_input(shape, 91 + si, special)
            m, am = _pool_ref(x)
            # forward (the amax slot on NaN-free maps: fmaxf drops a NaN, which no slot consumer relies on)
            y, pat = _rs(ctx, engine.RS_MAXPOOL_FWD, x, vi=(vi := vi + 1), slot_exact=not special)
            assert _same_bits(y, m), ("maxpool2_fwd", shape, special)
            assert np.array_equal(pat, am), "pool_pattern is not the first maximum in scan order"
            dy, old = _randn((n, c, h // 2, w // 2), 95 + si), _randn(shape, 97 + si)
            want = np.zeros((n, c, h // 2, w // 2, 4), dtype=F32)
            np.put_along_axis(want, am[..., None].astype(np.int64), dy[..., None], axis=-1)
            want = want.reshape(n, c, h // 2, w // 2, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(shape)
            for acc in (0, 1):
                dx, pat = _rs(ctx, engine.RS_MAXPOOL_BWD, x, dy, old=old if acc else None, vi=(vi := vi + 1))
                assert _same_bits(dx, want + old if acc else want), ("maxpool2_bwd", shape, special, acc)
                assert np.array_equal(pat, am)
                if not acc:          # the pattern names the window position that received the gradient
                    recv = dx.reshape(n, c, h // 2, 2, w // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
                    assert bool((np.take_along_axis(recv, pat[..., None].astype(np.int64), axis=-1)[..., 0] == dy).all())
                    assert bool(((recv != 0).sum(axis=-1) <= 1).all())
        _record("maxpool2", "fwd/bwd/pattern %s" % "x".join(map(str, shape)), bit_exact=1)


# ---- reflect_fold -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_reflect_fold_is_the_adjoint_of_reflection_pad(backend):
    """4 x 4 (the minimum: rows 1 and H - 2 are neighbours), 4 x 7, 5 x 4, 9 x 6, against float64 autograd through
    F.pad(mode="reflect"); sum|terms| is the same adjoint applied to |dxpad|."""
    ctx = _ctx(backend)
    worst = 0.0
    vi = 300
    for si, (n, c, h, w) in enumerate([(2, 4, 4, 4), (1, 8, 4, 7), (1, 36, 5, 4), (2, 36, 9, 6)]):
        g = _randn((n, c, h + 2, w + 2), 101 + si)
        old = _randn((n, c, h, w), 111 + si)

        def adjoint(v):
            z = torch.zeros((n, c, h, w), dtype=torch.float64, requires_grad=True)
            torch.nn.functional.pad(z, (1, 1, 1, 1), mode="reflect").backward(torch.from_numpy(v.astype(np.float64)))
            return z.grad.numpy()
        ref, tot = adjoint(g), adjoint(np.abs(g))
        for acc in (0, 1):
            got = _rs(ctx, engine.RS_REFLECT_FOLD, g, old=old if acc else None, vi=(vi := vi + 1))[0].astype(np.float64)
            want = ref + old if acc else ref
            bar = (4 + acc) * U * (tot + (np.abs(old) if acc else 0.0))
            fig = float((np.abs(got - want) / bar).max())
            worst = max(worst, fig)
            assert fig <= 1.0, ("reflect_fold", (n, c, h, w), acc, fig)
    _record("reflect_fold", "4x4 4x7 5x4 9x6", err_over_bar=worst)
    with pytest.raises(ValueError, match="reflect_fold"):
        engine.op_resample(ctx, engine.RS_REFLECT_FOLD, torch.zeros(1, 4, 5, 5))         # 3 x 3: rows 1 and H - 2 coincide
