"""AdaBound (Luo et al., ICLR 2019) as adabound 0.0.5 executes it with amsbound off -- the optimizer behind the reference's
--optimizer_G / --optimizer_D AdaBound (optimizers/__init__.py:37-60) -- as a fused HIP update: swn_op_adabound, the per-network
choice swn_model_set_optimizer, and NativeAdaBound behind define_optimizer.

The reference of every numeric check is `adabound_f64` below, the float64 restatement of the published update; parity is against
that algorithm, not against the package binary (which is not installed and never imported).

Bars.  p: |p_hip - p_ref| <= 1e-5 (|p_old| + |dp_ref|) + 1e-7, the bar of test_ops.test_adamw_matches_torch (about a dozen fp32
roundings of 2^-24 per element, an order of magnitude of head-room).  m and v: 1e-6 relative.  Both moments are sums of two
rounded terms, m = b1 m + (1 - b1) g' and v = b2 v + (1 - b2) g'^2 with g' = g + wd p itself a rounded sum, so the fp32 error
is relative to the magnitude of the terms, not to a result the terms may cancel in (m with alternating gradient signs, g' where
g ~ -wd p): the scale of the 1e-6 is |b1 m| + (1 - b1)(|g| + wd |p|) for m and b2 v + (1 - b2)(|g| + wd |p|)^2 for v, which IS
|m_ref| / v_ref wherever nothing cancels.  Four roundings of 2^-24 = 2.4e-7 of that scale are the worst case."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

from swapnet_amd import _C, engine
from tests import backends

pytestmark = pytest.mark.small_channel_winograd      # tests/conftest.py: small shapes on the Winograd forms

GAMMA, EPS = 1e-3, 1e-8          # the package defaults; the reference never passes others


def f32(x):
    """The value a float argument has once it crossed the C ABI."""
    return float(np.float32(x))


def f64(a):
    return torch.as_tensor(a).to(torch.float64)


def adabound_f64(p, g, m, v, lr, b1, b2, eps, wd, final_lr, base_lr, gamma, step):
    """One AdaBound step in float64 (numpy arrays or torch tensors in, float64 torch tensors on the same device out).  Returns
    (p, m, v, regime), regime = -1 / 0 / +1 where the per-element rate was clamped to the lower bound / left alone / clamped to
    the upper bound."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    g = g + wd * p                                        # coupled L2, not AdamW's decoupled decay
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() + eps                                # no bias correction inside denom
    step_size = lr * (1.0 - b2 ** step) ** 0.5 / (1.0 - b1 ** step)
    final = final_lr * lr / base_lr
    lower = final * (1.0 - 1.0 / (gamma * step + 1.0))
    upper = final * (1.0 + 1.0 / (gamma * step))
    raw = step_size / denom
    regime = (raw > upper).to(torch.int8) - (raw < lower).to(torch.int8)
    return p - raw.clamp(lower, upper) * m, m, v, regime


def assert_step_matches(got, old, g, ref, b1, b2, wd, what):
    """got / old / ref = (p, m, v) after the kernel / before the step / after the restatement."""
    got = [f64(a) for a in got]
    for a in got:
        assert bool(torch.isfinite(a).all()), (what, "NaN or Inf")
    p_old, m_old, v_old = (f64(a) for a in old)
    gmag = f64(g).abs() + wd * p_old.abs()
    checks = (("p", (got[0] - ref[0]).abs(), 1e-5 * (p_old.abs() + (ref[0] - p_old).abs()) + 1e-7),
              ("m", (got[1] - ref[1]).abs(), 1e-6 * ((b1 * m_old).abs() + (1.0 - b1) * gmag)),
              ("v", (got[2] - ref[2]).abs(), 1e-6 * (b2 * v_old + (1.0 - b2) * gmag * gmag)))
    print("%s: worst err / bar " % what + "  ".join("%s %.3f" % (n, float((e / b.clamp_min(1e-300)).max())) for n, e, b in checks))
    for name, err, bar in checks:
        bad = torch.nonzero(err > bar).flatten()
        assert bad.numel() == 0, (what, name, "elements over the bar", bad.numel(), "first", int(bad[0]), float(err[bad[0]]), float(bar[bad[0]]))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_restatement_against_a_hand_worked_example():
    """Step 1, wd = 0, lr = base_lr = 1e-3, final_lr = 0.1, betas (0.9, 0.999), gamma 1e-3, eps 1e-8, p = (1, 1), g = (1000, 0.5).
    By hand: m = 0.1 g = (100, 0.05); v = 0.001 g^2 = (1000, 2.5e-4); step_size = 1e-3 sqrt(0.001) / 0.1 = 3.16227766e-4;
    lower = 0.1 (1 - 1/1.001) = 9.99000999e-5, upper = 0.1 * 1001 = 100.1.
    Element 0: sqrt(v) = 31.6227766, rate = 3.16227766e-4 / 31.62277661 = 9.99999997e-6 < lower -> clamped low,
               p = 1 - 9.99000999e-5 * 100 = 0.99000999001.
    Element 1: sqrt(v) = 0.0158113883, rate = 3.16227766e-4 / 0.0158113983 = 0.0199999874 (inside the bounds),
               p = 1 - 0.0199999874 * 0.05 = 0.99900000063."""
    p, m, v, regime = adabound_f64([1.0, 1.0], [1000.0, 0.5], [0.0, 0.0], [0.0, 0.0], 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 1e-3, 1e-3, 1)
    assert regime.tolist() == [-1, 0]
    np.testing.assert_allclose(m.numpy(), [100.0, 0.05], rtol=1e-12)
    np.testing.assert_allclose(v.numpy(), [1000.0, 2.5e-4], rtol=1e-9)
    np.testing.assert_allclose(p.numpy(), [0.99000999001, 0.99900000063], rtol=0, atol=2e-11)
    # g = 0 and v = 0: step_size / eps clamps to the upper bound, times m = 0 -- finite, p unchanged
    p, m, v, regime = adabound_f64([0.5], [0.0], [0.0], [0.0], 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 1e-3, 1e-3, 1)
    assert regime.tolist() == [1] and p.tolist() == [0.5] and m.tolist() == [0.0] and v.tolist() == [0.0]


def _sim_net(net):
    from swapnet_amd.modules.native import NativeBackend, NativeNet
    backend = NativeBackend("warp", is_train=True, ctx=backends.hostsim_ctx(), default_shape=(2, 64, 64))
    return NativeNet(backend, net)


def test_options_and_the_simulator_refusal():
    from swapnet_amd import optimizers
    parser = optimizers.get_options_modifier("AdaBound")(argparse.ArgumentParser())
    ns = parser.parse_args([])
    assert (ns.b1, ns.b2, ns.final_lr) == (0.9, 0.999, 0.1)
    assert parser.parse_args(["--final_lr", "0.02"]).final_lr == 0.02
    opt = argparse.Namespace(optimizer_G="AdamW", optimizer_D="AdaBound", lr=1e-4, d_lr=4e-4, weight_decay=0.0, d_weight_decay=0.01,
                             b1=0.9, b2=0.999, final_lr=0.1)
    with pytest.raises(NotImplementedError, match="simulator"):
        optimizers.define_optimizer(_sim_net(engine.NET_D), opt, "D")
    o = optimizers.define_optimizer(_sim_net(engine.NET_G), opt, "G")              # AdamW on the simulator still works
    assert isinstance(o, optimizers.NativeAdamW) and not isinstance(o, optimizers.NativeAdaBound)
    assert o.param_groups[0]["lr"] == 1e-4 and "final_lr" not in o.param_groups[0]
    # ... and the library itself refuses, it never steps AdamW under AdaBound's name
    ctx = backends.hostsim_ctx()
    m = backends.get_model(ctx, "warp", 2, 64)
    with pytest.raises(NotImplementedError, match="simulator"):
        m.set_optimizer(engine.NET_D, engine.OPT_ADABOUND, final_lr=0.1, base_lr=4e-4)
    m.set_optimizer(engine.NET_D, engine.OPT_ADAMW)
    z = torch.zeros(8)
    with pytest.raises(NotImplementedError, match="simulator"):
        ctx.lib.call("swn_op_adabound", ctx.handle, _C.ptr(z), _C.ptr(z), _C.ptr(z), _C.ptr(z), C.c_size_t(8), C.c_float(1e-3),
                     C.c_float(0.9), C.c_float(0.999), C.c_float(1e-8), C.c_float(0.0), C.c_float(0.1), C.c_float(1e-3), C.c_float(1e-3), 1)


# ---- the op ------------------------------------------------------------------------------------------------------------------
OP_LR, OP_FINAL = f32(1e-3), f32(0.1)
OP_B1, OP_B2 = f32(0.9), f32(0.999)
OP_STEPS = (1, 2, 3, 3000)


def op_case(n, seed):
    """p, the per-step gradients and the hyper-parameters of the op tests.  With s = 10 lr / final_lr the rate of step 1 is
    final_lr s / |g|, inside the bounds for |g| / s in [1e-3, 1e3]; by step 3000 (on moments carried over three steps) the bounds
    have closed to final_lr [0.75, 1.33], i.e. |g| / s in [1.16, 2.05].  So the magnitudes |g| / s are drawn from a mixture over
    twelve decades that keeps every regime populated at every step: 20 % in 1e3.3 .. 1e6 (always clamped low), 15 % in 1e-6 ..
    1e-3.3 and 5 % exact zeros (always clamped high), 30 % in 1.2 .. 2.0 (never clamped), 30 % log-uniform in 1e-3 .. 1e3
    (unclamped early, clamped one way or the other late).  Every step draws fresh signs; the weights are spread over six
    decades so that wd p is the larger term of g + wd p for some elements and negligible for others."""
    r = np.random.default_rng(seed)
    s = 10.0 * OP_LR / OP_FINAL
    cls = r.choice(5, size=n, p=[0.20, 0.15, 0.05, 0.30, 0.30])
    lo = np.array([3.3, -6.0, 0.0, np.log10(1.2), -3.0])[cls]
    hi = np.array([6.0, -3.3, 0.0, np.log10(2.0), 3.0])[cls]
    mag = s * 10.0 ** (lo + (hi - lo) * r.random(n))
    mag[cls == 2] = 0.0
    grads = [(mag * r.choice([-1.0, 1.0], size=n)).astype(np.float32) for _ in OP_STEPS]
    p = (r.standard_normal(n) * 10.0 ** r.uniform(-6.0, 0.0, n)).astype(np.float32)
    return p, grads


def op_hyper(wd, step):
    return dict(lr=OP_LR, b1=OP_B1, b2=OP_B2, eps=f32(EPS), wd=f32(wd), final_lr=OP_FINAL, base_lr=OP_LR, gamma=f32(GAMMA), step=step)


def assert_coverage(regime, what):
    share = [float((regime == k).double().mean()) for k in (-1, 0, 1)]
    assert min(share) >= 0.10, (what, "share of elements clamped low / unclamped / clamped high", share)


def call_op(ctx, p, g, m, v, n, h, off=0):
    ctx.lib.call("swn_op_adabound", ctx.handle, C.c_void_p(p.data_ptr() + 4 * off), C.c_void_p(g.data_ptr() + 4 * off),
                 C.c_void_p(m.data_ptr() + 4 * off), C.c_void_p(v.data_ptr() + 4 * off), C.c_size_t(n),
                 C.c_float(h["lr"]), C.c_float(h["b1"]), C.c_float(h["b2"]), C.c_float(h["eps"]), C.c_float(h["wd"]),
                 C.c_float(h["final_lr"]), C.c_float(h["base_lr"]), C.c_float(h["gamma"]), int(h["step"]))


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_op_case_covers_every_regime(wd):
    """The coverage condition of the GPU test, from the restatement alone (and without a GPU): at every checked step at least
    10 % of the elements are clamped low, 10 % unclamped, 10 % clamped high."""
    for n in (1028, 4104):
        p, grads = op_case(n, seed=n)
        m, v = np.zeros(n), np.zeros(n)
        for g, step in zip(grads, OP_STEPS):
            p, m, v, regime = adabound_f64(p, g, m, v, **op_hyper(wd, step))
            assert_coverage(regime, (n, wd, step))
            assert bool(torch.isfinite(torch.stack([p, m, v])).all())


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", [4, 1028, 4104, 4194304 + 1200])
def test_op_matches_the_restatement(n, wd):
    """n = 4: one float4; 1028: one past a block; 4104; 4 194 304 + 1200: a second trip of the grid-stride loop (the grid is
    capped at 4096 blocks x 256 threads x 4 floats) with a partial block.  State carried through steps 1, 2, 3, then step 3000
    on the carried moments."""
    ctx = backends.gpu_ctx()
    p0, grads = op_case(n, seed=n)
    # the restatement on its own first: the case must populate all three regimes at every step (n = 4 is too few to hold shares)
    if n >= 1000:
        p, m, v = p0, np.zeros(n), np.zeros(n)
        for g, step in zip(grads, OP_STEPS):
            p, m, v, regime = adabound_f64(p, g, m, v, **op_hyper(wd, step))
            assert_coverage(regime, (n, wd, step))
    pd = torch.from_numpy(p0.copy()).to(ctx.device)
    md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
    for g, step in zip(grads, OP_STEPS):
        old = [t.cpu().numpy().copy() for t in (pd, md, vd)]
        gd = torch.from_numpy(g).to(ctx.device)
        h = op_hyper(wd, step)
        call_op(ctx, pd, gd, md, vd, n, h)
        got = [t.cpu().numpy() for t in (pd, md, vd)]
        ref = adabound_f64(old[0], g, old[1], old[2], **h)
        if n >= 1000:
            assert_coverage(ref[3], (n, wd, step, "from the kernel's carried state"))
        assert_step_matches(got, old, g, ref[:3], h["b1"], h["b2"], h["wd"], "n %d wd %g step %d" % (n, wd, step))


@pytest.mark.gpu
def test_op_launch_geometry_does_not_matter():
    """One call over [0, n) equals, bitwise, two calls over 16-byte-aligned halves."""
    ctx = backends.gpu_ctx()
    n, cut = 4104, 1028
    p0, grads = op_case(n, seed=7)
    out = []
    for split in (False, True):
        pd = torch.from_numpy(p0.copy()).to(ctx.device)
        md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
        for g, step in zip(grads, OP_STEPS):
            gd = torch.from_numpy(g).to(ctx.device)
            h = op_hyper(0.01, step)
            if split:
                call_op(ctx, pd, gd, md, vd, cut, h)
                call_op(ctx, pd, gd, md, vd, n - cut, h, off=cut)
            else:
                call_op(ctx, pd, gd, md, vd, n, h)
        out.append([t.cpu() for t in (pd, md, vd)])
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ---- the model step ------------------------------------------------------------------------------------------------------------
B, H = 2, 64                  # the smallest shape the existing model tests use
LABELS = [(0.75, 1.05, 0.9), (0.8, 1.0, 0.95), (0.85, 0.95, 1.0), (0.7, 1.1, 0.9), (0.9, 0.9, 1.05)]
HYPER = dict(lr=1e-4, d_lr=4e-4, weight_decay=0.0, d_weight_decay=0.01, b1=0.9, b2=0.999)
FINAL_LR = 0.1


def _net_hyper(net):
    k = "d_" if net == engine.NET_D else ""
    return dict(lr=f32(HYPER[k + "lr"]), b1=f32(HYPER["b1"]), b2=f32(HYPER["b2"]), eps=f32(EPS), wd=f32(HYPER[k + "weight_decay"]))


_seeded = {}


def seeded_state():
    """Weights and batch, computed once and never modified."""
    from oracle import swapnet_oracle as O              # seeded weights and batch only (the checker's generators)
    if not _seeded:
        torch.manual_seed(3)
        _seeded.update(G=O.warp_module_params(), D=O.patchgan_params(22), batch=O.synth_warp_batch(B, H, H, seed=5))
    return _seeded


def new_model(ctx, kinds):
    """kinds = (G's optimizer, D's optimizer)."""
    s = seeded_state()
    m = engine.NativeModel(ctx, "warp", B, H, H, is_train=True)
    backends.reset_state(m, {engine.NET_G: s["G"], engine.NET_D: s["D"]})
    m.set_hyper(**HYPER)
    for net, kind in zip((engine.NET_G, engine.NET_D), kinds):
        base = HYPER["lr"] if net == engine.NET_G else HYPER["d_lr"]
        m.set_optimizer(net, kind, final_lr=FINAL_LR, base_lr=base, gamma=GAMMA)
    for i, t in enumerate(s["batch"]):
        m.set_input(i, t)
    return m


def snapshot(m):
    return [m.arena(net, which).clone().cpu() for net in (engine.NET_G, engine.NET_D)
            for which in (engine.W_WEIGHT, engine.W_EXP_AVG, engine.W_EXP_AVG_SQ)]


def phased_step(m, k, check=None):
    """forward, backward_D, optimizer_step(D), backward_G, optimizer_step(G); check(net) runs around each optimizer step."""
    lab = LABELS[k]
    m.forward(True, 100 + 17 * k)
    for net in (engine.NET_D, engine.NET_G):
        if net == engine.NET_D:
            m.backward_D(lab[0], lab[1])
        else:
            m.backward_G(lab[2])
        if check:
            check(net, k)
        else:
            m.optimizer_step(net)


def run_steps(ctx, kinds, steps, mode, edit=None):
    """`steps` training steps, mode = "phased" | "fused" (swn_model_step) | "captured" (swn_model_step_captured: eager, record,
    replay ...).  edit = (k, final_lr): both optimizers get that final_lr before step k.  Returns (losses per step, final state)."""
    m = new_model(ctx, kinds)
    try:
        losses = []
        for k in range(steps):
            if edit and k == edit[0]:
                for net, kind in zip((engine.NET_G, engine.NET_D), kinds):
                    m.set_optimizer(net, kind, final_lr=edit[1], base_lr=HYPER["lr"] if net == engine.NET_G else HYPER["d_lr"], gamma=GAMMA)
            if mode == "phased":
                phased_step(m, k)
            else:
                m.step(LABELS[k], training=True, seed=100 + 17 * k, captured=mode == "captured")
            losses.append(m.losses())
        assert m.optim_step_count(engine.NET_G) == steps and m.optim_step_count(engine.NET_D) == steps
        return losses, snapshot(m)
    finally:
        m.close()


_phased = {}


def phased(ctx, kinds, steps, edit=None):
    """The phased reference run, computed once per configuration."""
    key = (kinds, steps, edit)
    if key not in _phased:
        _phased[key] = run_steps(ctx, kinds, steps, "phased", edit)
    return _phased[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", [(engine.OPT_ADABOUND, engine.OPT_ADAMW), (engine.OPT_ADAMW, engine.OPT_ADABOUND)], ids=["G", "D"])
def test_model_step_applies_adabound_to_the_chosen_network(kinds):
    """Two phased steps; the restatement applied to the weights, moments and gradients read back before each AdaBound step must
    give the post-step weights, per named parameter.  With G = AdaBound, D = AdamW, D's weights after step 1 are bitwise those of
    an all-AdamW model (D is stepped before G's optimizer is used)."""
    ctx = backends.gpu_ctx()
    m = new_model(ctx, kinds)
    d_after_first = []

    def check(net, k):
        if kinds[net] != engine.OPT_ADABOUND:
            m.optimizer_step(net)
            if net == engine.NET_D and k == 0:
                d_after_first.append(m.arena(engine.NET_D, engine.W_WEIGHT).clone().cpu())
            return
        which = (engine.W_WEIGHT, engine.W_EXP_AVG, engine.W_EXP_AVG_SQ)
        before = {w: m.state_dict(net, which=w) for w in which + (engine.W_GRAD,)}          # device tensors: clones of the arenas
        m.optimizer_step(net)
        after = {w: m.state_dict(net, which=w) for w in which}
        h = _net_hyper(net)
        for name in m.param_infos(net):
            old = [before[w][name].flatten() for w in which]
            g = before[engine.W_GRAD][name].flatten()
            ref = adabound_f64(old[0], g, old[1], old[2], final_lr=f32(FINAL_LR), base_lr=h["lr"], gamma=f32(GAMMA), step=k + 1, **h)
            got = [after[w][name].flatten() for w in which]
            assert_step_matches(got, old, g, ref[:3], h["b1"], h["b2"], h["wd"], "net %d step %d %s" % (net, k + 1, name))
            assert not torch.equal(got[0], old[0]) or not bool(g.any()), (name, "weights did not move")

    try:
        for k in range(2):
            phased_step(m, k, check)
        assert m.optim_step_count(engine.NET_G) == 2 and m.optim_step_count(engine.NET_D) == 2
        assert all(np.isfinite(v) for v in m.losses().values())
    finally:
        m.close()
    if kinds[engine.NET_D] == engine.OPT_ADAMW:
        ref = new_model(ctx, (engine.OPT_ADAMW, engine.OPT_ADAMW))
        try:
            ref.forward(True, 100)
            ref.backward_D(LABELS[0][0], LABELS[0][1])
            ref.optimizer_step(engine.NET_D)
            assert torch.equal(ref.arena(engine.NET_D, engine.W_WEIGHT).cpu(), d_after_first[0])
        finally:
            ref.close()


BOTH = (engine.OPT_ADABOUND, engine.OPT_ADABOUND)


def assert_same_run(got, want):
    for k, (a, b) in enumerate(zip(got[0], want[0])):
        assert a == b, ("losses of step", k, a, b)
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        assert torch.equal(a, b), ("state tensor", i, float((a - b).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fused", "captured"])
def test_fused_and_captured_steps_are_the_phased_step(mode):
    """AdaBound on both networks: swn_model_step (bucketed, side stream) and three swn_model_step_captured calls (eager, record,
    replay) give the weights, moments and losses of the phased steps, bit for bit (the pattern of tests/test_captured_step.py)."""
    ctx = backends.gpu_ctx()
    assert_same_run(run_steps(ctx, BOTH, 3, mode), phased(ctx, BOTH, 3))


@pytest.mark.gpu
def test_final_lr_edited_between_replays_takes_effect():
    """eager, record, replay; final_lr edited; two more captured steps (the second one a plain replay).  The result differs from
    the unedited run and equals a phased model given the same edit."""
    ctx = backends.gpu_ctx()
    edited = run_steps(ctx, BOTH, 5, "captured", edit=(3, 0.03))
    plain = run_steps(ctx, BOTH, 5, "captured")
    assert not torch.equal(plain[1][0], edited[1][0]) and not torch.equal(plain[1][3], edited[1][3])      # G's and D's weights
    assert plain[0][:3] == edited[0][:3]
    assert_same_run(edited, phased(ctx, BOTH, 5, edit=(3, 0.03)))


# ---- the Python surface --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_surface_trains_checkpoints_and_resumes(tmp_path):
    from swapnet_amd.models import create_model
    from swapnet_amd.optimizers import NativeAdaBound, NativeAdamW
    from tests.test_models_api import make_opt
    s = seeded_state()
    bodys, inputs, targets = s["batch"]
    data = dict(bodys=bodys, input_cloths=inputs, target_cloths=targets, cloth_paths=["c0", "c1"], body_paths=["b0", "b1"])

    def make(**kw):
        opt = make_opt(tmp_path, "gpu", optimizer_D="AdaBound", final_lr=0.05, **kw)
        model = create_model(opt)
        model.setup(opt)
        model.eval()
        return model

    model = make()
    assert isinstance(model.optimizer_D, NativeAdaBound) and not isinstance(model.optimizer_G, NativeAdaBound)
    assert isinstance(model.optimizer_G, NativeAdamW)
    model.net_generator.load_state_dict(s["G"])
    model.net_discriminator.load_state_dict(s["D"])
    group = model.optimizer_D.param_groups[0]
    assert {k: group[k] for k in ("lr", "betas", "final_lr", "gamma", "eps", "weight_decay", "amsbound")} == \
        dict(lr=4e-4, betas=(0.9, 0.999), final_lr=0.05, gamma=1e-3, eps=1e-8, weight_decay=0.01, amsbound=False)
    model.set_input(data)
    torch.manual_seed(11)
    model.optimize_parameters()
    assert all(np.isfinite(v) for v in model.get_current_losses().values())
    sd = model.optimizer_D.state_dict()
    names = list(s["D"].keys())
    assert list(sd["state"].keys()) == list(range(len(names)))
    for i, n in enumerate(names):
        st = sd["state"][i]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and type(st["step"]) is int and st["step"] == 1
        assert st["exp_avg"].shape == s["D"][n].shape and st["exp_avg_sq"].shape == s["D"][n].shape
    assert sd["param_groups"][0]["final_lr"] == 0.05 and sd["param_groups"][0]["params"] == list(range(len(names)))
    assert float(sd["state"][0]["exp_avg"].abs().max()) > 0

    # checkpoint and resume: a fresh model restored from the files continues bit-identically
    model.save_checkpoint("latest")
    m2 = make(continue_train=True)
    assert isinstance(m2.optimizer_D, NativeAdaBound) and m2.optimizer_D.state_dict()["state"][0]["step"] == 1
    for m in (model, m2):
        m.set_input(data)
        torch.manual_seed(7)
        m.optimize_parameters()
    assert model.get_current_losses() == m2.get_current_losses()
    for a, b in zip(model.net_discriminator.state_dict().values(), m2.net_discriminator.state_dict().values()):
        assert torch.equal(a, b)

    # halving lr halves the effective final_lr (base_lr stays the lr of construction): checked against the restatement
    model.optimizer_D.param_groups[0]["lr"] = 2e-4
    nm = model._native()
    nm.forward(False, 5)
    nm.backward_D(0.1, 0.9)
    before = {w: nm.state_dict(engine.NET_D, which=w, to_cpu=True) for w in (engine.W_WEIGHT, engine.W_GRAD, engine.W_EXP_AVG, engine.W_EXP_AVG_SQ)}
    model.optimizer_D.step()
    after = nm.state_dict(engine.NET_D, to_cpu=True)
    assert model.optimizer_D.state_dict()["state"][0]["step"] == 3
    moved_as_unhalved = 0
    for n in names:
        old = [before[w][n].flatten() for w in (engine.W_WEIGHT, engine.W_EXP_AVG, engine.W_EXP_AVG_SQ)]
        g = before[engine.W_GRAD][n].flatten()
        kw = dict(lr=f32(2e-4), b1=f32(0.9), b2=f32(0.999), eps=f32(EPS), wd=f32(0.01), final_lr=f32(0.05), gamma=f32(GAMMA), step=3)
        ref = adabound_f64(old[0], g, old[1], old[2], base_lr=f32(4e-4), **kw)
        got = f64(after[n].flatten())
        bar = 1e-5 * (f64(old[0]).abs() + (ref[0] - f64(old[0])).abs()) + 1e-7
        assert bool(((got - ref[0]).abs() <= bar).all()), n
        wrong = adabound_f64(old[0], g, old[1], old[2], base_lr=f32(2e-4), **kw)      # had base_lr followed the edit
        moved_as_unhalved += int(bool(((got - wrong[0]).abs() <= bar).all()))
    assert moved_as_unhalved < len(names), "the check cannot tell base_lr = 4e-4 from base_lr = 2e-4"

    # refused state dicts
    bad = model.optimizer_D.state_dict()
    bad["param_groups"][0]["amsbound"] = True
    with pytest.raises(NotImplementedError, match="amsbound"):
        model.optimizer_D.load_state_dict(bad)
    with pytest.raises(ValueError, match="final_lr"):
        model.optimizer_D.load_state_dict(model.optimizer_G.state_dict())
