"""BatchNorm2d + activation with a group dimension (swapnet_amd/csrc/batch_norm.hip) against torch.nn.BatchNorm2d in float64.

The reference of a call with `groups` runs is the float64 module applied to the runs ONE AFTER THE OTHER -- separate batch
statistics per run, the running buffers updated once per run in run order -- which is what the reference's discriminator does
with its fake and real passes and what one 2B batch with plain BatchNorm would silently get wrong.

Bars (the project's own): forward values, statistics and running buffers rel-L2 <= 1e-5; gradients rel-L2 <= 1e-4.  The gradient
bar needs every LeakyReLU to take the same branch in fp32 as in float64: the inputs are bimodal (|x| in [1, 1.3) with a random
sign, so the normalised values keep clear of zero while every channel still has elements on both branches) and every case asserts
on the float64 reference alone that no pre-activation lies within 1e-5 of the kink.
Every GPU test prints the figures it measured before it asserts (run with -s).  Measured on the MI355X, worst over the cases:
op y 5.0e-8, statistics 2.1e-8, running buffers 4.9e-8, dx 4.3e-8, d gamma 3.7e-8, d beta 4.5e-8; standalone discriminator
(predictions, running buffers) 2.5e-6; training steps: losses 2.6e-7, running buffers 6.0e-7, D gradients 6.0e-6 under batch
(torch fp32: 2.1e-6; ratio 2.8, bar max(1e-3, 2 x torch)), post-update D weights 1.7e-5 (torch 5.4e-6), G gradients 5.0e-3 at
step 0 (torch fp32 6.8e-3) and 6.3e-6 at step 1.
"""
import functools
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import swapnet_oracle as O
from swapnet_amd import _C, engine, modules
from swapnet_amd.modules import discriminators
from swapnet_amd.modules.native import NativeBackend
from tests import backends

EPS, MOMENTUM = 1e-5, 0.1
FWD_BAR, GRAD_BAR = 1e-5, 1e-4
ACT_NONE, ACT_LRELU = 0, 1

# (N, groups, H, W, C)
CASES = {
    "30rows": (4, 2, 5, 3, 128),          # 30 rows per group, nothing divides anything
    "odd31": (2, 1, 31, 31, 512),         # PatchGAN's odd map
    "narrow": (2, 2, 8, 8, 4),            # narrowest allocation; one image per group
    # 161 rows per image at C = 128: 8 rows of 32 float4 lanes per block, chunks of ceil(161 / 5) = 33 -> 40 rows (a whole
    # number of thread rows), so the image is 4 x 40 + 1: the last statistics block of every image sees ONE row
    "chunk+1": (2, 2, 7, 23, 128),
}
SEEDS = {"30rows": 0, "odd31": 0, "narrow": 0, "chunk+1": 0}


def plan_chunks(hw, n, c):
    """batch_norm.hip batch_norm_plan_chunks"""
    rows = max(1, 256 // (c // 4))
    nchunk = min(max(1, 1024 // n), max(1, hw // (rows * 4)), 256)
    chunk = -(-(-(-hw // nchunk)) // rows) * rows
    return -(-hw // chunk), chunk


def test_the_chunk_case_sits_one_row_above_a_multiple_of_the_chunk():
    n, _, h, w, c = CASES["chunk+1"]
    nchunk, chunk = plan_chunks(h * w, n, c)
    assert (nchunk, chunk) == (5, 40) and h * w == 4 * chunk + 1


def rel(a, b):
    return backends.rel_l2(a, b)


@functools.lru_cache(maxsize=None)
def case_data(name):
    n, groups, h, w, c = CASES[name]
    g = torch.Generator().manual_seed(1000 + SEEDS[name])
    sign = torch.randint(0, 2, (n, c, h, w), generator=g).double() * 2 - 1
    x = (sign * (1.0 + 0.3 * torch.rand(n, c, h, w, generator=g, dtype=torch.float64))).float()
    gamma = (0.5 + torch.rand(c, generator=g)).float()
    beta = ((torch.rand(c, generator=g) - 0.5) * 0.3).float() * gamma
    rm = torch.randn(c, generator=g).float() * 0.3
    rv = (0.5 + torch.rand(c, generator=g)).float()
    dy = torch.randn(n, c, h, w, generator=g).float()
    return dict(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, dy=dy)


@functools.lru_cache(maxsize=None)
def reference(name, groups, act, training=True):
    """float64 BatchNorm2d applied per group in order (+ LeakyReLU), with everything the op hands back."""
    d = case_data(name)
    c = d["x"].shape[1]
    bn = torch.nn.BatchNorm2d(c, eps=EPS, momentum=MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"]); bn.running_mean.copy_(d["rm"]); bn.running_var.copy_(d["rv"])
        bn.num_batches_tracked.fill_(7)
    bn.train(training)
    x = d["x"].double().requires_grad_(True)
    runs = x.chunk(groups)
    z = torch.cat([bn(r) for r in runs])
    y = F.leaky_relu(z, 0.2) if act == ACT_LRELU else z
    out = dict(y=y.detach(), min_abs_z=float(z.detach().abs().min()), rm=bn.running_mean.clone(), rv=bn.running_var.clone(),
               nbt=int(bn.num_batches_tracked))
    if training:
        stats = []
        for r in runs:
            r = r.detach()
            stats.append(torch.stack([r.mean((0, 2, 3)), 1.0 / torch.sqrt(r.var((0, 2, 3), unbiased=False) + EPS)], dim=1))
        out["stats"] = torch.stack(stats)
        out["dx"], out["dgamma"], out["dbeta"] = torch.autograd.grad(y, [x, bn.weight, bn.bias], d["dy"].double())
    return out


def op_fwd(ctx, name, groups, act, training=True):
    d = case_data(name)
    n, c, h, w = d["x"].shape
    dev = ctx.device
    x, gamma, beta = d["x"].to(dev), d["gamma"].to(dev), d["beta"].to(dev)
    rm, rv = d["rm"].to(dev).clone(), d["rv"].to(dev).clone()
    nbt = torch.full((1,), 7, dtype=torch.int64, device=dev)
    y = torch.empty_like(x)
    stats = torch.zeros(groups, c, 2, device=dev)
    ctx.lib.call("swn_op_batch_norm_act", ctx.handle, _C.ptr(x), n, c, h, w, groups, act, int(training), _C.ptr(gamma), _C.ptr(beta),
                 _C.ptr(rm), _C.ptr(rv), _C.ptr(nbt), _C.ptr(y), _C.ptr(stats))
    return dict(y=y.cpu(), stats=stats.cpu(), rm=rm.cpu(), rv=rv.cpu(), nbt=int(nbt.cpu()))


def op_bwd(ctx, name, groups, act, param_grads=True):
    d = case_data(name)
    n, c, h, w = d["x"].shape
    dev = ctx.device
    x, dy, gamma, beta = d["x"].to(dev), d["dy"].to(dev), d["gamma"].to(dev), d["beta"].to(dev)
    dx = torch.empty_like(x)
    dg, db = (torch.empty(c, device=dev), torch.empty(c, device=dev)) if param_grads else (None, None)
    ctx.lib.call("swn_op_batch_norm_act_bwd", ctx.handle, _C.ptr(x), _C.ptr(dy), n, c, h, w, groups, act, _C.ptr(gamma), _C.ptr(beta),
                 _C.ptr(dx), _C.ptr(dg), _C.ptr(db))
    return dict(dx=dx.cpu(), dgamma=None if dg is None else dg.cpu(), dbeta=None if db is None else db.cpu())


@pytest.mark.parametrize("act", [ACT_NONE, ACT_LRELU], ids=["none", "lrelu"])
@pytest.mark.parametrize("name", list(CASES))
def test_reference_preactivations_keep_clear_of_the_kink(name, act):
    """CPU: the float64 reference alone guarantees that no element can take the other LeakyReLU branch in fp32."""
    ref = reference(name, CASES[name][1], act)
    assert ref["min_abs_z"] >= 1e-5, (name, ref["min_abs_z"])


@pytest.mark.gpu
@pytest.mark.parametrize("act", [ACT_NONE, ACT_LRELU], ids=["none", "lrelu"])
@pytest.mark.parametrize("name", list(CASES))
def test_op_training_forward_and_backward_match_float64_per_group(name, act):
    ctx = backends.gpu_ctx()
    n, groups, h, w, c = CASES[name]
    ref = reference(name, groups, act)
    assert ref["min_abs_z"] >= 1e-5, (name, ref["min_abs_z"])
    got = op_fwd(ctx, name, groups, act)
    got.update(op_bwd(ctx, name, groups, act))
    errs = {k: rel(got[k], ref[k]) for k in ("y", "stats", "rm", "rv", "dx", "dgamma", "dbeta")}
    print("batch_norm op %s act %d: " % (name, act) + "  ".join("%s %.2e" % kv for kv in errs.items()))
    for k in ("y", "stats", "rm", "rv"):
        assert errs[k] <= FWD_BAR, (name, act, k, errs[k])
    for k in ("dx", "dgamma", "dbeta"):
        assert errs[k] <= GRAD_BAR, (name, act, k, errs[k])
    assert got["nbt"] == ref["nbt"] == 7 + groups
    if groups == 2:
        # the 2B-batching trap: the same batch under ONE set of statistics is a different function, by far more than the bar
        one = op_fwd(ctx, name, 1, act)
        one.update(op_bwd(ctx, name, 1, act))
        ref1 = reference(name, 1, act)
        for k in ("y", "rm", "dx"):
            assert rel(one[k], ref1[k]) <= (FWD_BAR if k != "dx" else GRAD_BAR), (name, act, k)
            assert rel(one[k], got[k]) > 100 * FWD_BAR, (name, act, k, rel(one[k], got[k]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["30rows", "odd31"])
def test_op_eval_mode_uses_the_running_buffers_and_leaves_them(name):
    ctx = backends.gpu_ctx()
    groups = CASES[name][1]
    d = case_data(name)
    ref = reference(name, groups, ACT_LRELU, training=False)
    got = op_fwd(ctx, name, groups, ACT_LRELU, training=False)
    e = rel(got["y"], ref["y"])
    print("batch_norm op eval %s: y %.2e" % (name, e))
    assert e <= FWD_BAR
    assert torch.equal(got["rm"], d["rm"]) and torch.equal(got["rv"], d["rv"]) and got["nbt"] == 7
    train = op_fwd(ctx, name, groups, ACT_LRELU)
    assert rel(train["y"], got["y"]) > 100 * FWD_BAR          # not the batch statistics


@pytest.mark.gpu
def test_op_is_deterministic_and_the_parameter_gradient_switch_leaves_dx_alone():
    ctx = backends.gpu_ctx()
    for name in ("30rows", "chunk+1"):
        groups = CASES[name][1]
        a, b = op_fwd(ctx, name, groups, ACT_LRELU), op_fwd(ctx, name, groups, ACT_LRELU)
        for k in ("y", "stats", "rm", "rv"):
            assert torch.equal(a[k], b[k]), (name, k)
        ga, gb = op_bwd(ctx, name, groups, ACT_LRELU), op_bwd(ctx, name, groups, ACT_LRELU)
        for k in ("dx", "dgamma", "dbeta"):
            assert torch.equal(ga[k], gb[k]), (name, k)
        assert torch.equal(op_bwd(ctx, name, groups, ACT_LRELU, param_grads=False)["dx"], ga["dx"])


@pytest.mark.gpu
def test_one_value_per_channel_is_refused_like_torch():
    ctx = backends.gpu_ctx()
    dev = ctx.device
    x, ones = torch.ones(1, 4, 1, 1, device=dev), torch.ones(4, device=dev)
    y = torch.empty_like(x)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ctx.lib.call("swn_op_batch_norm_act", ctx.handle, _C.ptr(x), 1, 4, 1, 1, 1, ACT_NONE, 1, _C.ptr(ones), _C.ptr(ones),
                     _C.ptr(ones.clone()), _C.ptr(ones.clone()), None, _C.ptr(y), None)
    with pytest.raises(ValueError):          # torch: "Expected more than 1 value per channel when training"
        torch.nn.BatchNorm2d(4)(torch.ones(1, 4, 1, 1))
    x2 = torch.ones(2, 4, 1, 1, device=dev)          # two groups of one image of one pixel: still one value per channel and run
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ctx.lib.call("swn_op_batch_norm_act", ctx.handle, _C.ptr(x2), 2, 4, 1, 1, 2, ACT_NONE, 1, _C.ptr(ones), _C.ptr(ones),
                     None, None, None, _C.ptr(torch.empty_like(x2)), None)


def test_the_host_simulator_refuses_batch_norm_by_name():
    """The simulator links the engine without batch_norm.hip: the op is the library's "not implemented" error, never a CPU path."""
    ctx = backends.hostsim_ctx()
    x, ones = torch.ones(2, 4, 2, 2), torch.ones(4)
    with pytest.raises(NotImplementedError, match="simulator"):
        ctx.lib.call("swn_op_batch_norm_act", ctx.handle, _C.ptr(x), 2, 4, 2, 2, 1, ACT_NONE, 1, _C.ptr(ones), _C.ptr(ones),
                     None, None, None, _C.ptr(torch.empty_like(x)), None)
    with pytest.raises(NotImplementedError, match="simulator"):
        ctx.lib.call("swn_op_batch_norm_act_bwd", ctx.handle, _C.ptr(x), _C.ptr(x.clone()), 2, 4, 2, 2, 1, ACT_NONE, _C.ptr(ones),
                     _C.ptr(ones), _C.ptr(torch.empty_like(x)), None, None)


# ---------------------------------------------------------------------------------------------------------------------
# The discriminator under --norm batch / none: standalone, seeded init, two training steps of the warp model, refusals
# ---------------------------------------------------------------------------------------------------------------------

D_IN, SIZE, BATCH = 22, 64, 2          # warp conditioning: 3 body + 19 cloth channels
D_KINDS = {"basic": ("basic", 3), "n1": ("n_layers", 1), "pixel": ("pixel", 3)}


def torch_norm(norm, c):
    if norm == "batch":
        return nn.BatchNorm2d(c, affine=True, track_running_stats=True)
    if norm == "instance":
        return nn.InstanceNorm2d(c, affine=False, track_running_stats=False)
    return nn.Identity()


class TorchPatchGAN(nn.Module):
    """The published pix2pix / CycleGAN NLayerDiscriminator (Isola et al. 2017; ndf 64, 4x4 kernels, LeakyReLU 0.2): convs in front
    of a norm layer carry a bias only under InstanceNorm."""

    def __init__(self, input_nc, n_layers, norm):
        super().__init__()
        use_bias = norm == "instance"
        seq = [nn.Conv2d(input_nc, 64, 4, 2, 1), nn.LeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            seq += [nn.Conv2d(64 * prev, 64 * mult, 4, 2, 1, bias=use_bias), torch_norm(norm, 64 * mult), nn.LeakyReLU(0.2, True)]
        prev, mult = mult, min(2 ** n_layers, 8)
        seq += [nn.Conv2d(64 * prev, 64 * mult, 4, 1, 1, bias=use_bias), torch_norm(norm, 64 * mult), nn.LeakyReLU(0.2, True)]
        seq += [nn.Conv2d(64 * mult, 1, 4, 1, 1)]
        self.model = nn.Sequential(*seq)

    def forward(self, x):
        return self.model(x)


class TorchPixelGAN(nn.Module):
    """The published 1x1 PixelDiscriminator: both convs behind the first take bias=use_bias."""

    def __init__(self, input_nc, norm):
        super().__init__()
        use_bias = norm == "instance"
        self.net = nn.Sequential(nn.Conv2d(input_nc, 64, 1), nn.LeakyReLU(0.2, True), nn.Conv2d(64, 128, 1, bias=use_bias),
                                 torch_norm(norm, 128), nn.LeakyReLU(0.2, True), nn.Conv2d(128, 1, 1, bias=use_bias))

    def forward(self, x):
        return self.net(x)


def torch_D(kind, norm):
    netD, n_layers = D_KINDS[kind]
    return TorchPixelGAN(D_IN, norm) if netD == "pixel" else TorchPatchGAN(D_IN, n_layers, norm)


def published_init(net, gain=0.02):
    """init_weights of pix2pix / CycleGAN, init_type normal: conv weights N(0, gain), biases 0, BatchNorm weights N(1, gain)."""
    def fn(m):
        if isinstance(m, nn.Conv2d):
            nn.init.normal_(m.weight.data, 0.0, gain)
            if m.bias is not None:
                nn.init.constant_(m.bias.data, 0.0)
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.normal_(m.weight.data, 1.0, gain)
            nn.init.constant_(m.bias.data, 0.0)
    net.apply(fn)
    return net


def native_D(ctx, kind, norm, batch=BATCH):
    netD, n_layers = D_KINDS[kind]
    backend = NativeBackend("warp", is_train=True, dropout=0.0, ctx=ctx, default_shape=(batch, SIZE, SIZE))
    return discriminators.define_D(D_IN, 64, netD, n_layers, norm, backend=backend), backend


def close_backend(backend):
    for m in backend.models.values():
        m.close()


def d_input(seed=5):
    bodys, _, targets = O.synth_warp_batch(BATCH, SIZE, SIZE, seed=seed)
    return torch.cat((bodys, targets), 1)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["batch", "none"])
@pytest.mark.parametrize("kind", list(D_KINDS))
def test_standalone_discriminator_matches_float64_and_keeps_the_torch_state_dict(kind, norm):
    ctx = backends.gpu_ctx()
    torch.manual_seed(11)
    ref = published_init(torch_D(kind, norm)).double()
    for m in ref.modules():
        if isinstance(m, nn.BatchNorm2d):                               # non-trivial affine and running state
            with torch.no_grad():
                m.bias.normal_(0.0, 0.1); m.running_mean.normal_(0.0, 0.1); m.running_var.uniform_(0.5, 1.5)
    sd = OrderedDict((k, v.clone().float() if v.is_floating_point() else v.clone()) for k, v in ref.state_dict().items())
    net, backend = native_D(ctx, kind, norm)
    try:
        net.load_state_dict(sd)
        back = net.state_dict()
        assert set(back) == set(sd)                                     # incl. num_batches_tracked; no inner conv bias
        assert not any(k in back for k in ("model.2.bias", "net.2.bias", "net.5.bias"))
        for k, v in sd.items():                                         # save -> load round trip is exact
            assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
        x = d_input()
        worst = 0.0
        for mode in (True, False):                                      # train (batch statistics + running update), then eval
            ref.train(mode); net.train(mode)
            with torch.no_grad():
                want = ref(x.double())
            got = net(x).cpu()
            assert got.shape == want.shape
            e = rel(got, want)
            worst = max(worst, e)
            assert e <= FWD_BAR, (kind, norm, "train" if mode else "eval", e)
            after, want_sd = net.state_dict(), ref.state_dict()
            for k in want_sd:
                if "running" in k:
                    eb = rel(after[k], want_sd[k])
                    worst = max(worst, eb)
                    assert eb <= FWD_BAR, (kind, norm, mode, k, eb)
                elif k.endswith("num_batches_tracked"):
                    assert int(after[k]) == int(want_sd[k]) == 1, (k, int(after[k]))
        print("standalone D %s %s: worst rel-L2 (predictions, running buffers) %.2e" % (kind, norm, worst))
        # a checkpoint of another norm kind is refused with the keys named
        other = torch_D(kind, "instance").state_dict()
        with pytest.raises(RuntimeError, match="bias"):
            net.load_state_dict(other)
    finally:
        close_backend(backend)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["batch", "none"])
@pytest.mark.parametrize("kind", list(D_KINDS))
def test_seeded_init_equals_the_published_rule(kind, norm):
    ctx = backends.gpu_ctx()
    torch.manual_seed(1234)
    want = published_init(torch_D(kind, norm)).state_dict()
    torch.manual_seed(1234)
    net, backend = native_D(ctx, kind, norm)
    try:
        modules.init_weights(net, "normal", 0.02)
        got = net.state_dict()
        assert set(got) == set(want)
        for k, v in want.items():
            assert torch.equal(got[k], v), k
        here = torch.rand(4)                                            # ... and the global RNG stands where torch's build leaves it
        torch.manual_seed(1234)
        published_init(torch_D(kind, norm))
        assert torch.equal(here, torch.rand(4))
    finally:
        close_backend(backend)


# ---- two training steps -------------------------------------------------------------------------------------------------
LABELS = (0.0, 1.0, 1.0)            # hard labels: fake, real (backward_D), real (backward_G)


def noise_bias_G(name):             # biases feeding an InstanceNorm of the generator: true gradient 0 (tests/test_warp_step.py)
    return name.endswith(".bias") and "resblocks" in name


@functools.lru_cache(maxsize=None)
def reference_steps(norm):
    """Two optimize_parameters steps of the warp model in torch fp32 and, from the same pre-step state, in float64: the oracle's
    differentiable generator and its step (oracle.swapnet_oracle.WarpStepOracle) composed with THIS file's discriminator -- the
    three discriminator calls of a step go through one torch module whose BatchNorm buffers update in place, call by call."""
    torch.manual_seed(3)
    G = O.warp_module_params()
    dref = published_init(torch_D("basic", norm))
    Dp = OrderedDict((k, v.detach().clone()) for k, v in dref.named_parameters())
    bufs = {torch.float32: OrderedDict((k, v.clone()) for k, v in dref.named_buffers())}
    batch = O.synth_warp_batch(BATCH, SIZE, SIZE, seed=1234)
    mods = {torch.float32: dref, torch.float64: torch_D("basic", norm).double()}

    def forward_in(dtype):
        def fwd(P, x, n_layers=None, taps=None):
            return torch.func.functional_call(mods[dtype].train(), {**P, **bufs[dtype]}, (x,))
        return fwd

    st = O.WarpStepOracle(G, Dp, training=False)
    steps = []
    saved = O.patchgan_forward
    try:
        for _ in range(2):
            s64 = st.astype(torch.float64)
            bufs[torch.float64] = OrderedDict((k, v.clone().double() if v.is_floating_point() else v.clone()) for k, v in bufs[torch.float32].items())
            pre = dict(G={k: v.clone() for k, v in st.G.items()}, D={k: v.clone() for k, v in st.D.items()},
                       bufs={k: v.clone() for k, v in bufs[torch.float32].items()},
                       mG={k: v.clone() for k, v in st.optG.m.items()}, vG={k: v.clone() for k, v in st.optG.v.items()},
                       mD={k: v.clone() for k, v in st.optD.m.items()}, vD={k: v.clone() for k, v in st.optD.v.items()})
            O.patchgan_forward = forward_in(torch.float32)
            st.step(*batch, labels=LABELS)
            O.patchgan_forward = forward_in(torch.float64)
            s64.step(*batch, labels=LABELS)
            steps.append(dict(pre=pre, loss32=dict(st.losses), loss64=dict(s64.losses),
                              gD32=dict(st.grads_D), gD64=dict(s64.grads_D), gG32=dict(st.grads_G), gG64=dict(s64.grads_G),
                              pD32={k: v.clone() for k, v in st.D.items()}, pD64={k: v.clone() for k, v in s64.D.items()},
                              bufs64={k: v.clone() for k, v in bufs[torch.float64].items()}))
    finally:
        O.patchgan_forward = saved
    return batch, steps


def load_state(m, pre, step_index):
    """The whole training state of the reference before a step: weights, buffers, both Adam moments, step counters (as
    tests/test_warp_step.py re-synchronises before its second step: Adam's first update is +-lr * sign(g))."""
    m.load_state_dict(engine.NET_G, pre["G"])
    m.load_state_dict(engine.NET_D, {**pre["D"], **pre["bufs"]})
    for net, mk, vk in ((engine.NET_G, "mG", "vG"), (engine.NET_D, "mD", "vD")):
        m.load_state_dict(net, pre[mk], which=engine.W_EXP_AVG)
        m.load_state_dict(net, pre[vk], which=engine.W_EXP_AVG_SQ)
        m.optim_step_count(net, step_index)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["batch", "none"])
def test_two_training_steps_of_the_warp_model_match_float64(norm):
    ctx = backends.gpu_ctx()
    batch, steps = reference_steps(norm)
    m = engine.NativeModel(ctx, "warp", BATCH, SIZE, SIZE, is_train=True, dropout=0.0, norm=norm)
    try:
        m.set_hyper()
        for i, t in enumerate(batch):
            m.set_input(i, t)
        for si, s in enumerate(steps):
            load_state(m, s["pre"], si)
            m.forward(False, 0)
            m.backward_D(LABELS[0], LABELS[1])
            gD = m.state_dict(engine.NET_D, which=engine.W_GRAD, to_cpu=True)
            m.optimizer_step(engine.NET_D)
            pD = m.state_dict(engine.NET_D, to_cpu=True)
            # backward_G from the float64 step's updated weights: Adam's update is +-lr * sign(g) at these step counts, so round-off
            # in near-zero gradient entries moves single weights by 2 lr whoever computes them (what torch's own fp32 step makes of
            # that on loss_G_gan is printed below).  The update itself is held by postD above.
            m.load_state_dict(engine.NET_D, {k: v.float() for k, v in s["pD64"].items()}, strict=False)
            m.backward_G(LABELS[2])
            gG = m.state_dict(engine.NET_G, which=engine.W_GRAD, to_cpu=True)
            m.optimizer_step(engine.NET_G)
            L = m.losses()
            after = m.state_dict(engine.NET_D, to_cpu=True)
            worst = {}
            for k in ("D_fake", "D_real", "G_gan"):
                worst[k] = abs(L[k] - s["loss64"][k]) / abs(s["loss64"][k])
            assert set(gD) == set(s["gD64"])                          # every D gradient, gamma and beta included
            wD = backends.assert_grads_vs_fp64(gD, s["gD32"], s["gD64"], lambda k: False, (norm, si, "gradD"))
            wP = backends.assert_grads_vs_fp64(pD, s["pD32"], s["pD64"], lambda k: False, (norm, si, "postD"))
            wG = backends.assert_grads_vs_fp64(gG, s["gG32"], s["gG64"], noise_bias_G, (norm, si, "gradG"))
            worst["buffers"] = 0.0
            if norm == "batch":
                # THREE sequential running updates: fake batch, real batch, then the fakes through the updated D
                for k, v in s["bufs64"].items():
                    if v.is_floating_point():
                        worst["buffers"] = max(worst["buffers"], rel(after[k], v))
                    else:
                        assert int(after[k]) == int(v) == 3 * (si + 1), (k, int(after[k]), int(v))
            print("warp step %d --norm %s: torch fp32's own loss_G_gan is %.2e from float64" % (
                si, norm, abs(s["loss32"]["G_gan"] - s["loss64"]["G_gan"]) / abs(s["loss64"]["G_gan"])))
            print("warp step %d --norm %s: losses D_fake %.2e D_real %.2e G_gan %.2e  buffers %.2e  gradD %.2e (torch fp32 %.2e)  "
                  "postD %.2e (%.2e)  gradG %.2e (%.2e)" % (si, norm, worst["D_fake"], worst["D_real"], worst["G_gan"], worst["buffers"],
                                                          wD[0], wD[1], wP[0], wP[1], wG[0], wG[1]))
            for k in ("D_fake", "D_real", "G_gan", "buffers"):
                assert worst[k] <= FWD_BAR, (norm, si, k, worst[k])
    finally:
        m.close()


@pytest.mark.gpu
def test_the_captured_step_is_bit_equal_to_the_eager_one_under_batch_norm():
    ctx = backends.gpu_ctx()
    batch, steps = reference_steps("batch")
    results = []
    for captured in (False, True):
        m = engine.NativeModel(ctx, "warp", BATCH, SIZE, SIZE, is_train=True, dropout=0.0, norm="batch")
        try:
            m.set_hyper()
            load_state(m, steps[0]["pre"], 0)
            for i, t in enumerate(batch):
                m.set_input(i, t)
            for si in range(3):                                       # captured: eager, record, replay
                m.step(LABELS, training=False, seed=si, captured=captured)
            ctx.sync()
            results.append((m.losses(), m.arena(engine.NET_D, engine.W_WEIGHT).clone(), m.arena(engine.NET_G, engine.W_WEIGHT).clone(),
                            {k: v.cpu() for k, v in m.state_dict(engine.NET_D).items() if "running" in k or "tracked" in k}))
        finally:
            m.close()
    (la, da, ga, ba), (lb, db, gb, bb) = results
    assert la == lb, (la, lb)
    assert torch.equal(da, db) and torch.equal(ga, gb)
    assert len(ba) == 9 and all(torch.equal(ba[k], bb[k]) for k in ba)          # three norm sites x (mean, var, counter)
    assert all(int(v) == 9 for k, v in ba.items() if k.endswith("num_batches_tracked"))


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _opt(tmp_path, **kw):
    from tests.test_models_api import make_opt
    return make_opt(tmp_path, "sim", **kw)


def test_texture_stage_and_gradient_penalties_refuse_a_non_instance_norm(tmp_path):
    from swapnet_amd.models import create_model
    with pytest.raises(NotImplementedError, match="texture"):
        create_model(_opt(tmp_path, model="texture", norm="batch"))
    with pytest.raises(NotImplementedError, match="gradient penalty"):
        create_model(_opt(tmp_path, gan_mode="wgan-gp", norm="batch"))
    with pytest.raises(NotImplementedError, match="gradient penalty"):
        create_model(_opt(tmp_path, gan_mode="dragan-lp", norm="none"))
    # the library refuses on its own too, whatever the Python layer checked
    ctx = backends.hostsim_ctx()
    with pytest.raises(NotImplementedError, match="texture"):
        engine.NativeModel(ctx, "texture", 1, 64, 64, is_train=True, norm="none")
    m = engine.NativeModel(ctx, "warp", 1, 64, 64, is_train=True, norm="none")
    try:
        with pytest.raises(NotImplementedError, match="norm"):
            m.set_hyper(gp_mode=1)
    finally:
        m.close()


def test_the_host_simulator_refuses_norm_batch_and_runs_norm_none(tmp_path):
    from swapnet_amd.models import create_model
    with pytest.raises(NotImplementedError, match="simulator"):
        create_model(_opt(tmp_path, norm="batch"))
    with pytest.raises(NotImplementedError, match="simulator"):
        engine.NativeModel(backends.hostsim_ctx(), "warp", 1, 64, 64, is_train=True, norm="batch")
    model = create_model(_opt(tmp_path, norm="none", batch_size=1))
    sd = model.net_discriminator.state_dict()
    assert "model.2.weight" in sd and "model.2.bias" not in sd and "model.0.bias" in sd and "model.11.bias" in sd
    assert not any("running" in k for k in sd)
    bodys, inputs, targets = O.synth_warp_batch(1, 64, 64, seed=5)
    model.set_input(dict(bodys=bodys, input_cloths=inputs, target_cloths=targets, cloth_paths=[""], body_paths=[""]))
    before = model.net_discriminator.state_dict()["model.5.weight"].clone()
    model.optimize_parameters()
    losses = model.get_current_losses()
    assert all(v == v and abs(v) < 1e6 for v in losses.values()), losses
    assert not torch.equal(model.net_discriminator.state_dict()["model.5.weight"], before)
