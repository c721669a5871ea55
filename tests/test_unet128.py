"""Texture stage under --netG unet_128: the plain pix2pix U-Net (Isola et al. 2017) with BatchNorm2d -- UnetGenerator(3, 3, num_downs 7,
ngf 64, BatchNorm2d, use_dropout=True) on the textures alone -- and the fused BatchNorm -> Dropout site it needs
(swapnet_amd/csrc/batch_norm.hip, swn_op_batch_norm_act_dropout), against float64.

The reference is this file's restatement of the published architecture: `TorchUnet128` (an nn.Module with the published state-dict
keys, for strict loading and the seeded init) and `unet128_forward`, the same network written functionally with F.batch_norm and
the oracle's _lrelu / _relu / _dropout, so that the oracle's replay scopes work; the running buffers live in a side dict outside
the parameter dict.  The skip tensor of every non-outermost block is LeakyReLU(x) (the in-place LeakyReLU of the published code).

Bars (the project's own): forward values, losses, statistics and running buffers rel-L2 <= 1e-5 against float64; gradients <= 1e-4
against float64 with the activation pattern pinned (O.PatternReplay of the native pass's export) and the dropout masks replayed
(O.MaskReplay of swn_model_dropout_mask's export).  Pinning is required: un-pinned, torch's own fp32 gradient is 2e-3 .. 5.5e-3 from
float64 on this network (a handful of sign flips out of 5 M elements); pinned it is <= 7.2e-6 and the forward 1.2e-6
(test_the_reference_alone_is_inside_the_bars_when_pinned measures it for the inputs used here).  replay.check() stays at its cap:
at most 1e-3 of the elements of a group may differ.

B = 1 at 128 x 128 trains: the deepest norm site (the innermost block's upnorm) sees the 2 x 2 output of the innermost transposed conv,
4 values per channel.  One value per channel -- what torch refuses -- is not reachable at the sizes the builder accepts: the only
1 x 1 map is the innermost down conv's output, and the innermost block has no downnorm.

Every GPU test prints what it measured before it asserts (run with -s).  Measured on the MI355X, worst over the cases:
fused op y 6.5e-8, dx 6.6e-8, d gamma 4.0e-8, d beta 2.8e-8 (kept share 0.494 .. 0.500); standalone generator train forward 7.0e-7,
eval forward 3.2e-7, running buffers 2.2e-7; training steps: losses 6.3e-7, generated batch 8.0e-7, running buffers 3.1e-7, pinned
gradients G 9.3e-6 (B = 1; 8.1e-6 at B = 2), D 4.6e-6, at most 4 replayed branches differing per group.  The reference alone, on
the same inputs (CPU, torch fp32 against float64, pinned): forward 1.1e-6, gradients G 9.3e-6, D 2.3e-6.
The discriminator's three inner conv biases feed an InstanceNorm (true gradient 0): they are left out of the relative comparison, as
in tests/test_texture_step.py; every other tensor of both networks is held to the bar.
"""
import functools
import warnings
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import swapnet_oracle as O
from swapnet_amd import engine, modules
from swapnet_amd.modules.native import NativeBackend
from tests import backends

FWD_BAR, GRAD_BAR = 1e-5, 1e-4
EPS, MOMENTUM = 1e-5, 0.1
DEPTH = 7
LABELS = (0.0, 1.0, 1.0)                            # hard labels: fake, real (backward_D), real (backward_G)
# tape positions + 1 of the two BatchNorm -> Dropout sites (blocks 5 and 4, in forward order): conv0, five (conv, norm) pairs, the
# innermost conv, then (convT, norm, relu) per block on the way up
DROP_SALTS = (17, 20)


def rel(a, b):
    return backends.rel_l2(a.detach(), b.detach())


def d_noise_bias(k):
    """The texture stage's PatchGAN runs under InstanceNorm: the biases of its three inner convs feed a norm layer, their true
    gradient is 0 and what any evaluation returns for them is round-off (as in tests/test_texture_step.py).  No relative distance
    exists for them; every other discriminator tensor, and every generator tensor, is compared."""
    return k in ("model.2.bias", "model.5.bias", "model.8.bias")


def prefix(d):
    return "model" + "".join(".model.1" if j == 0 else ".model.3" for j in range(d))


def expected_keys():
    """The 70 state-dict keys in torch's (module-tree) order."""
    def bn(p):
        return [p + s for s in (".weight", ".bias", ".running_mean", ".running_var", ".num_batches_tracked")]
    keys = [prefix(0) + ".model.0.weight"]
    for d in range(1, DEPTH - 1):
        keys += [prefix(d) + ".model.1.weight"] + bn(prefix(d) + ".model.2")
    keys += [prefix(DEPTH - 1) + ".model.1.weight", prefix(DEPTH - 1) + ".model.3.weight"] + bn(prefix(DEPTH - 1) + ".model.4")
    for d in range(DEPTH - 2, 0, -1):
        keys += [prefix(d) + ".model.5.weight"] + bn(prefix(d) + ".model.6")
    return keys + [prefix(0) + ".model.3.weight", prefix(0) + ".model.3.bias"]


class _Block(nn.Module):
    def __init__(self, outer, inner, sub=None, outermost=False, dropout=False):
        super().__init__()
        self.outermost = outermost
        down = nn.Conv2d(outer if not outermost else 3, inner, 4, 2, 1, bias=False)
        if outermost:
            seq = [down, sub, nn.ReLU(True), nn.ConvTranspose2d(inner * 2, 3, 4, 2, 1), nn.Tanh()]
        elif sub is None:
            seq = [nn.LeakyReLU(0.2, True), down, nn.ReLU(True), nn.ConvTranspose2d(inner, outer, 4, 2, 1, bias=False), nn.BatchNorm2d(outer)]
        else:
            seq = [nn.LeakyReLU(0.2, True), down, nn.BatchNorm2d(inner), sub, nn.ReLU(True),
                   nn.ConvTranspose2d(inner * 2, outer, 4, 2, 1, bias=False), nn.BatchNorm2d(outer)] + ([nn.Dropout(0.5)] if dropout else [])
        self.model = nn.Sequential(*seq)

    def forward(self, x):
        return self.model(x) if self.outermost else torch.cat([x, self.model(x)], 1)


class TorchUnet128(nn.Module):
    """The published U-Net generator with num_downs 7, ngf 64, BatchNorm2d, dropout: built from the innermost block outwards."""

    def __init__(self):
        super().__init__()
        b = _Block(512, 512)
        b = _Block(512, 512, b, dropout=True)
        b = _Block(512, 512, b, dropout=True)
        b = _Block(256, 512, b)
        b = _Block(128, 256, b)
        b = _Block(64, 128, b)
        self.model = _Block(3, 64, b, outermost=True)

    def forward(self, x):
        return self.model(x)


def published_init(net, init_type="normal", gain=0.02):
    """init_weights of pix2pix / CycleGAN: conv and transposed-conv weights by init_type, biases 0, BatchNorm weights N(1, gain)."""
    def fn(m):
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            if init_type == "normal":
                nn.init.normal_(m.weight.data, 0.0, gain)
            else:
                nn.init.kaiming_normal_(m.weight.data, a=0, mode="fan_in")
            if m.bias is not None:
                nn.init.constant_(m.bias.data, 0.0)
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.normal_(m.weight.data, 1.0, gain)
            nn.init.constant_(m.bias.data, 0.0)
    net.apply(fn)
    return net


def unet128_forward(P, bufs, x, training=False):
    """The same network functionally.  training: False (running buffers, nothing updated, no dropout), True (torch RNG dropout) or
    an O.MaskReplay.  In training mode `bufs` (running_mean / running_var / num_batches_tracked per site) is updated in place."""
    train = training is not False

    def bn(name, h):
        y = F.batch_norm(h, bufs[name + ".running_mean"], bufs[name + ".running_var"], P[name + ".weight"], P[name + ".bias"],
                         train, MOMENTUM, EPS)
        if train:
            bufs[name + ".num_batches_tracked"] += 1
        return y

    def block(d, x):
        p = prefix(d)
        if d == 0:
            h = F.conv2d(x, P[p + ".model.0.weight"], None, stride=2, padding=1)
            h = O._relu(block(1, h))
            return torch.tanh(F.conv_transpose2d(h, P[p + ".model.3.weight"], P[p + ".model.3.bias"], stride=2, padding=1))
        xl = O._lrelu(x)
        h = F.conv2d(xl, P[p + ".model.1.weight"], None, stride=2, padding=1)
        if d == DEPTH - 1:
            h = bn(p + ".model.4", F.conv_transpose2d(O._relu(h), P[p + ".model.3.weight"], None, stride=2, padding=1))
        else:
            h = O._relu(block(d + 1, bn(p + ".model.2", h)))
            h = bn(p + ".model.6", F.conv_transpose2d(h, P[p + ".model.5.weight"], None, stride=2, padding=1))
            if d in (4, 5):
                h = O._dropout(h, 0.5, training)
        return torch.cat([xl, h], 1)

    return block(0, x)


def split_state(sd, dtype):
    """torch state dict -> (parameters, buffers) in `dtype` (the counters stay int64)."""
    P = OrderedDict((k, v.clone().to(dtype)) for k, v in sd.items() if "running" not in k and "tracked" not in k)
    bufs = OrderedDict((k, v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items() if k not in P)
    return P, bufs


@functools.lru_cache(maxsize=None)
def seeded_state(seed=11):
    """Published init plus non-trivial beta and running buffers, as fp32 tensors."""
    torch.manual_seed(seed)
    net = published_init(TorchUnet128())
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.bias.normal_(0.0, 0.1); m.running_mean.normal_(0.0, 0.1); m.running_var.uniform_(0.5, 1.5)
    return OrderedDict((k, v.clone()) for k, v in net.state_dict().items())


# ---- the library's dropout stream, restated (hip_util.h drop_scale; Net::drop_seed): what swn_model_dropout_mask exports ----------
def _mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(11)


def drop_mask(seed, salt, n, c, h, w, p=0.5):
    """NCHW keep/scale factors of the site with `salt` under the step seed `seed`: element index ((n*H + y)*W + x)*C + c."""
    with np.errstate(over="ignore"):
        s = np.uint64(seed) * np.uint64(0x9E3779B1) + np.uint64(salt)
        idx = np.arange(n * h * w * c, dtype=np.uint64)
        bits = _mix64(s * np.uint64(0xD1342543DE82EF95) + idx) & np.uint64(0xFFFFFF)
    u = bits.astype(np.float32) * np.float32(1.0 / 16777216.0)
    m = np.where(u >= np.float32(p), np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0)).astype(np.float32)
    return torch.from_numpy(m.reshape(n, h, w, c)).permute(0, 3, 1, 2).contiguous()


def unet_masks(seed, B, H):
    """The two dropout sites in forward order: block 5 (512 channels at H / 32), block 4 (512 at H / 16)."""
    return [drop_mask(seed, DROP_SALTS[0], B, 512, H >> 5, H >> 5), drop_mask(seed, DROP_SALTS[1], B, 512, H >> 4, H >> 4)]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restated reference alone
# ---------------------------------------------------------------------------------------------------------------------
def test_the_restated_unet_has_the_70_published_keys_and_trains_at_batch_one():
    net = TorchUnet128()
    sd = net.state_dict()
    assert list(sd) == expected_keys() and len(sd) == 70
    assert sum(v.dim() == 4 for v in sd.values()) == 14 and sum(k.endswith("tracked") for k in sd) == 11
    assert len([k for k in sd if "running" in k or "tracked" in k]) == 33
    assert sorted(k for k in sd if k.endswith(".bias") and sd[k.replace(".bias", ".weight")].dim() == 4) == ["model.model.3.bias"]
    norm_c = [sd[k].numel() for k in sd if k.endswith("running_mean")]
    assert norm_c == [128, 256, 512, 512, 512, 512, 512, 512, 256, 128, 64]
    # B = 1 at 128 x 128: torch trains (the deepest norm site has 2 x 2 = 4 values per channel); the functional form agrees with it
    x = O.synth_texture_batch(1, 128, 128, seed=3)[0]
    sites = []
    hooks = [m.register_forward_hook(lambda m, i, o: sites.append(i[0].shape[0] * i[0].shape[2] * i[0].shape[3]))
             for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
    net.train()
    torch.manual_seed(4)
    want = net(x.clone())
    for h in hooks:
        h.remove()
    assert min(sites) == 4
    P, bufs = split_state(sd, torch.float32)
    for k in bufs:
        if k.endswith("running_var"):
            bufs[k].fill_(1.0)
        else:
            bufs[k].zero_()
    torch.manual_seed(4)
    got = unet128_forward(P, bufs, x, training=True)
    assert rel(got, want) < 1e-6
    after = net.state_dict()
    for k, v in bufs.items():
        assert torch.allclose(v.float(), after[k].float(), rtol=1e-5, atol=1e-7), k
    assert all(int(v) == 1 for k, v in bufs.items() if k.endswith("tracked"))
    # one value per channel is what torch refuses; the innermost 1 x 1 map has no norm, so no accepted size reaches it
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        nn.BatchNorm2d(4).train()(torch.ones(1, 4, 1, 1))


@functools.lru_cache(maxsize=None)
def step_case(B):
    """Weights, inputs and the seeded VGG16 of the training-step tests (B = 2: two steps; B = 1: one)."""
    sd = seeded_state(11)
    G, bufs = split_state(sd, torch.float32)
    torch.manual_seed(21)
    D = O.patchgan_params(22)
    vgg = O.vgg16_feature_params()
    batch = O.synth_texture_batch(B, 128, 128, seed=31 + B)
    return G, bufs, D, vgg, batch


class swapped_generator:
    """O.TextureStepOracle with the oracle's TextureModule forward swapped for this file's U-Net for the duration; the running
    buffers of the dtype being evaluated come from `bufs_by_dtype`."""

    def __init__(self, bufs_by_dtype):
        self.bufs = bufs_by_dtype

    def __enter__(self):
        self.saved = O.texture_module_forward
        bufs = self.bufs

        def fwd(P, input_tex, rois, cloth, num_roi=12, training=False, taps=None):
            return unet128_forward(P, bufs[input_tex.dtype], input_tex, training)
        O.texture_module_forward = fwd
        return self

    def __exit__(self, *exc):
        O.texture_module_forward = self.saved
        return False


STEP_SEEDS = (101, 102)


@pytest.mark.parametrize("B", [2, 1])
def test_the_reference_alone_is_inside_the_bars_when_pinned(B):
    """torch fp32 with its own pattern recorded, replayed in float64, on the inputs, seeds and masks of the GPU step tests: every
    gradient tensor within 1e-4, the forward within 1e-5 -- the bars measure the kernels, not the reference."""
    G, bufs, D, vgg, batch = step_case(B)
    masks = unet_masks(STEP_SEEDS[0], B, 128)
    b32 = OrderedDict((k, v.clone()) for k, v in bufs.items())
    b64 = OrderedDict((k, v.clone().double() if v.is_floating_point() else v.clone()) for k, v in bufs.items())
    with swapped_generator({torch.float32: b32, torch.float64: b64}):
        s32 = O.TextureStepOracle(G, D, vgg, training=O.MaskReplay(masks))
        rec = O.PatternReplay()
        s32.patterns = rec
        s32.step(*batch, labels=list(LABELS))
        s64 = O.TextureStepOracle(G, D, vgg, training=O.MaskReplay(masks), dtype=torch.float64)
        s64.patterns = O.PatternReplay(rec.groups)
        s64.step(*batch, labels=list(LABELS))
    flips = s64.patterns.check()
    fwd = rel(s32.fakes, s64.fakes)
    wG = max(rel(s32.grads_G[k], v) for k, v in s64.grads_G.items())
    wD = max(rel(s32.grads_D[k], v) for k, v in s64.grads_D.items() if not d_noise_bias(k))
    wB = max(rel(b32[k], v) for k, v in b64.items() if v.is_floating_point())
    print("reference alone, B = %d: flips %s  forward %.2e  buffers %.2e  worst gradient G %.2e D %.2e" % (B, flips, fwd, wB, wG, wD))
    assert fwd <= FWD_BAR and wB <= FWD_BAR and wG <= GRAD_BAR and wD <= GRAD_BAR


def _opt(tmp_path, backend, **kw):
    from tests.test_models_api import make_opt
    return make_opt(tmp_path, backend, model="texture", netG="unet_128", crop_size=128, **kw)


def test_the_host_simulator_refuses_unet_128_by_name(tmp_path):
    from swapnet_amd.models import create_model
    with pytest.raises(NotImplementedError, match="simulator"):
        create_model(_opt(tmp_path, "sim"))
    with pytest.raises(NotImplementedError, match="simulator"):
        engine.NativeModel(backends.hostsim_ctx(), "texture", 1, 128, 128, is_train=True, netG="unet_128")
    # ... behind the texture stage's own refusal of a non-instance --norm, whose message is unchanged
    with pytest.raises(NotImplementedError, match="texture"):
        create_model(_opt(tmp_path, "sim", norm="batch"))
    from swapnet_amd.modules.pix2pix_modules import UnetGenerator
    for args in ((3, 3, 8, 64, "batch", True), (3, 3, 7, 64, "instance", True), (3, 3, 7, 64, "batch", False), (4, 3, 7, 64, "batch", True)):
        with pytest.raises(NotImplementedError):
            UnetGenerator(*args)


def test_construction_order_of_the_bare_unet_is_innermost_block_first():
    keys = [k.rsplit(".", 1)[0] for k in expected_keys() if k.endswith(".weight")]
    order = [k for k in modules._construction_order(OrderedDict((k, {}) for k in keys))]
    convs = [k for k in order if not k.endswith((".model.2", ".model.6", ".model.4"))]
    assert convs[:2] == [prefix(6) + ".model.1", prefix(6) + ".model.3"] and convs[-2:] == [prefix(0) + ".model.0", prefix(0) + ".model.3"]
    assert convs[2:4] == [prefix(5) + ".model.1", prefix(5) + ".model.5"]
    # the discriminator's flat `model.K` names are left in state-dict order
    flat = OrderedDict((k, {}) for k in ("model.0", "model.2", "model.3", "model.5"))
    assert modules._construction_order(flat) == list(flat)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the fused op
# ---------------------------------------------------------------------------------------------------------------------
OP_SHAPES = {"deepest_b2": (2, 512, 2, 2), "deepest_b1": (1, 512, 2, 2), "4x4": (2, 512, 4, 4), "chunk+1": (2, 128, 7, 23)}


@functools.lru_cache(maxsize=None)
def op_data(name):
    n, c, h, w = OP_SHAPES[name]
    g = torch.Generator().manual_seed(2000 + len(name))
    x = torch.randn(n, c, h, w, generator=g)
    gamma = 0.5 + torch.rand(c, generator=g)
    beta = (torch.rand(c, generator=g) - 0.5) * 0.3
    dy = torch.randn(n, c, h, w, generator=g)
    return x, gamma, beta, dy


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OP_SHAPES))
def test_op_batch_norm_dropout_matches_float64_times_the_exported_mask(name):
    ctx = backends.gpu_ctx()
    x, gamma, beta, dy = op_data(name)
    n, c, h, w = x.shape
    y, mask, dx, dg, db = (t.cpu() for t in engine.op_batch_norm_act_dropout(ctx, x, gamma, beta, dy=dy, act=0, p=0.5, seed=7))
    assert set(mask.unique().tolist()) <= {0.0, 2.0}
    assert torch.equal(mask, drop_mask(7, 1, n, c, h, w))                # the export is the one definition; this file restates it
    kept = float((mask != 0).float().mean())
    bn = nn.BatchNorm2d(c, eps=EPS, momentum=MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    xd = x.double().requires_grad_(True)
    want = bn(xd) * mask.double()
    wdx, wdg, wdb = torch.autograd.grad(want, [xd, bn.weight, bn.bias], dy.double())
    errs = dict(y=rel(y, want.detach()), dx=rel(dx, wdx), dgamma=rel(dg, wdg), dbeta=rel(db, wdb))
    print("batch_norm + dropout op %s: kept %.3f  " % (name, kept) + "  ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs["y"] <= FWD_BAR
    for k in ("dx", "dgamma", "dbeta"):
        assert errs[k] <= GRAD_BAR, (name, k, errs[k])
    if name in ("4x4", "chunk+1"):
        assert 0.4 <= kept <= 0.6, kept
    assert bool((y[mask == 0] == 0).all()) and bool((dx.abs().sum() > 0))
    # deterministic per seed; another seed draws another mask
    again = [t.cpu() for t in engine.op_batch_norm_act_dropout(ctx, x, gamma, beta, dy=dy, act=0, p=0.5, seed=7)]
    for a, b in zip((y, mask, dx, dg, db), again):
        assert torch.equal(a, b)
    other = engine.op_batch_norm_act_dropout(ctx, x, gamma, beta, dy=dy, act=0, p=0.5, seed=8)
    assert not torch.equal(other[1].cpu(), mask) and not torch.equal(other[0].cpu(), y)


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1], ids=["none", "lrelu"])
def test_op_without_dropout_is_bit_identical_to_the_plain_batch_norm_op(act):
    """p = 0 launches the kernels swn_op_batch_norm_act / _bwd launch; with an activation on, the bimodal inputs of
    tests/test_batch_norm.py."""
    from tests import test_batch_norm as TBN
    ctx = backends.gpu_ctx()
    for name in ("chunk+1", "odd31"):
        d = TBN.case_data(name)
        fwd, bwd = TBN.op_fwd(ctx, name, 1, act), TBN.op_bwd(ctx, name, 1, act)
        y, mask, dx, dg, db = engine.op_batch_norm_act_dropout(ctx, d["x"], d["gamma"], d["beta"], dy=d["dy"], act=act, p=0.0, seed=3)
        assert mask is None
        assert torch.equal(y.cpu(), fwd["y"]) and torch.equal(dx.cpu(), bwd["dx"])
        assert torch.equal(dg.cpu(), bwd["dgamma"]) and torch.equal(db.cpu(), bwd["dbeta"])
        # with the mask on and an activation: the float64 module, LeakyReLU, then the mask
        y, mask, dx, dg, db = (t.cpu() for t in engine.op_batch_norm_act_dropout(ctx, d["x"], d["gamma"], d["beta"], dy=d["dy"], act=act, p=0.5, seed=5))
        c = d["x"].shape[1]
        bn = nn.BatchNorm2d(c, eps=EPS, momentum=MOMENTUM).double().train()
        with torch.no_grad():
            bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"])
        xd = d["x"].double().requires_grad_(True)
        z = bn(xd)
        assert float(z.detach().abs().min()) >= 1e-5
        want = (F.leaky_relu(z, 0.2) if act else z) * mask.double()
        wdx, wdg, wdb = torch.autograd.grad(want, [xd, bn.weight, bn.bias], d["dy"].double())
        errs = dict(y=rel(y, want.detach()), dx=rel(dx, wdx), dgamma=rel(dg, wdg), dbeta=rel(db, wdb))
        print("batch_norm + act %d + dropout op %s: " % (act, name) + "  ".join("%s %.2e" % kv for kv in errs.items()))
        assert errs["y"] <= FWD_BAR and max(errs["dx"], errs["dgamma"], errs["dbeta"]) <= GRAD_BAR, errs


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the generator standalone, seeded init
# ---------------------------------------------------------------------------------------------------------------------
def native_unet(ctx, B, H, is_train=False):
    from swapnet_amd.modules.pix2pix_modules import UnetGenerator
    backend = NativeBackend("texture", is_train=is_train, ctx=ctx, default_shape=(B, H, H))
    return UnetGenerator(3, 3, 7, 64, norm_layer=nn.BatchNorm2d, use_dropout=True, backend=backend), backend


def close_backend(backend):
    for m in backend.models.values():
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B,H", [(2, 128), (1, 256)])
def test_standalone_generator_matches_float64_and_keeps_the_torch_state_dict(B, H):
    ctx = backends.gpu_ctx()
    sd = seeded_state(11)
    net, backend = native_unet(ctx, B, H)
    try:
        net.load_state_dict(sd)
        back = net.state_dict()
        assert list(back) == expected_keys()                             # 70 keys, no key for any bias that does not exist
        for k, v in sd.items():                                          # save -> load round trip is exact, int64 counters included
            assert back[k].dtype == v.dtype and back[k].shape == v.shape and torch.equal(back[k], v), k
        TorchUnet128().load_state_dict(back, strict=True)                # the published module takes the native state dict
        x = O.synth_texture_batch(B, H, H, seed=5)[0]
        P, bufs = split_state(sd, torch.float64)
        # train mode: batch statistics, one running update, dropout -- the masks of the seed the module draws, replayed
        torch.manual_seed(77)
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)))
        torch.manual_seed(77)
        net.train()
        got = net(x).cpu()
        m = backend.cur
        masks = [t.cpu() for t, _ in m.dropout_masks(engine.NET_G, seed=seed)]
        assert [tuple(t.shape) for t in masks] == [(B, 512, H >> 5, H >> 5), (B, 512, H >> 4, H >> 4)]
        for t, want in zip(masks, unet_masks(seed, B, H)):
            assert torch.equal(t, want)
        with torch.no_grad():
            want = unet128_forward(P, bufs, x.double(), training=O.MaskReplay(masks))
        e_train = rel(got, want)
        after = net.state_dict()
        e_buf = max(rel(after[k], v) for k, v in bufs.items() if v.is_floating_point())
        print("standalone unet_128 B %d %d x %d: train forward %.2e  running buffers %.2e" % (B, H, H, e_train, e_buf))
        assert e_train <= FWD_BAR and e_buf <= FWD_BAR
        assert all(int(after[k]) == int(v) == 1 for k, v in bufs.items() if not v.is_floating_point())
        # eval mode: the running buffers (as the train pass left them), nothing updated, no dropout
        net.eval()
        got = net(x).cpu()
        with torch.no_grad():
            want = unet128_forward(P, bufs, x.double(), training=False)
        e_eval = rel(got, want)
        print("standalone unet_128 B %d %d x %d: eval forward %.2e" % (B, H, H, e_eval))
        assert e_eval <= FWD_BAR
        final = net.state_dict()
        for k in bufs:
            assert torch.equal(final[k], after[k]), k
        # a TextureModule checkpoint (--netG swapnet) is refused with the keys named
        torch.manual_seed(1)
        with pytest.raises(RuntimeError, match="unet.model"):
            net.load_state_dict(O.texture_module_params(img_size=128))
    finally:
        close_backend(backend)


@pytest.mark.gpu
def test_sizes_other_than_128_and_256_are_refused():
    ctx = backends.gpu_ctx()
    with pytest.raises(ValueError, match="128 or 256"):
        engine.NativeModel(ctx, "texture", 1, 64, 64, is_train=False, netG="unet_128")
    with pytest.raises(ValueError, match="128 or 256"):
        engine.NativeModel(ctx, "texture", 1, 256, 128, is_train=False, netG="unet_128")


@pytest.mark.gpu
@pytest.mark.parametrize("init_type", ["normal", "kaiming"])
def test_seeded_init_equals_the_published_rule(init_type):
    ctx = backends.gpu_ctx()
    torch.manual_seed(1234)
    want = published_init(TorchUnet128(), init_type).state_dict()
    torch.manual_seed(1234)
    net, backend = native_unet(ctx, 1, 128)
    try:
        modules.init_weights(net, init_type, 0.02)
        got = net.state_dict()
        assert list(got) == list(want)
        for k, v in want.items():
            assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
        here = torch.rand(4)                                             # ... and the global RNG stands where torch's build leaves it
        torch.manual_seed(1234)
        published_init(TorchUnet128(), init_type)
        assert torch.equal(here, torch.rand(4))
    finally:
        close_backend(backend)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: training steps
# ---------------------------------------------------------------------------------------------------------------------
def vgg_state_dict(model, vgg):
    names = list(model.param_infos(engine.NET_VGG).keys())
    return {names[2 * i + j]: t for i, wb in enumerate(vgg) for j, t in enumerate(wb)}


def load_training_state(m, st, bufs, step_index):
    """The oracle's whole training state into the native model: weights, buffers, both Adam moments, step counters."""
    f32 = lambda d: {k: v.float() if v.is_floating_point() else v for k, v in d.items()}
    m.load_state_dict(engine.NET_G, {**f32(st.G), **f32(bufs)})
    m.load_state_dict(engine.NET_D, f32(st.D))
    for net, opt in ((engine.NET_G, st.optG), (engine.NET_D, st.optD)):
        m.load_state_dict(net, f32(opt.m), which=engine.W_EXP_AVG)
        m.load_state_dict(net, f32(opt.v), which=engine.W_EXP_AVG_SQ)
        m.optim_step_count(net, step_index)


def run_pinned_steps(ctx, B, nsteps):
    G, bufs0, D, vgg, batch = step_case(B)
    b64 = OrderedDict((k, v.clone().double() if v.is_floating_point() else v.clone()) for k, v in bufs0.items())
    s64 = O.TextureStepOracle(G, D, vgg, dtype=torch.float64)
    m = engine.NativeModel(ctx, "texture", B, 128, 128, is_train=True, netG="unet_128")
    worst = dict(loss=0.0, gradG=0.0, gradD=0.0, buffers=0.0, fakes=0.0)
    try:
        assert list(m.param_infos(engine.NET_G)) == list(G) and len(m.buffer_infos(engine.NET_G)) == 33
        m.load_state_dict(engine.NET_VGG, vgg_state_dict(m, vgg))
        m.set_hyper()
        for i, t in enumerate(batch):
            m.set_input(i, t)
        for si in range(nsteps):
            load_training_state(m, s64, b64, si)                         # (before the second step: the oracle's state after the first)
            seed = STEP_SEEDS[si]
            masks = [t.cpu() for t, _ in m.dropout_masks(engine.NET_G, seed=seed)]
            for t, want in zip(masks, unet_masks(seed, B, 128)):
                assert torch.equal(t, want)
            m.forward(True, seed)
            m.backward_D(LABELS[0], LABELS[1])
            gD = m.state_dict(engine.NET_D, which=engine.W_GRAD, to_cpu=True)
            m.optimizer_step(engine.NET_D)
            m.backward_G(LABELS[2])
            gG = m.state_dict(engine.NET_G, which=engine.W_GRAD, to_cpu=True)
            m.optimizer_step(engine.NET_G)
            replay = O.PatternReplay(backends.collect_patterns(m, vgg=True))
            s64.training, s64.patterns = O.MaskReplay(masks), replay
            with swapped_generator({torch.float64: b64}):
                s64.step(*batch, labels=list(LABELS))
            flips = replay.check()
            L, after = m.losses(), m.state_dict(engine.NET_G, to_cpu=True)
            e_loss = max(abs(L[k] - v) / abs(v) for k, v in s64.losses.items())
            e_buf = max(rel(after[k], v) for k, v in b64.items() if v.is_floating_point())
            e_out = rel(m.output(), s64.fakes)
            print("unet_128 step %d B %d: flips %s  losses %.2e  fakes %.2e  running buffers %.2e" % (si, B, flips, e_loss, e_out, e_buf))
            assert set(gG) == set(s64.grads_G) and set(gD) == set(s64.grads_D)      # every gradient, gamma and beta included
            wG = backends.assert_grads_replayed(gG, s64.grads_G, lambda k: False, GRAD_BAR, ("unet_128", B, si, "G"))
            wD = backends.assert_grads_replayed(gD, s64.grads_D, d_noise_bias, GRAD_BAR, ("unet_128", B, si, "D"))
            print("unet_128 step %d B %d: worst pinned gradient G %.2e D %.2e" % (si, B, wG, wD))
            assert e_loss <= FWD_BAR and e_buf <= FWD_BAR and e_out <= FWD_BAR, (si, e_loss, e_buf, e_out)
            assert all(int(after[k]) == int(v) == si + 1 for k, v in b64.items() if not v.is_floating_point())
            for k, v in dict(loss=e_loss, gradG=wG, gradD=wD, buffers=e_buf, fakes=e_out).items():
                worst[k] = max(worst[k], v)
    finally:
        m.close()
    return worst


@pytest.mark.gpu
def test_two_training_steps_match_float64_with_pattern_and_masks_replayed():
    print("unet_128 B 2, two steps:", {k: "%.2e" % v for k, v in run_pinned_steps(backends.gpu_ctx(), 2, 2).items()})


@pytest.mark.gpu
def test_one_training_step_at_batch_one_matches_float64():
    print("unet_128 B 1, one step:", {k: "%.2e" % v for k, v in run_pinned_steps(backends.gpu_ctx(), 1, 1).items()})


def fresh_step_model(ctx, B):
    G, bufs, D, vgg, batch = step_case(B)
    m = engine.NativeModel(ctx, "texture", B, 128, 128, is_train=True, netG="unet_128")
    backends.reset_state(m, {engine.NET_G: {**G, **bufs}, engine.NET_D: D})
    m.load_state_dict(engine.NET_VGG, vgg_state_dict(m, vgg))
    for i, t in enumerate(batch):
        m.set_input(i, t)
    return m


@pytest.mark.gpu
def test_the_captured_step_is_bit_equal_to_the_eager_one():
    ctx = backends.gpu_ctx()
    results = []
    for captured in (False, True):
        m = fresh_step_model(ctx, 2)
        try:
            for si in range(3):                                           # captured: eager, record, replay
                m.step(LABELS, training=True, seed=40 + si, captured=captured)
            ctx.sync()
            results.append((m.losses(), m.arena(engine.NET_D, engine.W_WEIGHT).clone(), m.arena(engine.NET_G, engine.W_WEIGHT).clone(),
                            {k: v.cpu() for k, v in m.state_dict(engine.NET_G).items() if "running" in k or "tracked" in k}))
        finally:
            m.close()
    (la, da, ga, ba), (lb, db, gb, bb) = results
    assert la == lb, (la, lb)
    assert torch.equal(da, db) and torch.equal(ga, gb)
    assert len(ba) == 33 and all(torch.equal(ba[k], bb[k]) for k in ba)
    assert all(int(v) == 3 for k, v in ba.items() if k.endswith("num_batches_tracked"))


@pytest.mark.gpu
def test_a_model_of_a_second_batch_size_shares_the_running_buffers():
    ctx = backends.gpu_ctx()
    m = fresh_step_model(ctx, 2)
    m1 = None
    try:
        m.step(LABELS, training=True, seed=9)
        m1 = engine.NativeModel(ctx, "texture", 1, 128, 128, share=m)
        assert m1.netG == "unet_128"
        key = prefix(3) + ".model.6.running_mean"
        a = m.get_buffer(engine.NET_G, key, (256,), torch.float32).cpu()
        assert torch.equal(m1.get_buffer(engine.NET_G, key, (256,), torch.float32).cpu(), a) and float(a.abs().sum()) > 0
        m1.set_input(0, step_case(1)[4][0])
        m1.forward(True, 10)                                              # a training-mode forward of the sharer updates the one set
        b = m.get_buffer(engine.NET_G, key, (256,), torch.float32).cpu()
        assert not torch.equal(a, b) and torch.equal(m1.get_buffer(engine.NET_G, key, (256,), torch.float32).cpu(), b)
        cnt = prefix(3) + ".model.6.num_batches_tracked"
        assert int(m.get_buffer(engine.NET_G, cnt, (), torch.int64)) == int(m1.get_buffer(engine.NET_G, cnt, (), torch.int64)) == 2
        m1.forward(False, 0)                                              # eval: nothing moves
        assert torch.equal(m.get_buffer(engine.NET_G, key, (256,), torch.float32).cpu(), b)
    finally:
        if m1 is not None:
            m1.close()
        m.close()


@pytest.mark.gpu
def test_pipeline_refuses_a_unet_128_texture_model():
    ctx = backends.gpu_ctx()
    w = engine.NativeModel(ctx, "warp", 1, 128, 128, is_train=False)
    t = engine.NativeModel(ctx, "texture", 1, 128, 128, is_train=False, netG="unet_128")
    try:
        with pytest.raises(NotImplementedError, match="unet_128"):
            engine.NativePipeline(w, t)
    finally:
        t.close(); w.close()


def compact_batch(B=2, Hs=128):
    g = np.random.RandomState(5)
    sample = np.zeros((B, 5), dtype=np.float32)
    for b in range(B):
        sample[b] = (b % 2, 1, 1.0, Hs // 2, Hs // 2)
    rois = np.sort(g.randint(0, Hs, (B, 12, 2, 2)), axis=2).reshape(B, 12, 4).astype(np.float32)
    return {"textures_u8": torch.from_numpy(g.randint(0, 256, (B, Hs, Hs, 3)).astype(np.uint8)),
            "cloth_labels_u8": torch.from_numpy(g.randint(0, 19, (B, 16, 16)).repeat(4, 1).repeat(4, 2).astype(np.uint8)),
            "rois_raw": torch.from_numpy(rois), "sample_params": torch.from_numpy(sample), "crop": (0, 0, Hs, Hs),
            "norm_stats": ((0.5,) * 3, (0.5,) * 3), "cloth_paths": ["c%d" % b for b in range(B)], "texture_paths": ["t%d" % b for b in range(B)]}


@pytest.mark.gpu
def test_create_model_trains_saves_and_tests_with_netG_unet_128(tmp_path):
    from swapnet_amd.models import create_model
    from swapnet_amd.modules.pix2pix_modules import UnetGenerator
    opt = _opt(tmp_path, "gpu", init_type="normal")
    torch.manual_seed(1234)
    want = published_init(TorchUnet128()).state_dict()
    torch.manual_seed(1234)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                   # (seeded-random VGG16 where no pretrained weights are at hand)
        model = create_model(opt)
    model.setup(opt)
    assert isinstance(model.net_generator, UnetGenerator)
    start = model.net_generator.state_dict()
    assert list(start) == expected_keys()
    for k, v in want.items():                                             # torch.manual_seed(s); create_model(opt) starts from torch's weights
        assert torch.equal(start[k], v), k
    tex, rois, cloths, tgt = O.synth_texture_batch(2, 128, 128, seed=8)
    data = dict(input_textures=tex, rois=rois, cloths=cloths, target_textures=tgt, cloth_paths=["c0", "c1"], texture_paths=["t0", "t1"])
    for batch in (data, compact_batch()):                                 # the float batch, then the compact uint8 one
        model.set_input(batch)
        model.optimize_parameters()
        losses = model.get_current_losses()
        assert losses and all(np.isfinite(v) for v in losses.values()), losses
    assert model.fakes.shape == (2, 3, 128, 128)
    sd = model.net_generator.state_dict()
    moved = prefix(2) + ".model.1.weight"
    assert not torch.equal(sd[moved], start[moved]) and not torch.equal(sd[prefix(2) + ".model.6.weight"], start[prefix(2) + ".model.6.weight"])
    assert all(int(v) == 2 for k, v in sd.items() if k.endswith("tracked"))
    assert all(not torch.equal(v, start[k]) for k, v in sd.items() if "running" in k)
    # checkpoint round trip through the reference's file names
    model.save_checkpoint("latest")
    opt2 = _opt(tmp_path, "gpu", init_type="normal", continue_train=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m2 = create_model(opt2)
    m2.setup(opt2)
    sd2 = m2.net_generator.state_dict()
    assert list(sd2) == list(sd)
    for k, v in sd.items():
        assert sd2[k].dtype == v.dtype and torch.equal(sd2[k], v), k
    # eval + test(): the running buffers, untouched
    model.eval()
    model.set_input(data)
    model.test()
    assert bool(torch.isfinite(model.fakes).all())
    after = model.net_generator.state_dict()
    for k, v in sd.items():
        if "running" in k or "tracked" in k:
            assert torch.equal(after[k], v), k
