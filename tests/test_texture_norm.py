"""The texture stage under --norm batch and --norm none (device library): the TextureModule's pix2pix U-Net and the stage's PatchGAN
take the flag's norm layer; `encode` = UNetDown(36, 36) keeps its InstanceNorm.

Reference: a torch module restated here from the published pix2pix block structure (Isola et al. 2017), as
tests/test_unet128.py::TorchUnet128 is -- blocks [LeakyReLU, conv, norm, sub-block, ReLU, convT, norm, (Dropout)], built from the
innermost block outwards, use_bias false under BatchNorm2d / Identity except the outermost ConvTranspose2d -- behind the RoIAlign +
encode front of oracle.swapnet_oracle; and the same network in functional form (texture_forward), whose activations and dropout go
through the oracle's replay hooks so a training step can be pinned: the activation pattern and the dropout masks of the native step
are replayed in float64 (tests/test_unet128.py::run_pinned_steps).  The discriminator is tests/test_batch_norm.py's TorchPatchGAN,
restated functionally for the same reason.

Bars: forward, losses and running buffers 1e-5, pinned gradients 1e-4 (the project's pinned bars).  Under batch / none the
PatchGAN's inner convs have no bias, so no discriminator tensor is left out of the comparison.
"""
import functools
import math
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
from tests.test_batch_norm import TorchPatchGAN
from tests.test_unet128 import (EPS, FWD_BAR, GRAD_BAR, LABELS, MOMENTUM, close_backend, compact_batch, published_init, rel, split_state,
                                vgg_state_dict)

NORMS = ["batch", "none"]
RC, CC = 36, 19                                     # ROI-pooled texture channels (12 rois x 3), cloth channels
STEP_SEEDS = (101, 102)


def depth_of(size):
    return int(math.log2(size))


def prefix(d):
    return "unet.model" + "".join(".model.1" if j == 0 else ".model.3" for j in range(d))


def torch_norm(norm, c):
    return nn.BatchNorm2d(c) if norm == "batch" else nn.Identity()


class _Block(nn.Module):
    def __init__(self, norm, outer, inner, sub=None, outermost=False, dropout=False, input_nc=None):
        super().__init__()
        self.outermost = outermost
        down = nn.Conv2d(outer if input_nc is None else input_nc, inner, 4, 2, 1, bias=False)
        if outermost:
            seq = [down, sub, nn.ReLU(True), nn.ConvTranspose2d(inner * 2, outer, 4, 2, 1), nn.Tanh()]
        elif sub is None:
            seq = [nn.LeakyReLU(0.2, True), down, nn.ReLU(True), nn.ConvTranspose2d(inner, outer, 4, 2, 1, bias=False), torch_norm(norm, outer)]
        else:
            seq = [nn.LeakyReLU(0.2, True), down, torch_norm(norm, inner), sub, nn.ReLU(True),
                   nn.ConvTranspose2d(inner * 2, outer, 4, 2, 1, bias=False), torch_norm(norm, outer)] + ([nn.Dropout(0.5)] if dropout else [])
        self.model = nn.Sequential(*seq)

    def forward(self, x):
        return self.model(x) if self.outermost else torch.cat([x, self.model(x)], 1)


class _Unet(nn.Module):
    def __init__(self, norm, num_downs):
        super().__init__()
        b = _Block(norm, 512, 512)
        for _ in range(num_downs - 5):
            b = _Block(norm, 512, 512, b, dropout=True)
        b = _Block(norm, 256, 512, b)
        b = _Block(norm, 128, 256, b)
        b = _Block(norm, 64, 128, b)
        self.model = _Block(norm, 3, 64, b, outermost=True, input_nc=RC + CC)

    def forward(self, x):
        return self.model(x)


class TorchTextureModule(nn.Module):
    """encode = UNetDown(36, 36) (conv without bias, InstanceNorm2d, LeakyReLU), defined before the U-Net of depth log2(size)."""

    def __init__(self, norm, size):
        super().__init__()
        self.encode = nn.Module()
        self.encode.model = nn.Sequential(nn.Conv2d(RC, RC, 4, 2, 1, bias=False), nn.InstanceNorm2d(RC), nn.LeakyReLU(0.2))
        self.unet = _Unet(norm, depth_of(size))

    def forward(self, tex, rois, cloth):
        pooled = O.roi_align(tex, O.reshape_rois(rois), (128, 128), 1.0, 1).to(tex.dtype)
        pooled = pooled.view(tex.shape[0], -1, 128, 128)
        enc = self.encode.model(pooled)
        up = F.interpolate(enc, scale_factor=tex.shape[2] / enc.shape[2])
        return self.unet(torch.cat((up, cloth), 1))


def bn_step(P, bufs, name, h, train):
    y = F.batch_norm(h, bufs[name + ".running_mean"], bufs[name + ".running_var"], P[name + ".weight"], P[name + ".bias"], train, MOMENTUM, EPS)
    if train:
        bufs[name + ".num_batches_tracked"] += 1
    return y


def texture_forward(P, bufs, tex, rois, cloth, norm, training=False):
    """The same network functionally.  training: False (running buffers, no dropout), True (torch RNG dropout) or an O.MaskReplay;
    in training mode `bufs` is updated in place."""
    train = training is not False
    depth = depth_of(tex.shape[2])
    nrm = (lambda name, h: bn_step(P, bufs, name, h, train)) if norm == "batch" else (lambda name, h: h)
    pooled = O.roi_align(tex, O.reshape_rois(rois), (128, 128), 1.0, 1).to(tex.dtype)
    enc = O.unet_down(pooled.view(tex.shape[0], -1, 128, 128), P["encode.model.0.weight"])
    x = torch.cat((F.interpolate(enc, scale_factor=tex.shape[2] / enc.shape[2]), cloth), 1)

    def block(d, x):
        p = prefix(d)
        if d == 0:
            h = F.conv2d(x, P[p + ".model.0.weight"], None, stride=2, padding=1)
            h = O._relu(block(1, h))
            return torch.tanh(F.conv_transpose2d(h, P[p + ".model.3.weight"], P[p + ".model.3.bias"], stride=2, padding=1))
        xl = O._lrelu(x)
        h = F.conv2d(xl, P[p + ".model.1.weight"], None, stride=2, padding=1)
        if d == depth - 1:
            h = nrm(p + ".model.4", F.conv_transpose2d(O._relu(h), P[p + ".model.3.weight"], None, stride=2, padding=1))
        else:
            h = O._relu(block(d + 1, nrm(p + ".model.2", h)))
            h = nrm(p + ".model.6", F.conv_transpose2d(h, P[p + ".model.5.weight"], None, stride=2, padding=1))
            if 4 <= d < depth - 1:
                h = O._dropout(h, 0.5, training)
        return torch.cat([xl, h], 1)

    return block(0, x)


def patchgan_forward(P, bufs, x, norm):
    """TorchPatchGAN(22, 3, norm) in train mode, functionally, with the oracle's LeakyReLU hooks."""
    nrm = (lambda name, h: bn_step(P, bufs, name, h, True)) if norm == "batch" else (lambda name, h: h)
    x = O._lrelu(F.conv2d(x, P["model.0.weight"], P["model.0.bias"], stride=2, padding=1))
    for idx, stride in ((2, 2), (5, 2), (8, 1)):
        x = O._lrelu(nrm("model.%d" % (idx + 1), F.conv2d(x, P["model.%d.weight" % idx], None, stride=stride, padding=1)))
    return F.conv2d(x, P["model.11.weight"], P["model.11.bias"], stride=1, padding=1)


def nontrivial_norm_state(net):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.bias.normal_(0.0, 0.1); m.running_mean.normal_(0.0, 0.1); m.running_var.uniform_(0.5, 1.5)
    return net


@functools.lru_cache(maxsize=None)
def seeded_state(norm, size, seed=11):
    torch.manual_seed(seed)
    net = nontrivial_norm_state(published_init(TorchTextureModule(norm, size)))
    return OrderedDict((k, v.clone()) for k, v in net.state_dict().items())


def to64(bufs):
    return OrderedDict((k, v.clone().double() if v.is_floating_point() else v.clone()) for k, v in bufs.items())


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restated reference alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
def test_the_restated_module_has_the_published_keys_and_agrees_with_its_functional_form(norm):
    net = nontrivial_norm_state(published_init(TorchTextureModule(norm, 64)))
    sd = net.state_dict()
    convs = [k for k in sd if sd[k].dim() == 4]
    assert convs[0] == "encode.model.0.weight" and len(convs) == 1 + 2 * 6
    assert [k for k in sd if k.endswith(".bias") and sd[k[:-4] + "weight"].dim() == 4] == ["unet.model.model.3.bias"]
    sites = [k[:-len(".running_mean")] for k in sd if k.endswith("running_mean")]
    if norm == "batch":
        assert sites == [prefix(d) + ".model.2" for d in range(1, 5)] + [prefix(5) + ".model.4"] + [prefix(d) + ".model.6" for d in range(4, 0, -1)]
    else:
        assert not sites and len(sd) == 14
    tex, rois, cloths, _ = O.synth_texture_batch(2, 64, 64, seed=3)
    P, bufs = split_state(sd, torch.float32)
    net.train()
    torch.manual_seed(4)
    want = net(tex, rois, cloths)
    torch.manual_seed(4)
    got = texture_forward(P, bufs, tex, rois, cloths, norm, training=True)
    assert rel(got, want) < 1e-6
    after = net.state_dict()
    for k, v in bufs.items():
        assert torch.allclose(v.float(), after[k].float(), rtol=1e-5, atol=1e-7), k


def test_the_host_simulator_keeps_refusing_the_texture_stage(tmp_path):
    from swapnet_amd.modules.swapnet_modules import TextureModule
    backend = NativeBackend("texture", is_train=False, ctx=backends.hostsim_ctx(), default_shape=(1, 64, 64))
    for norm in NORMS:
        with pytest.raises(NotImplementedError, match="for the texture stage"):
            TextureModule(norm_type=norm, img_size=64, backend=backend)
        with pytest.raises(NotImplementedError, match="device library"):
            engine.NativeModel(backends.hostsim_ctx(), "texture", 1, 64, 64, is_train=False, norm=norm)
    with pytest.raises(NotImplementedError, match="not found"):
        TextureModule(norm_type="group", img_size=64, backend=backend)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the generator standalone, seeded init
# ---------------------------------------------------------------------------------------------------------------------
def native_module(ctx, norm, B, H):
    from swapnet_amd.modules.swapnet_modules import TextureModule
    backend = NativeBackend("texture", is_train=False, ctx=ctx, default_shape=(B, H, H))
    return TextureModule(norm_type=norm, img_size=H, backend=backend), backend


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("B,H", [(2, 64), (1, 128)])
def test_standalone_generator_matches_float64_and_keeps_the_torch_state_dict(B, H, norm):
    ctx = backends.gpu_ctx()
    sd = seeded_state(norm, H)
    net, backend = native_module(ctx, norm, B, H)
    try:
        net.load_state_dict(sd)
        back = net.state_dict()
        assert list(back) == list(sd)                                     # torch's keys in torch's order; no key for a bias that does not exist
        for k, v in sd.items():
            assert back[k].dtype == v.dtype and back[k].shape == v.shape and torch.equal(back[k], v), k
        TorchTextureModule(norm, H).load_state_dict(back, strict=True)
        tex, rois, cloths, _ = O.synth_texture_batch(B, H, H, seed=5)
        P, bufs = split_state(sd, torch.float64)
        torch.manual_seed(77)
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)))
        torch.manual_seed(77)
        net.train()
        got = net(tex, rois, cloths).cpu()
        masks = [t.cpu() for t, _ in backend.cur.dropout_masks(engine.NET_G, seed=seed)]
        assert [tuple(t.shape) for t in masks] == [(B, 512, H >> d, H >> d) for d in range(depth_of(H) - 2, 3, -1)]
        with torch.no_grad():
            want = texture_forward(P, bufs, tex.double(), rois, cloths.double(), norm, training=O.MaskReplay(masks))
        e_train = rel(got, want)
        after = net.state_dict()
        e_buf = max([rel(after[k], v) for k, v in bufs.items() if v.is_floating_point()] + [0.0])
        assert all(int(after[k]) == int(v) == 1 for k, v in bufs.items() if not v.is_floating_point())
        net.eval()
        got = net(tex, rois, cloths).cpu()
        with torch.no_grad():
            want = texture_forward(P, bufs, tex.double(), rois, cloths.double(), norm, training=False)
        e_eval = rel(got, want)
        print("standalone TextureModule --norm %s B %d %d x %d: train forward %.2e  eval forward %.2e  running buffers %.2e" % (
            norm, B, H, H, e_train, e_eval, e_buf))
        assert e_train <= FWD_BAR and e_buf <= FWD_BAR and e_eval <= FWD_BAR
        final = net.state_dict()
        for k in bufs:
            assert torch.equal(final[k], after[k]), k                      # eval moves nothing
        torch.manual_seed(1)
        with pytest.raises(RuntimeError, match="bias"):                   # an instance-norm checkpoint is refused with the keys named
            net.load_state_dict(O.texture_module_params(img_size=H))
    finally:
        close_backend(backend)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_seeded_init_equals_the_published_rule(norm):
    ctx = backends.gpu_ctx()
    torch.manual_seed(1234)
    want = published_init(TorchTextureModule(norm, 64)).state_dict()
    torch.manual_seed(1234)
    net, backend = native_module(ctx, norm, 1, 64)
    try:
        modules.init_weights(net, "normal", 0.02)
        got = net.state_dict()
        assert list(got) == list(want)
        for k, v in want.items():
            assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
        here = torch.rand(4)                                              # the global RNG stands where torch's build leaves it
        torch.manual_seed(1234)
        published_init(TorchTextureModule(norm, 64))
        assert torch.equal(here, torch.rand(4))
    finally:
        close_backend(backend)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: training steps
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_case(norm, B):
    G, gbufs = split_state(seeded_state(norm, 64), torch.float32)
    torch.manual_seed(21)
    from tests.test_batch_norm import published_init as d_init
    dnet = nontrivial_norm_state(d_init(TorchPatchGAN(3 + CC, 3, norm)))
    # Without a norm layer the published init (gain 0.02, biases 0) leaves both predictions at ~ 0, where the gradient of the
    # prediction conv's bias, 0.5 (mean sigmoid(fake) + mean sigmoid(real) - 1), cancels to 1e-5 of its terms -- below what fp32
    # resolves to 1e-4.  Conv biases off zero keep that scalar conditioned.
    with torch.no_grad():
        dnet.model[0].bias.normal_(0.0, 0.1)
        dnet.model[-1].bias.fill_(0.3)
    D, dbufs = split_state(dnet.state_dict(), torch.float32)
    return G, gbufs, D, dbufs, O.vgg16_feature_params(), O.synth_texture_batch(B, 64, 64, seed=31 + B)


class swapped_networks:
    """O.TextureStepOracle with the oracle's generator and discriminator forwards swapped for this file's for the duration."""

    def __init__(self, norm, gbufs, dbufs):
        self.norm, self.gbufs, self.dbufs = norm, gbufs, dbufs

    def __enter__(self):
        self.saved = O.texture_module_forward, O.patchgan_forward
        norm, gbufs, dbufs = self.norm, self.gbufs, self.dbufs
        O.texture_module_forward = lambda P, tex, rois, cloth, num_roi=12, training=False, taps=None: texture_forward(
            P, gbufs, tex, rois, cloth, norm, training)
        O.patchgan_forward = lambda P, x, n_layers=None, taps=None: patchgan_forward(P, dbufs, x, norm)
        return self

    def __exit__(self, *exc):
        O.texture_module_forward, O.patchgan_forward = self.saved
        return False


def load_training_state(m, st, gbufs, dbufs, step_index):
    f32 = lambda d: {k: v.float() if v.is_floating_point() else v for k, v in d.items()}
    m.load_state_dict(engine.NET_G, {**f32(st.G), **f32(gbufs)})
    m.load_state_dict(engine.NET_D, {**f32(st.D), **f32(dbufs)})
    for net, opt in ((engine.NET_G, st.optG), (engine.NET_D, st.optD)):
        m.load_state_dict(net, f32(opt.m), which=engine.W_EXP_AVG)
        m.load_state_dict(net, f32(opt.v), which=engine.W_EXP_AVG_SQ)
        m.optim_step_count(net, step_index)


def run_pinned_steps(ctx, norm, B, nsteps):
    G, gbufs0, D, dbufs0, vgg, batch = step_case(norm, B)
    gb64, db64 = to64(gbufs0), to64(dbufs0)
    s64 = O.TextureStepOracle(G, D, vgg, dtype=torch.float64)
    m = engine.NativeModel(ctx, "texture", B, 64, 64, is_train=True, norm=norm)
    worst = dict(loss=0.0, gradG=0.0, gradD=0.0, buffers=0.0, fakes=0.0)
    try:
        assert list(m.param_infos(engine.NET_G)) == list(G) and list(m.param_infos(engine.NET_D)) == list(D)
        assert len(m.buffer_infos(engine.NET_G)) == len(gbufs0) and len(m.buffer_infos(engine.NET_D)) == len(dbufs0)
        m.load_state_dict(engine.NET_VGG, vgg_state_dict(m, vgg))
        m.set_hyper()
        for i, t in enumerate(batch):
            m.set_input(i, t)
        for si in range(nsteps):
            load_training_state(m, s64, gb64, db64, si)
            seed = STEP_SEEDS[si]
            masks = [t.cpu() for t, _ in m.dropout_masks(engine.NET_G, seed=seed)]
            assert [tuple(t.shape) for t in masks] == [(B, 512, 4, 4)]
            m.forward(True, seed)
            m.backward_D(LABELS[0], LABELS[1])
            gD = m.state_dict(engine.NET_D, which=engine.W_GRAD, to_cpu=True)
            m.optimizer_step(engine.NET_D)
            m.backward_G(LABELS[2])
            gG = m.state_dict(engine.NET_G, which=engine.W_GRAD, to_cpu=True)
            m.optimizer_step(engine.NET_G)
            replay = O.PatternReplay(backends.collect_patterns(m, vgg=True))
            s64.training, s64.patterns = O.MaskReplay(masks), replay
            with swapped_networks(norm, gb64, db64):
                s64.step(*batch, labels=list(LABELS))
            flips = replay.check()
            L = m.losses()
            afterG, afterD = m.state_dict(engine.NET_G, to_cpu=True), m.state_dict(engine.NET_D, to_cpu=True)
            e_loss = max(abs(L[k] - v) / abs(v) for k, v in s64.losses.items())
            e_buf = max([rel(afterG[k], v) for k, v in gb64.items() if v.is_floating_point()] +
                        [rel(afterD[k], v) for k, v in db64.items() if v.is_floating_point()] + [0.0])
            e_out = rel(m.output(), s64.fakes)
            print("texture --norm %s step %d B %d: flips %s  losses %.2e  fakes %.2e  running buffers %.2e" % (norm, si, B, flips, e_loss, e_out, e_buf))
            assert set(gG) == set(s64.grads_G) and set(gD) == set(s64.grads_D)      # every gradient, gamma and beta included
            wG = backends.assert_grads_replayed(gG, s64.grads_G, lambda k: False, GRAD_BAR, (norm, B, si, "G"))
            wD = backends.assert_grads_replayed(gD, s64.grads_D, lambda k: False, GRAD_BAR, (norm, B, si, "D"))
            print("texture --norm %s step %d B %d: worst pinned gradient G %.2e D %.2e" % (norm, si, B, wG, wD))
            assert e_loss <= FWD_BAR and e_buf <= FWD_BAR and e_out <= FWD_BAR, (si, e_loss, e_buf, e_out)
            assert all(int(afterG[k]) == int(v) == si + 1 for k, v in gb64.items() if not v.is_floating_point())
            assert all(int(afterD[k]) == int(v) == 3 * (si + 1) for k, v in db64.items() if not v.is_floating_point())
            for k, v in dict(loss=e_loss, gradG=wG, gradD=wD, buffers=e_buf, fakes=e_out).items():
                worst[k] = max(worst[k], v)
    finally:
        m.close()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_two_training_steps_match_float64_with_pattern_and_masks_replayed(norm):
    print("texture --norm %s B 2, two steps:" % norm, {k: "%.2e" % v for k, v in run_pinned_steps(backends.gpu_ctx(), norm, 2, 2).items()})


@pytest.mark.gpu
def test_one_training_step_at_batch_one_under_batch_norm():
    print("texture --norm batch B 1, one step:", {k: "%.2e" % v for k, v in run_pinned_steps(backends.gpu_ctx(), "batch", 1, 1).items()})


def fresh_step_model(ctx, norm, B):
    G, gbufs, D, dbufs, vgg, batch = step_case(norm, B)
    m = engine.NativeModel(ctx, "texture", B, 64, 64, is_train=True, norm=norm)
    backends.reset_state(m, {engine.NET_G: {**G, **gbufs}, engine.NET_D: {**D, **dbufs}})
    m.load_state_dict(engine.NET_VGG, vgg_state_dict(m, vgg))
    for i, t in enumerate(batch):
        m.set_input(i, t)
    return m


def running_state(m):
    return {(net, k): v.cpu() for net in (engine.NET_G, engine.NET_D) for k, v in m.state_dict(net).items() if "running" in k or "tracked" in k}


@pytest.mark.gpu
def test_the_captured_step_is_bit_equal_to_the_eager_one_under_batch_norm():
    ctx = backends.gpu_ctx()
    results = []
    for captured in (False, True):
        m = fresh_step_model(ctx, "batch", 2)
        try:
            for si in range(3):                                           # captured: eager, record, replay
                m.step(LABELS, training=True, seed=40 + si, captured=captured)
            ctx.sync()
            results.append((m.losses(), m.arena(engine.NET_D, engine.W_WEIGHT).clone(), m.arena(engine.NET_G, engine.W_WEIGHT).clone(), running_state(m)))
        finally:
            m.close()
    (la, da, ga, ba), (lb, db, gb, bb) = results
    assert la == lb, (la, lb)
    assert torch.equal(da, db) and torch.equal(ga, gb)
    assert len(ba) == 3 * (9 + 3) and all(torch.equal(ba[k], bb[k]) for k in ba)
    assert all(int(v) == (3 if net == engine.NET_G else 9) for (net, k), v in ba.items() if k.endswith("num_batches_tracked"))


@pytest.mark.gpu
def test_a_model_of_a_second_batch_size_shares_the_running_buffers():
    ctx = backends.gpu_ctx()
    m = fresh_step_model(ctx, "batch", 2)
    m1 = None
    try:
        m.step(LABELS, training=True, seed=9)
        m1 = engine.NativeModel(ctx, "texture", 1, 64, 64, share=m)
        assert m1.norm == "batch"
        key, cnt = prefix(3) + ".model.6.running_mean", prefix(3) + ".model.6.num_batches_tracked"
        a = m.get_buffer(engine.NET_G, key, (256,), torch.float32).cpu()
        assert torch.equal(m1.get_buffer(engine.NET_G, key, (256,), torch.float32).cpu(), a) and float(a.abs().sum()) > 0
        for i, t in enumerate(step_case("batch", 1)[5]):
            m1.set_input(i, t)
        m1.forward(True, 10)                                              # a training-mode forward of the sharer updates the one set
        b = m.get_buffer(engine.NET_G, key, (256,), torch.float32).cpu()
        assert not torch.equal(a, b) and torch.equal(m1.get_buffer(engine.NET_G, key, (256,), torch.float32).cpu(), b)
        assert int(m.get_buffer(engine.NET_G, cnt, (), torch.int64)) == int(m1.get_buffer(engine.NET_G, cnt, (), torch.int64)) == 2
        m1.forward(False, 0)                                              # eval: nothing moves
        assert torch.equal(m.get_buffer(engine.NET_G, key, (256,), torch.float32).cpu(), b)
    finally:
        if m1 is not None:
            m1.close()
        m.close()


@pytest.mark.gpu
def test_the_pipeline_takes_a_batch_norm_texture_model_in_eval_mode():
    ctx = backends.gpu_ctx()
    torch.manual_seed(3)
    Gw = O.warp_module_params()
    w = engine.NativeModel(ctx, "warp", 1, 64, 64, is_train=False)
    t = engine.NativeModel(ctx, "texture", 1, 64, 64, is_train=False, norm="batch")
    pipe = None
    try:
        w.load_state_dict(engine.NET_G, Gw)
        t.load_state_dict(engine.NET_G, seeded_state("batch", 64))
        bodys, inputs, _ = O.synth_warp_batch(1, 64, 64, seed=9)
        tex, rois, _, _ = O.synth_texture_batch(1, 64, 64, seed=10)
        w.set_input(0, bodys); w.set_input(1, inputs)
        t.set_input(0, tex); t.set_input(1, rois)
        pipe = engine.NativePipeline(w, t)
        outs = []
        for use_graph in (False, True, True, True):                       # eager; then eager, capture, replay
            pipe.run(use_graph)
            ctx.sync()
            outs.append(t.output().cpu().clone())
        labels = pipe.labels()
        before = running_state_G(t)
        t.set_input_labels(2, labels)
        t.forward(False, 0)                                               # the eager eval-mode forward on the pipeline's labels
        ctx.sync()
        want = t.output().cpu()
        assert float(want.abs().max()) > 0
        for o in outs:
            assert torch.equal(o, want)
        sd = seeded_state("batch", 64)
        for k, v in before.items():                                       # inference: the running buffers are read, never written
            assert torch.equal(v, sd[k]), k
    finally:
        if pipe is not None:
            pipe.close()
        t.close(); w.close()


def running_state_G(m):
    return {k: v.cpu() for k, v in m.state_dict(engine.NET_G).items() if "running" in k or "tracked" in k}


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the public API
# ---------------------------------------------------------------------------------------------------------------------
def _opt(tmp_path, **kw):
    from tests.test_models_api import make_opt
    return make_opt(tmp_path, "gpu", model="texture", crop_size=64, **kw)


@pytest.mark.gpu
def test_create_model_trains_saves_and_tests_under_norm_batch(tmp_path):
    from swapnet_amd.models import create_model
    from swapnet_amd.modules.swapnet_modules import TextureModule
    opt = _opt(tmp_path, norm="batch", init_type="normal")
    torch.manual_seed(1234)
    want = published_init(TorchTextureModule("batch", 64)).state_dict()
    torch.manual_seed(1234)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                   # (seeded-random VGG16 where no pretrained weights are at hand)
        model = create_model(opt)
    model.setup(opt)
    assert isinstance(model.net_generator, TextureModule)
    start = model.net_generator.state_dict()
    assert list(start) == list(want)
    for k, v in want.items():                                             # torch.manual_seed(s); create_model(opt) starts from torch's weights
        assert torch.equal(start[k], v), k
    dsd = model.net_discriminator.state_dict()
    assert "model.3.running_mean" in dsd and "model.2.bias" not in dsd
    tex, rois, cloths, tgt = O.synth_texture_batch(2, 64, 64, seed=8)
    data = dict(input_textures=tex, rois=rois, cloths=cloths, target_textures=tgt, cloth_paths=["c0", "c1"], texture_paths=["t0", "t1"])
    for batch in (data, compact_batch(2, 64)):                            # the float batch, then the compact uint8 one
        model.set_input(batch)
        model.optimize_parameters()
        losses = model.get_current_losses()
        assert losses and all(np.isfinite(v) for v in losses.values()), losses
    assert model.fakes.shape == (2, 3, 64, 64)
    sd = model.net_generator.state_dict()
    moved = prefix(2) + ".model.1.weight"
    assert not torch.equal(sd[moved], start[moved]) and not torch.equal(sd[prefix(2) + ".model.6.weight"], start[prefix(2) + ".model.6.weight"])
    assert all(int(v) == 2 for k, v in sd.items() if k.endswith("tracked"))
    assert all(int(v) == 6 for k, v in model.net_discriminator.state_dict().items() if k.endswith("tracked"))
    model.save_checkpoint("latest")
    opt2 = _opt(tmp_path, norm="batch", init_type="normal", continue_train=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m2 = create_model(opt2)
    m2.setup(opt2)
    for net, net2 in ((model.net_generator, m2.net_generator), (model.net_discriminator, m2.net_discriminator)):
        a, b = net.state_dict(), net2.state_dict()
        assert list(a) == list(b)
        for k, v in a.items():
            assert b[k].dtype == v.dtype and torch.equal(b[k], v), k
    model.eval()
    model.set_input(data)
    model.test()
    assert bool(torch.isfinite(model.fakes).all())
    after = model.net_generator.state_dict()
    for k, v in sd.items():
        if "running" in k or "tracked" in k:
            assert torch.equal(after[k], v), k


@pytest.mark.gpu
def test_netG_unet_128_builds_under_norm_batch_with_a_batch_norm_discriminator(tmp_path):
    from swapnet_amd.models import create_model
    from tests.test_models_api import make_opt
    from tests.test_unet128 import expected_keys
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        model = create_model(make_opt(tmp_path, "gpu", model="texture", netG="unet_128", crop_size=128, norm="batch"))
    assert list(model.net_generator.state_dict()) == expected_keys()     # the generator ignores the flag
    dsd = model.net_discriminator.state_dict()
    assert sum(k.endswith("running_mean") for k in dsd) == 3 and "model.2.bias" not in dsd
