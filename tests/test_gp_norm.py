"""--gan_mode wgan-gp / dragan-lp under --norm batch and --norm none (warp stage, device library): the reverse-over-reverse pass of
csrc/gp.cpp through BatchNorm2d (batch_norm.hip batch_norm_bwd2) and through conv -> LeakyReLU alone.

Reference: tests/test_batch_norm.py's TorchPatchGAN under published_init, in torch fp32 and float64, in train mode, fed with the
oracle's generator output; the penalty restated from its published formula (Gulrajani et al. 2017; Kodali et al. 2017):

    x_hat = a + alpha (b - a),  a = conditioned real batch,  b = conditioned fakes (wgan-gp) or a + 0.5 std(a) beta (dragan)
    g     = d sum(D(x_hat)) / d x_hat                                     (create_graph: D's parameters stay in the graph)
    gp    = mean_n (||g_n||_2 - 1)^2   (lp: max(0, ||g_n||_2 - 1)^2);     loss_D = 0.5 (loss_D_fake + loss_D_real) + lambda_gp gp

with alpha / beta handed to the library through set_gp_random.  Under batch the module is called in train mode on x_hat too: one
discriminator step makes the running updates fake, real, x_hat, and the generator pass's fakes through the updated discriminator
are the fourth.  wgan-gp covers the real / fake interpolation and the gp form, dragan-lp the perturbed-real one and the lp form.
n_layers_D = 1: a single norm site, on the k4 s1 layer right behind layer 0 (under wgan-gp: with dragan-lp's perturbed input torch's
own fp32 evaluation of that case is 4.7e-5 from float64 in loss_D_gp -- one LeakyReLU branch -- which a 1e-5 bar cannot judge).

Measured on the MI355X: losses within 1.3e-6 of float64 (torch fp32's own loss_D_gp: up to 9.8e-7), running buffers within 4.2e-7,
worst gradient rel-L2 2.8e-6 (torch fp32 1.8e-6) -- but for model.3.bias at n_layers_D = 1, 6.5e-3 in three of its 128 channels and
1.5e-6 without them: LeakyReLU branches the first-order pass takes differently on the native generator's fp32 fakes, the signature
backends.assert_grads_vs_fp64 accepts and reports.
"""
import functools
from collections import OrderedDict

import pytest
import torch
from torch import nn

from oracle import swapnet_oracle as O
from swapnet_amd import engine
from tests import backends
from tests.test_batch_norm import BATCH, D_IN, FWD_BAR, SIZE, TorchPatchGAN, published_init, rel

MODES = {"wgan-gp": (2, 1), "dragan-lp": (0, 3)}        # name -> (gan_mode, gp_mode) of swn_hyper
LABELS = (0.0, 1.0, 1.0)                                # hard labels: fake, real (backward_D), real (backward_G)
LAMBDA_GP = 10.0
CASES = [("batch", "wgan-gp", 3), ("batch", "dragan-lp", 3), ("none", "wgan-gp", 3), ("none", "dragan-lp", 3), ("batch", "wgan-gp", 1)]
# Without a norm layer the published gain 0.02 leaves ||g_n|| at 0.65 -- the lp form is then exactly 0 and holds nothing -- so the
# none cases draw the weights with gain 0.03 (five convs: ||g_n|| ~ 5).  Under batch the norms are ~ 14-20 with the published gain.
GAIN = {"batch": 0.02, "none": 0.03}


def penalty(f, real, fake, mode, alpha, beta):
    if mode.startswith("dragan"):
        b = real + 0.5 * real.std() * beta.to(real.dtype)
    else:
        b = fake
    x = (real + alpha.to(real.dtype) * (b - real)).detach().requires_grad_(True)
    pred = f(x)
    g, = torch.autograd.grad(pred, x, grad_outputs=torch.ones_like(pred), create_graph=True)
    norm = g.reshape(g.shape[0], -1).norm(p=2, dim=1)
    return ((norm - 1) ** 2).mean() if mode.endswith("gp") else (torch.clamp(norm - 1, min=0) ** 2).mean()


@functools.lru_cache(maxsize=None)
def reference(norm, mode, n_layers):
    """backward_D of one step in torch fp32 and float64 from the same state: losses, every D gradient, the buffers behind the
    three running updates.  Computed once per case."""
    torch.manual_seed(3)
    G = O.warp_module_params()
    d32 = published_init(TorchPatchGAN(D_IN, n_layers, norm), GAIN[norm])
    for m in d32.modules():
        if isinstance(m, nn.BatchNorm2d):                               # beta != 0, non-trivial running state
            with torch.no_grad():
                m.bias.normal_(0.0, 0.1); m.running_mean.normal_(0.0, 0.1); m.running_var.uniform_(0.5, 1.5)
    pre = OrderedDict((k, v.clone()) for k, v in d32.state_dict().items())
    bodys, inputs, targets = O.synth_warp_batch(BATCH, SIZE, SIZE, seed=1234)
    g = torch.Generator().manual_seed(77)
    alpha = torch.rand([BATCH, 1, 1, 1], generator=g)
    beta = torch.rand([BATCH, D_IN, SIZE, SIZE], generator=g) if mode.startswith("dragan") else None
    out = dict(G=G, pre=pre, batch=(bodys, inputs, targets), alpha=alpha, beta=beta)
    for dtype in (torch.float32, torch.float64):
        D = d32 if dtype == torch.float32 else TorchPatchGAN(D_IN, n_layers, norm).double()
        if dtype == torch.float64:
            D.load_state_dict(OrderedDict((k, v.double() if v.is_floating_point() else v.clone()) for k, v in pre.items()))
        D.train()
        with torch.no_grad():
            fakes = O.warp_module_forward(OrderedDict((k, v.to(dtype)) for k, v in G.items()), bodys.to(dtype), inputs.to(dtype), training=False)
        cond_fake, cond_real = torch.cat((bodys.to(dtype), fakes), 1), torch.cat((bodys, targets), 1).to(dtype)
        lab = [torch.tensor([v], dtype=dtype) for v in LABELS]
        loss_fake = O.gan_loss(D(cond_fake), lab[0], mode, False)
        loss_real = O.gan_loss(D(cond_real), lab[1], mode, True)
        loss_gp = LAMBDA_GP * penalty(D, cond_real, cond_fake, mode, alpha, beta)
        loss = 0.5 * (loss_fake + loss_real) + loss_gp
        names = [k for k, _ in D.named_parameters()]
        grads = torch.autograd.grad(loss, list(D.parameters()))
        tag = "32" if dtype == torch.float32 else "64"
        out["g" + tag] = OrderedDict(zip(names, [t.detach() for t in grads]))
        out["L" + tag] = {k: float(v.detach()) for k, v in dict(D=loss, D_fake=loss_fake, D_real=loss_real, D_gp=loss_gp).items()}
        out["bufs" + tag] = OrderedDict((k, v.clone()) for k, v in D.named_buffers())
        if dtype == torch.float64:
            out["D64"], out["cond_fake64"] = D, cond_fake
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("norm,mode,n_layers", CASES, ids=["%s-%s-n%d" % c for c in CASES])
def test_backward_D_with_a_gradient_penalty_matches_float64(norm, mode, n_layers):
    ctx = backends.gpu_ctx()
    r = reference(norm, mode, n_layers)
    m = engine.NativeModel(ctx, "warp", BATCH, SIZE, SIZE, is_train=True, dropout=0.0, norm=norm, n_layers_D=n_layers)
    try:
        m.load_state_dict(engine.NET_G, r["G"])
        m.load_state_dict(engine.NET_D, r["pre"])
        m.set_hyper(gan_mode=MODES[mode][0], gp_mode=MODES[mode][1], lambda_gp=LAMBDA_GP)
        for i, t in enumerate(r["batch"]):
            m.set_input(i, t)
        m.forward(False, 0)
        m.set_gp_random(r["alpha"], r["beta"])
        m.backward_D(LABELS[0], LABELS[1])
        gD = m.state_dict(engine.NET_D, which=engine.W_GRAD, to_cpu=True)
        L = m.losses()
        after3 = m.state_dict(engine.NET_D, to_cpu=True)
        worst = {k: abs(L[k] - r["L64"][k]) / abs(r["L64"][k]) for k in ("D_gp", "D_fake", "D_real", "D")}
        # every D gradient, gamma and beta included; under none the inner layers have no bias, so no second-order bias gradient
        assert set(gD) == set(r["g64"]), (sorted(set(gD) ^ set(r["g64"])))
        assert L["D_gp"] > 0
        worst["buffers"] = 0.0
        if norm == "batch":
            for k, v in r["bufs64"].items():                              # fake, real, x_hat
                if v.is_floating_point():
                    worst["buffers"] = max(worst["buffers"], rel(after3[k], v))
                else:
                    assert int(after3[k]) == int(v) == 3, (k, int(after3[k]), int(v))
        else:
            assert not m.buffer_infos(engine.NET_D)
        print("gp %s %s n%d: losses D_gp %.2e D_fake %.2e D_real %.2e D %.2e (torch fp32's own D_gp %.2e)  buffers %.2e" % (
            norm, mode, n_layers, worst["D_gp"], worst["D_fake"], worst["D_real"], worst["D"],
            abs(r["L32"]["D_gp"] - r["L64"]["D_gp"]) / abs(r["L64"]["D_gp"]), worst["buffers"]))
        w = backends.assert_grads_vs_fp64(gD, r["g32"], r["g64"], lambda k: False, (norm, mode, n_layers, "gradD"))
        print("gp %s %s n%d: worst gradD rel-L2 vs float64: native %.2e, torch fp32 %.2e" % (norm, mode, n_layers, w[0], w[1]))
        for k, v in worst.items():
            assert v <= FWD_BAR, (norm, mode, n_layers, k, v)
        # the rest of the step: the generator pass sends the fakes through the UPDATED discriminator, the fourth running update
        m.optimizer_step(engine.NET_D)
        m.backward_G(LABELS[2])
        if norm == "batch":
            after4 = m.state_dict(engine.NET_D, to_cpu=True)
            D = r["D64"]
            saved = OrderedDict((k, v.clone()) for k, v in D.state_dict().items())
            try:
                D.load_state_dict(OrderedDict((k, after4[k].double() if k in dict(D.named_parameters()) else v) for k, v in saved.items()))
                with torch.no_grad():
                    D.train()(r["cond_fake64"])
                w4 = 0.0
                for k, v in D.named_buffers():
                    if v.is_floating_point():
                        w4 = max(w4, rel(after4[k], v))
                    else:
                        assert int(after4[k]) == int(v) == 4, (k, int(after4[k]), int(v))
            finally:
                D.load_state_dict(saved)                                    # the shared reference stays as it was
            print("gp %s %s n%d: buffers after the generator pass %.2e" % (norm, mode, n_layers, w4))
            assert w4 <= FWD_BAR, (norm, mode, n_layers, "buffers after the full step", w4)
    finally:
        m.close()
