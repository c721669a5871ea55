"""Drop-in boundary: the reference's model API -- create_model(opt), set_input,
optimize_parameters, get_current_losses, fakes, save_checkpoint / load, optimizer state dicts --
served by swapnet_amd.  With the same torch seed the model draws the same three smooth labels
as the reference and must therefore reproduce the golden losses of the REAL reference."""
import argparse
import os

import numpy as np
import pytest
import torch

from oracle import swapnet_oracle as O
from oracle.golden_io import compare
from tests import backends

pytestmark = pytest.mark.small_channel_winograd      # tests/conftest.py: small shapes on the Winograd forms

BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]


def make_opt(tmp, backend, **kw):
    lib = None
    if backend == "sim":
        lib = backends.hostsim_ctx().lib
    else:
        backends.gpu_ctx()
    o = dict(gpu_id=0, is_train=True, checkpoints_dir=str(tmp), name="t", no_confirm=True, model="warp",
             body_channels=12, body_representation="rgb", cloth_channels=19, cloth_representation="labels",
             texture_channels=3, init_type="kaiming", init_gain=0.02, discriminator="basic", n_layers_D=3,
             norm="instance", gan_label_mode="smooth", gan_mode="vanilla", lambda_discriminator=1.0, lambda_gan=1.0,
             lambda_gp=10, optimizer_G="AdamW", optimizer_D="AdamW", lr=1e-4, d_lr=4e-4, weight_decay=0.0,
             d_weight_decay=0.01, b1=0.9, b2=0.999, beta1=0.5, verbose=False, continue_train=False,
             load_epoch="latest", batch_size=2, crop_size=64, warp_mode="gan", lambda_ce=100.0,
             body_norm_stats=((0.0,) * 3, (1.0,) * 3), texture_norm_stats=((0.0,) * 3, (1.0,) * 3),
             netG="swapnet", lambda_l1=10.0, lambda_content=20.0, lambda_style=1e-8, _swapnet_lib=lib)
    o.update(kw)
    return argparse.Namespace(**o)


@pytest.mark.parametrize("backend", BACKENDS)
def test_warp_model_reproduces_reference_losses_and_checkpoints(backend, tmp_path, golden_dir):
    from swapnet_amd.models import create_model
    gold = np.load(os.path.join(golden_dir, "warp_step_64.npz"))
    opt = make_opt(tmp_path, backend)
    model = create_model(opt)
    model.setup(opt)
    assert model.loss_names == ["D", "D_real", "D_fake", "G", "G_gan", "G_ce"]          # base_gan.py:161-167, warp_model.py:76
    assert model.model_names == ["generator", "discriminator"]
    # weights of the reference run (same seed => same kaiming draws in the oracle's RNG-faithful builder)
    torch.manual_seed(int(gold["meta/init_seed"]))
    G, D = O.warp_module_params(), O.patchgan_params(22)
    model.net_generator.load_state_dict(G)
    model.net_discriminator.load_state_dict(D)
    model.eval()                                                   # dropout off, like the golden run
    bodys, inputs, targets = O.synth_warp_batch(2, 64, 64, seed=1234)
    data = dict(bodys=bodys, input_cloths=inputs, target_cloths=targets, cloth_paths=["c0", "c1"], body_paths=["b0", "b1"])
    model.set_input(data)
    torch.manual_seed(int(gold["meta/step_seeds"][0]))            # the step draws its 3 labels from here
    model.optimize_parameters()
    losses = model.get_current_losses()
    assert list(losses.keys()) == model.loss_names
    for k, v in losses.items():
        ref = float(gold["step0/loss/" + k])
        assert abs(v - ref) <= 1e-3 * abs(ref) + 1e-6, (k, v, ref)
    ok, msg = compare(gold, "step0/fakes", model.fakes, 1e-3, 1e-3)
    assert ok, msg
    assert model.fakes[0].argmax(dim=0).shape == (64, 64)           # inference.py:149 / data_utils.py:322
    assert model.get_image_paths() == (("c0", "b0"), ("c1", "b1"))
    model.compute_visuals()
    vis = model.get_current_visuals()
    assert set(vis) == {"inputs_decoded", "bodys_unnormalized", "fakes_decoded", "targets_decoded"}
    assert torch.equal(vis["fakes_decoded"], O.decode_cloth_labels(model.fakes.cpu()))
    # ---- checkpoints: reference file names + key layout, loadable by plain torch ----------
    model.save_checkpoint("latest")
    for f in ("latest_net_generator.pth", "latest_net_discriminator.pth", "latest_optim_G.pth", "latest_optim_D.pth"):
        assert os.path.exists(os.path.join(model.save_dir, f)), f
    sd = torch.load(os.path.join(model.save_dir, "latest_net_generator.pth"))
    assert list(sd.keys()) == list(G.keys()) and sd["upsample_and_pad.2.weight"].shape == (19, 192, 4, 4)
    osd = torch.load(os.path.join(model.save_dir, "latest_optim_D.pth"))
    ps = [torch.nn.Parameter(v.clone()) for v in D.values()]
    topt = torch.optim.AdamW(ps, lr=4e-4, weight_decay=0.01)
    topt.load_state_dict(osd)                                      # torch accepts our optimizer state dict
    assert float(topt.state[ps[0]]["step"]) == 1.0
    # resume: a fresh model restored from the checkpoint continues bit-identically
    opt2 = make_opt(tmp_path, backend, continue_train=True)
    m2 = create_model(opt2)
    m2.setup(opt2)
    m2.eval()
    for m in (model, m2):
        m.set_input(data)
        torch.manual_seed(7)
        m.optimize_parameters()
    assert model.get_current_losses() == m2.get_current_losses()
    a = model.net_generator.state_dict()["body_down2.model.0.weight"]
    b = m2.net_generator.state_dict()["body_down2.model.0.weight"]
    assert torch.equal(a, b)
    # a smaller last batch (CappedDataLoader tail) keeps training on the same state
    small = {k: (v[:1] if torch.is_tensor(v) else v[:1]) for k, v in data.items()}
    model.set_input(small)
    torch.manual_seed(8)
    model.optimize_parameters()
    assert model.fakes.shape == (1, 19, 64, 64) and all(np.isfinite(v) for v in model.get_current_losses().values())
    assert model.optimizer_G.state_dict()["state"][0]["step"] == 3


@pytest.mark.parametrize("backend", BACKENDS)
def test_inference_only_generator_and_error_conventions(backend, tmp_path):
    from swapnet_amd.models import create_model, find_model_using_name
    opt = make_opt(tmp_path, backend, is_train=False, batch_size=1)
    model = create_model(opt)
    assert model.model_names == ["generator"] and not hasattr(model, "net_discriminator")   # base_gan.py:145
    torch.manual_seed(0)
    G = O.warp_module_params()
    model.net_generator.load_state_dict(G)
    model.eval()
    bodys, inputs, _ = O.synth_warp_batch(1, 64, 64, seed=5)
    model.set_input(dict(bodys=bodys, input_cloths=inputs, cloth_paths=[""], body_paths=[""]))
    model.test()                                                   # base_model.py:103-110
    with torch.no_grad():
        ref = O.warp_module_forward(G, bodys, inputs)
    assert float((model.fakes.cpu() - ref).norm() / ref.norm()) < 1e-3
    # error conventions
    with pytest.raises(NotImplementedError):
        find_model_using_name("pix2pix")
    from swapnet_amd.modules.loss import GANLoss
    with pytest.raises(NotImplementedError):
        GANLoss("mescheder-r1-gp")          # in --gan_mode choices but not implemented, like the reference (loss.py:62)
    with pytest.raises(NotImplementedError):
        GANLoss("nonsense")
    from swapnet_amd import optimizers
    with pytest.raises(ValueError):
        optimizers.define_optimizer(model.net_generator, opt, "X")
    with pytest.raises(RuntimeError):
        model.net_generator.load_state_dict({"bogus": torch.zeros(1)})
    with pytest.raises(RuntimeError):
        create_model(make_opt(tmp_path, backend, gpu_id=None))


def test_gan_label_draw_order_matches_reference(golden_dir):
    """GANLoss draws: fake-D, real-D, real-G, all from U(0.7,1.1) (loss.py:93,102)."""
    from swapnet_amd.modules.loss import GANLoss
    gold = np.load(os.path.join(golden_dir, "warp_step_64.npz"))
    c = GANLoss("vanilla", smooth_labels=True)
    torch.manual_seed(int(gold["meta/step_seeds"][0]))
    got = [c.sample_label(False), c.sample_label(True), c.sample_label(True)]
    np.testing.assert_allclose(got, gold["step0/labels"], rtol=0, atol=1e-7)
    assert all(0.7 <= v <= 1.1 for v in got)
    h = GANLoss("vanilla", smooth_labels=False)
    assert h.sample_label(True) == 1.0 and h.sample_label(False) == 0.0


@pytest.mark.parametrize("backend", BACKENDS)
def test_integer_label_inputs_equal_onehot_inputs(backend, tmp_path):
    """cloth segmentations handed over as the on-disk integer label map
    (datasets/data_utils.py:298-343) and expanded on the device give bit-identical results to the
    reference dataloader's one-hot tensors."""
    from swapnet_amd.models import create_model
    opt = make_opt(tmp_path, backend, is_train=False, batch_size=2)
    model = create_model(opt)
    torch.manual_seed(0)
    model.net_generator.load_state_dict(O.warp_module_params())
    model.eval()
    bodys, inputs, _ = O.synth_warp_batch(2, 64, 64, seed=5)
    labels = O.onehot_to_labels(inputs)                      # (2,64,64) int64; background rows are all-zero -> 0
    assert torch.equal(O.labels_to_onehot(labels, 19), inputs)
    model.set_input(dict(bodys=bodys, input_cloths=inputs, cloth_paths=[""] * 2, body_paths=[""] * 2))
    model.test()
    a = model.fakes.cpu().clone()
    model.set_input(dict(bodys=bodys, input_cloths=labels, cloth_paths=[""] * 2, body_paths=[""] * 2))
    model.test()
    assert torch.equal(a, model.fakes.cpu())


@pytest.mark.parametrize("backend", BACKENDS)
def test_two_stage_device_pipeline_equals_reference_two_pass_inference(backend):
    """inference.py's warp -> .npz (argmax labels) -> texture hand-off, kept in HBM
    (SURVEY.md 8(f) rank 2): equals the oracle's two passes with the label round trip."""
    from swapnet_amd.pipeline import TwoStagePipeline
    ctx = backends.gpu_ctx() if backend == "gpu" else backends.hostsim_ctx()
    torch.manual_seed(3)
    Gw, Gt = O.warp_module_params(), O.texture_module_params(img_size=64)
    bodys, inputs, _ = O.synth_warp_batch(1, 64, 64, seed=9)
    tex, rois, _, _ = O.synth_texture_batch(1, 64, 64, seed=10)
    with torch.no_grad():
        warped = O.warp_module_forward(Gw, bodys, inputs)
        labels = O.onehot_to_labels(warped)                           # what compress_and_save_cloth stores
        cloth = O.labels_to_onehot(labels, 19)                        # what decompress_cloth_segment returns
        ref = O.texture_module_forward(Gt, tex, rois, cloth)
    pipe = TwoStagePipeline(Gw, Gt, img_size=64, ctx=ctx)
    out, lab = pipe(bodys, inputs, tex, rois, return_labels=True)
    # argmax of near-tied tanh outputs may legitimately flip on a handful of pixels (fp32 round-off)
    agree = (lab.cpu().long() == labels).float().mean().item()
    assert agree > 0.999, agree
    # value check, unconditional: the texture stage sees the labels the DEVICE argmax produced, so the oracle's
    # second pass is evaluated on exactly those labels (identical to `labels` except on flipped near-ties)
    with torch.no_grad():
        ref_dev = O.texture_module_forward(Gt, tex, rois, O.labels_to_onehot(lab.cpu().long(), 19))
    assert float((out.cpu() - ref_dev).norm() / ref_dev.norm()) < 1e-3
    if agree == 1.0:
        assert torch.equal(ref_dev, ref)
    # second and third call with OTHER inputs: on the GPU these replay the hipGraph captured by the first call --
    # the replay must read the newly staged inputs and reproduce the eager result bit for bit
    bodys2, inputs2, _ = O.synth_warp_batch(1, 64, 64, seed=19)
    tex2, rois2, _, _ = O.synth_texture_batch(1, 64, 64, seed=20)
    out2, lab2 = pipe(bodys2, inputs2, tex2, rois2, return_labels=True)
    assert pipe.last_call_was_graph_replay == (backend == "gpu")
    eager = TwoStagePipeline(Gw, Gt, img_size=64, ctx=ctx, use_graph=False)
    out2e, lab2e = eager(bodys2, inputs2, tex2, rois2, return_labels=True)
    assert not eager.last_call_was_graph_replay
    assert torch.equal(lab2.cpu(), lab2e.cpu()) and torch.equal(out2.cpu(), out2e.cpu())
    out3 = pipe(bodys, inputs, tex, rois)
    assert torch.equal(out3.cpu(), out.cpu())


@pytest.mark.parametrize("stage", ["warp", "texture"])
def test_seeded_init_equals_the_reference(stage, tmp_path, golden_dir):
    """`torch.manual_seed(s); create_model(opt)` gives the weights the reference
    gives -- the native init consumes the CPU RNG like the reference's constructors + init_weights do
    (construction order, incl. the pix2pix U-Net's inside-out recursion; module-tree order for the
    re-draw).  Against the init weights recorded from the real reference in tests/golden/*_step_64.npz."""
    from swapnet_amd.models import create_model
    gold = np.load(os.path.join(golden_dir, "%s_step_64.npz" % stage))
    opt = make_opt(tmp_path, "sim", model=stage)
    torch.manual_seed(int(gold["meta/init_seed"]))
    model = create_model(opt)
    for net, tag in ((model.net_generator, "G"), (model.net_discriminator, "D")):
        sd = net.state_dict()
        keys = [k[len("init/%s/" % tag):-len("/norm")] for k in gold.files if k.startswith("init/%s/" % tag) and k.endswith("/norm")]
        assert keys and set(keys) == set(sd.keys()), (tag, sorted(set(keys) ^ set(sd.keys()))[:4])
        for k in keys:
            ok, msg = compare(gold, "init/%s/%s" % (tag, k), sd[k], rtol=1e-6, atol_frac=1e-6)
            assert ok, msg
    if stage == "warp":
        # ... and from there one seeded step is the reference's step: nothing was loaded from outside
        model.eval()
        bodys, inputs, targets = O.synth_warp_batch(2, 64, 64, seed=1234)
        model.set_input(dict(bodys=bodys, input_cloths=inputs, target_cloths=targets, cloth_paths=["", ""], body_paths=["", ""]))
        torch.manual_seed(int(gold["meta/step_seeds"][0]))
        model.optimize_parameters()
        for k, v in model.get_current_losses().items():
            ref = float(gold["step0/loss/" + k])
            assert abs(v - ref) <= 1e-3 * abs(ref) + 1e-6, (k, v, ref)


def test_seeded_init_matches_oracle_for_the_8_level_unet(tmp_path):
    """Same property at the C3 size (crop 256: 8 U-Net levels, inside-out construction order) against the
    oracle's RNG-faithful builder (itself pinned to the reference at 64x64): exact equality."""
    from swapnet_amd.models import create_model
    opt = make_opt(tmp_path, "sim", model="texture", crop_size=256, batch_size=1)
    torch.manual_seed(11)
    model = create_model(opt)
    torch.manual_seed(11)
    G, D = O.texture_module_params(img_size=256), O.patchgan_params(22)
    sg, sd = model.net_generator.state_dict(), model.net_discriminator.state_dict()
    assert list(sg.keys()) == list(G.keys()) and list(sd.keys()) == list(D.keys())
    assert all(torch.equal(sg[k].cpu(), G[k]) for k in G)
    assert all(torch.equal(sd[k].cpu(), D[k]) for k in D)


def test_optimizer_param_groups_are_live_and_per_network(tmp_path):
    """editing optimizer.param_groups (what an lr scheduler does) must reach the native step, and
    the two optimizers keep separate betas (loading optimizer_D's state must not overwrite G's)."""
    from swapnet_amd.models import create_model
    opt = make_opt(tmp_path, "sim")
    model = create_model(opt)
    model.eval()
    bodys, inputs, targets = O.synth_warp_batch(2, 64, 64, seed=1234)
    data = dict(bodys=bodys, input_cloths=inputs, target_cloths=targets, cloth_paths=["", ""], body_paths=["", ""])
    model.set_input(data)
    g0 = model.net_generator.state_dict()["upsample_and_pad.2.weight"].clone()
    d0 = model.net_discriminator.state_dict()["model.0.weight"].clone()
    model.optimizer_G.param_groups[0]["lr"] = 0.0                 # scheduler-style edit
    torch.manual_seed(1)
    model.optimize_parameters()
    assert torch.equal(model.net_generator.state_dict()["upsample_and_pad.2.weight"], g0)      # lr 0: G frozen
    assert not torch.equal(model.net_discriminator.state_dict()["model.0.weight"], d0)         # D still trains
    model.optimizer_G.param_groups[0]["lr"] = 1e-4
    torch.manual_seed(2)
    model.optimize_parameters()
    assert not torch.equal(model.net_generator.state_dict()["upsample_and_pad.2.weight"], g0)
    # separate betas: D's state dict with other betas leaves G's hyper-parameters alone
    sd = model.optimizer_D.state_dict()
    sd["param_groups"][0]["betas"] = (0.5, 0.9)
    model.optimizer_D.load_state_dict(sd)
    h = model.backend.hyper
    assert (h["d_b1"], h["d_b2"]) == (0.5, 0.9) and (h["b1"], h["b2"]) == (0.9, 0.999)
    assert model.optimizer_G.state_dict()["param_groups"][0]["betas"] == (0.9, 0.999)


def test_ce_mode_draws_no_labels_and_skips_D(tmp_path):
    """--warp_mode ce (warp_model.py:169-183): generator only; GANLoss is never called, so the global RNG is not
    consumed (a seeded run stays aligned with the reference) and the discriminator is untouched."""
    from swapnet_amd.models import create_model
    opt = make_opt(tmp_path, "sim", warp_mode="ce")
    model = create_model(opt)
    model.eval()
    bodys, inputs, targets = O.synth_warp_batch(2, 64, 64, seed=1234)
    model.set_input(dict(bodys=bodys, input_cloths=inputs, target_cloths=targets, cloth_paths=["", ""], body_paths=["", ""]))
    d0 = {k: v.clone() for k, v in model.net_discriminator.state_dict().items()}
    torch.manual_seed(5)
    model.optimize_parameters()
    nxt = torch.rand(1)
    torch.manual_seed(5)
    assert torch.equal(nxt, torch.rand(1))                        # no draws happened
    assert all(torch.equal(v, d0[k]) for k, v in model.net_discriminator.state_dict().items())


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_model_of_another_batch_size_shares_the_training_state(backend):
    """swn_model_create_shared (round 4): the model NativeBackend builds for an epoch's last, smaller batch
    uses the first model's parameter arenas instead of a second copy of weights, gradients and Adam moments plus transfers.
    One step on the small model IS a step of the shared state (same memory, same counters); it allocates far less than a
    model of its own; and it keeps working after the sharer's handle is gone."""
    from oracle import swapnet_oracle as O
    from swapnet_amd import engine
    ctx = backends.gpu_ctx() if backend == "gpu" else backends.hostsim_ctx()
    torch.manual_seed(1)
    G, D = O.warp_module_params(), O.patchgan_params(22)
    root = engine.NativeModel(ctx, "warp", 2, 64, 64)
    backends.reset_state(root, {engine.NET_G: G, engine.NET_D: D})
    before = ctx.bytes_allocated()
    small = engine.NativeModel(ctx, "warp", 1, 64, 64, share=root)
    added_shared = ctx.bytes_allocated() - before
    own = engine.NativeModel(ctx, "warp", 1, 64, 64)
    added_own = ctx.bytes_allocated() - before - added_shared
    try:
        # same memory: the arenas of the sharing model ARE the sharer's
        for net in (engine.NET_G, engine.NET_D):
            for which in (engine.W_WEIGHT, engine.W_GRAD, engine.W_EXP_AVG, engine.W_EXP_AVG_SQ):
                assert small.arena(net, which).data_ptr() == root.arena(net, which).data_ptr()
                assert own.arena(net, which).data_ptr() != root.arena(net, which).data_ptr()
        # a step on the small model against the same step on an independent model loaded with the same state
        backends.reset_state(own, {engine.NET_G: G, engine.NET_D: D})
        batch = O.synth_warp_batch(1, 64, 64, seed=3)
        for m in (small, own):
            m.set_hyper()
            for i, t in enumerate(batch):
                m.set_input(i, t)
            m.step([0.9, 0.8, 1.0], training=False, seed=0)
        assert small.losses() == own.losses()
        assert torch.equal(root.arena(engine.NET_G, engine.W_WEIGHT).cpu(), own.arena(engine.NET_G, engine.W_WEIGHT).cpu())
        assert root.optim_step_count(engine.NET_G) == 1 and root.optim_step_count(engine.NET_D) == 1
        # ... and the sharer trains on from there at its own batch size
        b2 = O.synth_warp_batch(2, 64, 64, seed=4)
        for i, t in enumerate(b2):
            root.set_input(i, t)
        root.step([0.9, 0.8, 1.0], training=False, seed=0)
        assert small.optim_step_count(engine.NET_G) == 2
        # the sharing model holds the shared buffers alive
        w = small.arena(engine.NET_G, engine.W_WEIGHT).clone()
        root.close()
        for i, t in enumerate(batch):
            small.set_input(i, t)
        small.step([0.9, 0.8, 1.0], training=False, seed=0)
        assert small.optim_step_count(engine.NET_G) == 3
        assert not torch.equal(small.arena(engine.NET_G, engine.W_WEIGHT), w)
        # footprint: activations and derived operands only -- no second set of four arenas (2.2 GB of the warp stage's ~2.25 GB state)
        state_bytes = 4 * 4 * (small.arena(engine.NET_G, engine.W_WEIGHT).numel() + small.arena(engine.NET_D, engine.W_WEIGHT).numel())
        assert 0 < added_shared <= added_own - 0.99 * state_bytes, (added_shared, added_own, state_bytes)
        print("shared model added %.1f MB, an independent one %.1f MB; four arenas of both networks are %.1f MB"
              % (added_shared / 1e6, added_own / 1e6, state_bytes / 1e6))
    finally:
        small.close(); own.close(); root.close()
