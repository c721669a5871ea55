"""The image sheet of the two-stage pipeline (swn_pipeline_enable_images / swn_pipeline_images) and BaseModel.get_current_images():
every image equals engine.op_image_u8 applied to the tensors it is made from (tests/test_image_out.py pins that op to the reference's
host chain), arming changes nothing the pipeline computed before, and on the device the images come out of the replayed graph."""
import argparse

import numpy as np
import pytest
import torch

from oracle import swapnet_oracle as O              # seeded weights and batches only
from swapnet_amd import engine
from swapnet_amd.util.draw_rois import BODY_COLORS
from tests import backends

pytestmark = pytest.mark.small_channel_winograd      # tests/conftest.py: small shapes on the Winograd forms

BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]
BODY_STATS = ((0.4, 0.5, 0.45), (0.3, 0.25, 0.2))
TEX_STATS = ((0.5, 0.45, 0.4), (0.2, 0.3, 0.25))
B, S = 2, 64
NAMES = ["inputs_decoded", "bodys_unnormalized", "fakes_decoded", "textures_unnormalized", "fakes", "fakes_scaled", "cloths_decoded"]


def _ctx(backend):
    return backends.gpu_ctx() if backend == "gpu" else backends.hostsim_ctx()


def _np(t):
    return t.cpu().numpy()


def _inputs(seed):
    bodys, inputs, _ = O.synth_warp_batch(B, S, S, seed=seed)
    tex, rois, _, _ = O.synth_texture_batch(B, S, S, seed=seed + 1)
    return bodys, inputs, tex, rois


def expected_sheet(ctx, bodys, inputs, tex, rois, out, lab):
    """The sheet from the op, applied to the staged inputs and to the pipeline's own output() / labels()."""
    width = int(round(0.01 * S))
    return {"inputs_decoded": _np(engine.op_image_u8(ctx, inputs, source=engine.SRC_ARGMAX)),
            "bodys_unnormalized": _np(engine.op_image_u8(ctx, bodys, rows=engine.image_rows(B, 3, *BODY_STATS))),
            "fakes_decoded": _np(engine.op_image_u8(ctx, labels=lab)),
            "cloths_decoded": _np(engine.op_image_u8(ctx, labels=lab)),
            "textures_unnormalized": _np(engine.op_image_u8(ctx, tex, rows=engine.image_rows(B, 3, *TEX_STATS), rois=rois, colours=BODY_COLORS,
                                                            width=width)),
            "fakes": _np(engine.op_image_u8(ctx, out)),
            "fakes_scaled": _np(engine.op_image_u8(ctx, out, scale_each=True))}


def assert_sheet(got, want, what):
    assert list(got) == NAMES, list(got)
    for k in NAMES:
        assert got[k].shape == (B, S, S, 3) and got[k].dtype == np.uint8, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("backend", BACKENDS)
def test_pipeline_images_equal_the_op_and_leave_the_pipeline_alone(backend):
    from swapnet_amd.pipeline import TwoStagePipeline
    ctx = _ctx(backend)
    torch.manual_seed(3)
    Gw, Gt = O.warp_module_params(), O.texture_module_params(img_size=S)
    a, b = _inputs(9), _inputs(19)
    armed = TwoStagePipeline(Gw, Gt, img_size=S, ctx=ctx, images=dict(body_norm_stats=BODY_STATS, texture_norm_stats=TEX_STATS))
    plain = TwoStagePipeline(Gw, Gt, img_size=S, ctx=ctx)
    with pytest.raises(ValueError, match="without images"):
        plain.images()
    with pytest.raises(ValueError, match="call the pipeline first"):
        armed.images()
    # three runs on the same inputs: eager (and capturing), replay, replay
    sheets, outs = [], []
    for i in range(3):
        out, lab = armed(*a, return_labels=True)
        outs.append((out.cpu().clone(), lab.cpu().clone()))
        sheets.append(armed.images())
        assert armed.last_call_was_graph_replay == (backend == "gpu" and i > 0), i
    assert armed.last_call_was_graph_replay == (backend == "gpu")          # the third run is a replay
    want = expected_sheet(ctx, *a, *outs[0])
    for i, sheet in enumerate(sheets):
        assert_sheet(sheet, want, "run %d" % i)
        assert torch.equal(outs[i][0], outs[0][0]) and torch.equal(outs[i][1], outs[0][1])
    assert sheets[0]["cloths_decoded"] is sheets[0]["fakes_decoded"]
    # the images are not constants of the capture: other inputs through the replayed graph
    out_b, lab_b = armed(*b, return_labels=True)
    assert armed.last_call_was_graph_replay == (backend == "gpu")
    sheet_b = armed.images()
    assert_sheet(sheet_b, expected_sheet(ctx, *b, out_b, lab_b), "other inputs")
    assert not np.array_equal(sheet_b["fakes"], sheets[0]["fakes"])
    # output() and labels() are bit-identical to an un-armed pipeline on the same inputs
    for inp, (o_armed, l_armed) in ((a, outs[0]), (b, (out_b.cpu(), lab_b.cpu()))):
        o_plain, l_plain = plain(*inp, return_labels=True)
        assert torch.equal(o_plain.cpu(), o_armed) and torch.equal(l_plain.cpu(), l_armed)
    # the outlines are there, and the decoded labels are the warped ones
    assert (sheets[0]["textures_unnormalized"] != _np(engine.op_image_u8(ctx, a[2], rows=engine.image_rows(B, 3, *TEX_STATS)))).any()
    # a reversed box is Pillow's ValueError, before anything runs
    bad = a[3].clone()
    bad[0, 0] = torch.tensor([9., 2., 3., 8.])
    with pytest.raises(ValueError, match="x1 must be greater"):
        armed(a[0], a[1], a[2], bad)


@pytest.mark.parametrize("backend", BACKENDS)
def test_arming_after_the_capture_captures_again(backend):
    ctx = _ctx(backend)
    torch.manual_seed(4)
    Gw, Gt = O.warp_module_params(), O.texture_module_params(img_size=S)
    warp = engine.NativeModel(ctx, "warp", B, S, S, is_train=False)
    tex = engine.NativeModel(ctx, "texture", B, S, S, is_train=False)
    warp.load_state_dict(engine.NET_G, Gw)
    tex.load_state_dict(engine.NET_G, Gt)
    pipe = engine.NativePipeline(warp, tex)
    bodys, inputs, textures, rois = _inputs(29)
    warp.set_input(0, bodys); warp.set_input(1, inputs); tex.set_input(0, textures); tex.set_input(1, rois)
    gpu = backend == "gpu"
    with pytest.raises(ValueError, match="not armed"):
        pipe.images()
    assert [pipe.run(True) for _ in range(2)] == [False, gpu]             # captured by the first call, replayed by the second
    out0, lab0 = tex.output().cpu(), pipe.labels().cpu()
    with pytest.raises(ValueError, match="colours"):
        pipe.enable_images(BODY_STATS, TEX_STATS, BODY_COLORS[:5], 1)
    pipe.enable_images(BODY_STATS, TEX_STATS, BODY_COLORS, 1)
    assert [pipe.run(True) for _ in range(3)] == [False, gpu, gpu]        # eager and capturing again, then replays
    assert torch.equal(tex.output().cpu(), out0) and torch.equal(pipe.labels().cpu(), lab0)
    want = expected_sheet(ctx, bodys, inputs, textures, rois, out0, lab0)
    got = pipe.images()
    assert list(got) == NAMES[:6] == list(engine.IMAGE_NAMES)
    for k in got:
        assert np.array_equal(got[k], want[k]), k
    # arming twice is fine: new tables (per-channel un-normalisation, wider outlines), captured again
    pipe.enable_images(BODY_STATS, TEX_STATS, BODY_COLORS[::-1].copy(), 2, reference_quirk=False)
    assert [pipe.run(True) for _ in range(3)] == [False, gpu, gpu]
    got = pipe.images()
    rows = engine.image_rows(B, 3, *TEX_STATS, reference_quirk=False)
    assert np.array_equal(got["textures_unnormalized"], _np(engine.op_image_u8(ctx, textures, rows=rows, rois=rois, colours=BODY_COLORS[::-1].copy(), width=2)))
    assert np.array_equal(got["bodys_unnormalized"], _np(engine.op_image_u8(ctx, bodys, rows=engine.image_rows(B, 3, *BODY_STATS, reference_quirk=False))))
    assert np.array_equal(got["fakes_scaled"], want["fakes_scaled"])
    pipe.close(); warp.close(); tex.close()


def _opt(tmp, backend, **kw):
    lib = backends.hostsim_ctx().lib if backend == "sim" else None
    if backend == "gpu":
        backends.gpu_ctx()
    o = dict(gpu_id=0, is_train=True, checkpoints_dir=str(tmp), name="t", no_confirm=True, model="warp",
             body_channels=12, body_representation="rgb", cloth_channels=19, cloth_representation="labels",
             texture_channels=3, init_type="kaiming", init_gain=0.02, discriminator="basic", n_layers_D=3,
             norm="instance", gan_label_mode="smooth", gan_mode="vanilla", lambda_discriminator=1.0, lambda_gan=1.0,
             lambda_gp=10, optimizer_G="AdamW", optimizer_D="AdamW", lr=1e-4, d_lr=4e-4, weight_decay=0.0,
             d_weight_decay=0.01, b1=0.9, b2=0.999, beta1=0.5, verbose=False, continue_train=False,
             load_epoch="latest", batch_size=B, crop_size=S, warp_mode="gan", lambda_ce=100.0,
             body_norm_stats=BODY_STATS, texture_norm_stats=TEX_STATS,
             netG="swapnet", lambda_l1=10.0, lambda_content=20.0, lambda_style=1e-8, _swapnet_lib=lib)
    o.update(kw)
    return argparse.Namespace(**o)


def _visuals_snapshot(model):
    return {k: (v.clone() if torch.is_tensor(v) else np.array(v)) for k, v in model.get_current_visuals().items()}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("is_train", [False, True], ids=["inference", "train"])
@pytest.mark.parametrize("stage", ["warp", "texture"])
def test_get_current_images_equals_the_op_on_the_models_tensors(backend, stage, is_train, tmp_path):
    from swapnet_amd.models import create_model
    opt = _opt(tmp_path, backend, model=stage, is_train=is_train)
    torch.manual_seed(5)
    model = create_model(opt)
    ctx = model.backend.ctx
    model.eval()
    if stage == "warp":
        bodys, inputs, targets = O.synth_warp_batch(B, S, S, seed=31)
        labels = O.onehot_to_labels(inputs).int()
        data = dict(bodys=bodys, input_cloths=labels, target_cloths=targets, cloth_paths=[""] * B, body_paths=[""] * B)     # a label map and a one-hot map
        if not is_train:
            model.net_generator.load_state_dict(O.warp_module_params())
    else:
        tex, rois, cloths, targets = O.synth_texture_batch(B, S, S, seed=32)
        data = dict(input_textures=tex, rois=rois, cloths=cloths, target_textures=targets, cloth_paths=[""] * B, texture_paths=[""] * B)
        if not is_train:
            model.net_generator.load_state_dict(O.texture_module_params(img_size=S))
    model.set_input(data)
    model.test()                                      # forward + compute_visuals
    before = _visuals_snapshot(model)
    images = model.get_current_images()
    if stage == "warp":
        want = {"inputs_decoded": engine.op_image_u8(ctx, labels=labels),
                "bodys_unnormalized": engine.op_image_u8(ctx, bodys, rows=engine.image_rows(B, 3, *BODY_STATS)),
                "fakes_decoded": engine.op_image_u8(ctx, model.fakes, source=engine.SRC_ARGMAX)}
        if is_train:
            want["targets_decoded"] = engine.op_image_u8(ctx, targets, source=engine.SRC_ARGMAX)
    else:
        rows = engine.image_rows(B, 3, *TEX_STATS)
        want = {"textures_unnormalized": engine.op_image_u8(ctx, tex, rows=rows, rois=rois, colours=BODY_COLORS, width=1),
                "cloths_decoded": engine.op_image_u8(ctx, cloths, source=engine.SRC_ARGMAX),
                "fakes": engine.op_image_u8(ctx, model.fakes),
                "fakes_scaled": engine.op_image_u8(ctx, model.fakes, scale_each=True)}
        if is_train:
            want["targets_unnormalized"] = engine.op_image_u8(ctx, targets, rows=rows)
        # the overlay compute_visuals() leaves out is drawn
        assert (images["textures_unnormalized"] != _np(engine.op_image_u8(ctx, tex, rows=rows))).any()
    assert list(images) == list(want) == list(model.visual_names)
    for k, v in images.items():
        assert isinstance(v, np.ndarray) and v.shape == (B, S, S, 3) and v.dtype == np.uint8, k
        assert np.array_equal(v, _np(want[k])), k
    # the decoded visuals agree with the host visuals, which are NCHW
    for k in before:
        if k.endswith("_decoded"):
            assert np.array_equal(images[k], before[k].numpy().transpose(0, 2, 3, 1)), k
    # get_current_visuals() is unchanged by the call: same keys, types and values
    after = model.get_current_visuals()
    assert list(after) == list(before)
    for k, v in after.items():
        assert type(v) is type(model.get_current_visuals()[k]) and torch.is_tensor(v) and torch.equal(v, before[k]), k
