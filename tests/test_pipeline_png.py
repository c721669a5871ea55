"""The PNG files of the two-stage pipeline's image sheet (swn_pipeline_enable_png / swn_pipeline_png, TwoStagePipeline(images=dict(...,
png=True)).images_png()): Pillow opens every file to exactly the array images() returns, the files come out of the replayed graph, and
arming the PNG launches changes nothing the pipeline computed without them."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import swapnet_oracle as O              # seeded weights and batches only
from swapnet_amd import engine
from swapnet_amd.util.draw_rois import BODY_COLORS
from tests import backends

pytestmark = pytest.mark.small_channel_winograd      # tests/conftest.py: small shapes on the Winograd forms

BODY_STATS = ((0.4, 0.5, 0.45), (0.3, 0.25, 0.2))
TEX_STATS = ((0.5, 0.45, 0.4), (0.2, 0.3, 0.25))
B, S = 2, 64
NAMES = ["inputs_decoded", "bodys_unnormalized", "fakes_decoded", "textures_unnormalized", "fakes", "fakes_scaled", "cloths_decoded"]


def _inputs(seed):
    bodys, inputs, _ = O.synth_warp_batch(B, S, S, seed=seed)
    tex, rois, _, _ = O.synth_texture_batch(B, S, S, seed=seed + 1)
    return bodys, inputs, tex, rois


def assert_files_decode_to(files, sheet, what):
    assert list(files) == NAMES, list(files)
    for k in NAMES:
        assert len(files[k]) == B and all(isinstance(f, bytes) for f in files[k]), (what, k)
        for b in range(B):
            im = Image.open(io.BytesIO(files[k][b]))
            im.load()
            print("%s %s[%d]: %d bytes" % (what, k, b, len(files[k][b])))
            assert im.mode == "RGB" and im.size == (S, S), (what, k, b)
            assert np.array_equal(np.asarray(im), sheet[k][b]), (what, k, b)


@pytest.mark.gpu
def test_pipeline_pngs_decode_to_the_image_sheet_and_leave_the_pipeline_alone():
    from swapnet_amd.pipeline import TwoStagePipeline
    ctx = backends.gpu_ctx()
    torch.manual_seed(3)
    Gw, Gt = O.warp_module_params(), O.texture_module_params(img_size=S)
    a, b = _inputs(9), _inputs(19)
    stats = dict(body_norm_stats=BODY_STATS, texture_norm_stats=TEX_STATS)
    png = TwoStagePipeline(Gw, Gt, img_size=S, ctx=ctx, images=dict(png=True, **stats))
    plain = TwoStagePipeline(Gw, Gt, img_size=S, ctx=ctx, images=dict(stats))
    with pytest.raises(ValueError, match="unknown"):
        TwoStagePipeline(Gw, Gt, img_size=S, ctx=ctx, images=dict(pngs=True, **stats))
    with pytest.raises(ValueError, match="call the pipeline first"):
        png.images_png()
    runs = []
    for i in range(3):                                       # eager (and capturing), replay, replay
        out, lab = png(*a, return_labels=True)
        assert png.last_call_was_graph_replay == (i > 0), i
        runs.append((out.cpu().clone(), lab.cpu().clone(), png.images(), png.images_png()))
    for i, (out, lab, sheet, files) in enumerate(runs):
        assert_files_decode_to(files, sheet, "run %d" % i)
        assert files == runs[0][3], "the replayed graph writes the same files"
    assert runs[0][3]["cloths_decoded"] is runs[0][3]["fakes_decoded"]
    # other inputs through the replayed graph: the files are not constants of the capture
    out_b, lab_b = png(*b, return_labels=True)
    assert png.last_call_was_graph_replay
    files_b = png.images_png()
    assert_files_decode_to(files_b, png.images(), "other inputs")
    assert files_b["fakes"] != runs[0][3]["fakes"]
    # float outputs, labels and images() are bit-equal to a pipeline armed with images only
    for inp, (o_png, l_png, sheet_png) in ((a, runs[0][:3]), (b, (out_b.cpu(), lab_b.cpu(), png.images()))):
        o_plain, l_plain = plain(*inp, return_labels=True)
        assert torch.equal(o_plain.cpu(), o_png) and torch.equal(l_plain.cpu(), l_png)
        sheet_plain = plain.images()
        for k in NAMES:
            assert np.array_equal(sheet_plain[k], sheet_png[k]), k
    with pytest.raises(ValueError, match="png=True"):
        plain.images_png()


@pytest.mark.gpu
def test_enable_png_needs_the_image_sheet_and_captures_again():
    ctx = backends.gpu_ctx()
    torch.manual_seed(4)
    Gw, Gt = O.warp_module_params(), O.texture_module_params(img_size=S)
    warp = engine.NativeModel(ctx, "warp", B, S, S, is_train=False)
    tex = engine.NativeModel(ctx, "texture", B, S, S, is_train=False)
    warp.load_state_dict(engine.NET_G, Gw)
    tex.load_state_dict(engine.NET_G, Gt)
    pipe = engine.NativePipeline(warp, tex)
    bodys, inputs, textures, rois = _inputs(29)
    warp.set_input(0, bodys); warp.set_input(1, inputs); tex.set_input(0, textures); tex.set_input(1, rois)
    with pytest.raises(ValueError, match="swn_pipeline_enable_images"):
        pipe.enable_png()
    with pytest.raises(ValueError, match="not armed"):
        pipe.png()
    pipe.enable_images(BODY_STATS, TEX_STATS, BODY_COLORS, 1)
    assert [pipe.run(True) for _ in range(2)] == [False, True]
    sheet = pipe.images()
    with pytest.raises(ValueError):
        pipe.enable_png(700)                                 # 700 rows of 193 bytes: beyond a chunk
    pipe.enable_png()
    assert [pipe.run(True) for _ in range(3)] == [False, True, True]        # eager and capturing again, then replays
    files = pipe.png()
    assert list(files) == list(engine.IMAGE_NAMES)
    for k in files:
        assert np.array_equal(pipe.images()[k], sheet[k]), k
        for i in range(B):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[k][i]))), sheet[k][i]), (k, i)
    pipe.enable_png(5)                                       # arming again: other chunks, captured again, the same images
    assert [pipe.run(True) for _ in range(2)] == [False, True]
    files5 = pipe.png()
    for k in files5:
        for i in range(B):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(files5[k][i]))), sheet[k][i]), (k, i)
    assert files5 != files
    pipe.close(); warp.close(); tex.close()


def test_the_host_simulator_refuses_the_pipeline_png_by_name():
    ctx = backends.hostsim_ctx()
    warp = engine.NativeModel(ctx, "warp", 1, 64, 64, is_train=False)
    tex = engine.NativeModel(ctx, "texture", 1, 64, 64, is_train=False)
    pipe = engine.NativePipeline(warp, tex)
    with pytest.raises(ValueError, match="swn_pipeline_enable_images"):
        pipe.enable_png()
    pipe.enable_images(BODY_STATS, TEX_STATS, BODY_COLORS, 1)
    with pytest.raises(NotImplementedError, match="simulator"):
        pipe.enable_png()
    pipe.close(); warp.close(); tex.close()
