"""--monitor_ssim WINDOW of the training TextureModel: 'ssim' joins loss_names and get_current_losses() reports the mean SSIM loss of
the fakes against the targets (max_val 2.0, the tanh range), evaluated when the losses are read; without the option nothing changes."""
import warnings

import pytest
import torch

from oracle import swapnet_oracle as O
from tests.test_models_api import BACKENDS, make_opt

pytestmark = pytest.mark.small_channel_winograd      # tests/conftest.py: small shapes on the Winograd forms

TODAY = ["D", "D_real", "D_fake", "G", "G_gan", "G_l1"]           # (the perceptual terms are off: the VGG16 passes are most of a small step)


def _model(tmp_path, backend, **kw):
    from swapnet_amd.models import create_model
    opt = make_opt(tmp_path, backend, model="texture", lambda_content=0.0, lambda_style=0.0, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (seeded-random VGG16: no weights file in the test environment)
        torch.manual_seed(3)
        model = create_model(opt)
    model.setup(opt)
    return model


@pytest.mark.parametrize("backend", BACKENDS)
def test_monitor_ssim_reports_the_mean_ssim_loss(backend, tmp_path):
    from swapnet_amd.modules.losses import SSIM
    model = _model(tmp_path, backend, monitor_ssim=5)
    assert model.loss_names == TODAY + ["ssim"]
    tex, rois, cloths, tgt = O.synth_texture_batch(1, 64, 64, seed=21)
    model.set_input(dict(input_textures=tex, rois=rois, cloths=cloths, target_textures=tgt, cloth_paths=["c"], texture_paths=["t"]))
    torch.manual_seed(5)
    model.optimize_parameters()
    assert model.loss_ssim == 0.0                                     # not evaluated on the step path: only when the losses are read
    losses = model.get_current_losses()
    assert list(losses) == model.loss_names
    fakes, targets = model.fakes, model.targets
    want = SSIM(5, "mean", 2.0)(fakes, targets.to(fakes.device))     # the module: kernels on the device, the torch branch on the CPU
    print("%s ssim %.6f (module %.6f)" % (backend, losses["ssim"], float(want)))
    assert 0.0 < losses["ssim"] <= 0.5
    assert abs(losses["ssim"] - float(want)) <= 1e-5 * float(want)
    assert model.get_current_losses() == losses                       # reading again changes nothing


def test_without_the_option_nothing_changes(tmp_path):
    model = _model(tmp_path, "sim")
    assert model.loss_names == TODAY and not hasattr(model, "loss_ssim")
    with pytest.raises(ValueError, match="odd window"):
        _model(tmp_path, "sim", monitor_ssim=4)
    from swapnet_amd.models.texture_model import TextureModel
    import argparse
    p = TextureModel.modify_commandline_options(argparse.ArgumentParser(), True)
    assert p.get_default("monitor_ssim") == 0
