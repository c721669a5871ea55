"""UnetGenerator with the reference's constructor + forward signature (modules/pix2pix_modules.py:113-177), executed by the
HIP library: the plain pix2pix U-Net (Isola et al. 2017) that the texture stage's --netG unet_128 trains as the baseline of the
ROI-pooled TextureModule.

Standalone use (inference, parity tests):
    net = UnetGenerator(3, 3, 7, 64, norm_layer="batch", use_dropout=True)
    net.load_state_dict(torch.load("latest_net_generator.pth"))     # reference checkpoint keys (model.model.0.weight, ...)
    fakes = net.eval()(textures)                                    # (B,3,H,W) in (-1,1), H = W in {128, 256}
Inside TextureModel the same object is a view onto the model's NativeBackend.
"""
import torch

from .. import engine
from .native import NativeBackend, NativeNet


def _norm_name(norm_layer):
    """"batch" / "instance" / "none", or torch's layer classes (functools.partial of them included), by name."""
    if isinstance(norm_layer, str):
        return norm_layer
    fn = getattr(norm_layer, "func", norm_layer)
    return {"BatchNorm2d": "batch", "InstanceNorm2d": "instance", "Identity": "none"}.get(getattr(fn, "__name__", ""), repr(norm_layer))


class UnetGenerator(NativeNet):
    """Seven UnetSkipConnectionBlocks, ngf 64, BatchNorm2d (no conv bias but the outermost transposed conv's), Dropout(0.5)
    behind the upnorm of the two inner ngf*8 blocks.  Only that configuration -- the one --netG unet_128 builds -- is native."""

    def __init__(self, input_nc, output_nc, num_downs, ngf=64, norm_layer="batch", use_dropout=False, backend=None, lib=None,
                 img_size=128):
        got = (input_nc, output_nc, num_downs, ngf, _norm_name(norm_layer), bool(use_dropout))
        if got != (3, 3, 7, 64, "batch", True):
            raise NotImplementedError("UnetGenerator(input_nc=%s, output_nc=%s, num_downs=%s, ngf=%s, norm_layer=%s, use_dropout=%s) "
                                      "is not implemented: the native builder is (3, 3, 7, 64, batch, True), --netG unet_128" % got)
        if backend is not None and backend.kind != "texture":
            raise ValueError("UnetGenerator on a backend of the %s stage" % backend.kind)
        if backend is not None and backend.models and backend.netG != "unet_128":
            raise ValueError("UnetGenerator on a backend whose generator is already built as %s" % backend.netG)
        backend = backend or NativeBackend("texture", is_train=False, lib=lib, default_shape=(1, img_size, img_size))
        backend.netG = "unet_128"           # the stage's native networks are built together, on first use
        super().__init__(backend, engine.NET_G)
        self.training = True

    def load_state_dict(self, state_dict, strict=True):
        foreign = [k for k in state_dict if k.startswith("unet.") or k.startswith("encode.")]
        if foreign:
            raise RuntimeError("Error(s) in loading state_dict for UnetGenerator: this is a TextureModule checkpoint (--netG swapnet), "
                               "unexpected keys %s" % foreign)
        return super().load_state_dict(state_dict, strict=strict)

    def forward(self, textures):
        B, _, H, W = textures.shape
        m = self._backend.ensure(B, H, W)
        m.set_input(0, textures)
        m.forward(training=self.training, seed=int(torch.randint(0, 2 ** 31 - 1, (1,))) if self.training else 0)
        return m.output()
