"""PatchGAN discriminator factory with the reference's signature
(/root/reference/modules/discriminators.py:45-136).  Inside a model step the native PatchGAN runs
fused on the zero-copy cat of condition and generator output; the module object is the parameter /
checkpoint view of it and `net(x)` evaluates it standalone through swn_model_discriminate."""
from .. import engine
from .native import NativeNet


def _bind_norm(backend, norm_layer):
    """The discriminator's norm layer (get_norm_layer's name: instance | batch | none) becomes a property of the stage's native
    networks, like n_layers_D.  batch / none: the convs in front of a norm layer have no bias (:104-107,151-154); batch: every norm
    site owns weight, bias and the running buffers (state-dict keys model.K.* / net.3.*).  On the host simulator warp stage only:
    the flag also selects the norm layer of the texture stage's U-Net generator, which is under batch / none in the device library."""
    if norm_layer not in engine.NORM_KINDS:
        raise NotImplementedError("normalization layer [%s] is not found" % norm_layer)
    if norm_layer != "instance" and backend.kind != "warp" and not backend.ctx.lib.is_device:
        raise NotImplementedError("normalization layer [%s] is not implemented for the texture stage: its U-Net generator takes "
                                  "the same norm layer and exists under instance norm only" % norm_layer)
    if backend.models and backend.norm != norm_layer:
        raise RuntimeError("the stage's networks already exist with norm = %s" % backend.norm)
    backend.norm = norm_layer


class NLayerDiscriminator(NativeNet):
    """PatchGAN with `n_layers` stride-2 levels (3 = the 70x70 "basic" one), ndf=64 (:91-136); norm_layer instance (bias on every
    conv), batch or none.  ndf is fixed at 64 as in the reference's only call site (models/base_gan.py:147)."""

    def __init__(self, backend, input_nc=22, ndf=64, n_layers=3, norm_layer="instance"):
        want = backend.cloth_channels + (backend.body_channels if backend.kind == "warp" else 3)
        if input_nc != want or ndf != 64:
            raise NotImplementedError("native PatchGAN: ndf 64, input channels = the stage's conditional "
                                      "input (%d here), got input_nc=%d ndf=%d" % (want, input_nc, ndf))
        if not 1 <= int(n_layers) <= 5:
            raise NotImplementedError("native PatchGAN: n_layers_D in [1, 5], got %d" % n_layers)
        if backend.models and backend.n_layers_D != int(n_layers):
            raise RuntimeError("the stage's networks already exist with n_layers_D = %d" % backend.n_layers_D)
        backend.n_layers_D = int(n_layers)
        _bind_norm(backend, norm_layer)
        super().__init__(backend, engine.NET_D)

    def forward(self, input):
        """NLayerDiscriminator.forward (:134-136): `input` = the conditioned batch in the reference's channel
        order, (B, 22, H, W) -> prediction map (B, 1, (H >> n_layers) - 2, (W >> n_layers) - 2).  Forward-only call on the current
        weights (inside a training step the discriminator runs fused in model.backward_D / backward_G); honours
        self.training like the torch module (BatchNorm: batch statistics and a running update in train mode)."""
        b, c, h, w = input.shape
        m = self._backend.ensure(b, h, w)
        return m.discriminate(input, training=self.training)

    __call__ = forward


class PixelDiscriminator(NativeNet):
    """1x1 PatchGAN ("pixelGAN", :139-175): Conv1x1(input_nc, 64) - LeakyReLU - Conv1x1(64, 128) - InstanceNorm - LeakyReLU -
    Conv1x1(128, 1); every conv carries a bias under instance norm (:152-155); state_dict keys net.{0,2,5}.{weight,bias}.  On the
    native side it is PatchGAN "depth 0" of the stage's context (swn_ctx_set_patchgan_layers(ctx, 0))."""

    def __init__(self, backend, input_nc=22, ndf=64, norm_layer="instance"):
        want = backend.cloth_channels + (backend.body_channels if backend.kind == "warp" else 3)
        if input_nc != want or ndf != 64:
            raise NotImplementedError("native PixelDiscriminator: ndf 64, input channels = the stage's conditional "
                                      "input (%d here), got input_nc=%d ndf=%d" % (want, input_nc, ndf))
        if backend.models and backend.n_layers_D != 0:
            raise RuntimeError("the stage's networks already exist with n_layers_D = %d" % backend.n_layers_D)
        backend.n_layers_D = 0
        _bind_norm(backend, norm_layer)
        super().__init__(backend, engine.NET_D)

    def forward(self, input):
        """PixelDiscriminator.forward (:172-174): (B, input_nc, H, W) -> (B, 1, H, W).  Inference-only call on the current weights."""
        b, c, h, w = input.shape
        return self._backend.ensure(b, h, w).discriminate(input, training=self.training)

    __call__ = forward


def define_D(input_nc, ndf, netD, n_layers_D=3, norm="batch", init_type="normal", init_gain=0.02, gpu_ids=[],
             backend=None):
    """discriminators.define_D (:45-88)."""
    from . import get_norm_layer
    norm_layer = get_norm_layer(norm_type=norm)
    if netD == "basic":
        return NLayerDiscriminator(backend, input_nc, ndf, n_layers=3, norm_layer=norm_layer)
    if netD == "n_layers":
        return NLayerDiscriminator(backend, input_nc, ndf, n_layers_D, norm_layer=norm_layer)
    if netD == "pixel":
        return PixelDiscriminator(backend, input_nc, ndf, norm_layer=norm_layer)
    raise NotImplementedError("Discriminator model name [%s] is not recognized" % netD)
