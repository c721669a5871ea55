"""modules/__init__.py of the reference: weight init + norm-layer selection
(/root/reference/modules/__init__.py:7-74), re-targeted at library-owned parameters.

Initialisation stays host-side in torch: tensors are drawn with the
reference's own initialisers in the reference's order and uploaded through the C-ABI."""
import math
from collections import OrderedDict

import torch
from torch.nn import init


def init_tensor(t, init_type="normal", init_gain=0.02):
    """init_func of modules.init_weights applied to one weight tensor (modules/__init__.py:19-34)."""
    if init_type == "normal":
        init.normal_(t, 0.0, init_gain)
    elif init_type == "xavier":
        init.xavier_normal_(t, gain=init_gain)
    elif init_type == "kaiming":
        init.kaiming_normal_(t, a=0, mode="fan_in")
    elif init_type == "orthogonal":
        init.orthogonal_(t, gain=init_gain)
    else:
        raise NotImplementedError("initialization method [%s] is not implemented" % init_type)
    return t


def _construction_order(layers):
    """Order in which the reference's layer constructors ran.  Plain modules are defined top to bottom
    (= state-dict order); the pix2pix U-Net is built recursively from the innermost block outwards, down
    conv before up conv in each block (modules/pix2pix_modules.py:113-177,208-246), while its state dict
    (module tree) lists the outermost block first."""
    # the TextureModule holds the U-Net as `unet`; a bare UnetGenerator (--netG unet_128) has the prefix `model` itself
    lead = "unet." if any(n.startswith("unet.") for n in layers) else ""
    is_unet = lambda n: n.startswith(lead + "model.model.")
    unet = [n for n in layers if is_unet(n)]
    if not unet:
        return list(layers)
    rest = [n for n in layers if not is_unet(n)]                      # `encode` is defined before the U-Net
    depth = lambda n: (len(n[len(lead):].split(".")) - 3) // 2        # [unet.]model.model.K = block 0
    # (a block's BatchNorm layers sit between its convs here; they draw nothing at construction and the caller skips them)
    order = sorted(unet, key=lambda n: (-depth(n), int(n.rsplit(".", 1)[1])))
    return rest + order


def init_weights(net, init_type="normal", init_gain=0.02):
    """modules.init_weights (modules/__init__.py:7-45) for a swapnet_amd network: `init_type` on every
    Conv*/ConvTranspose* weight, bias := 0.  `net` is any module exposing `native_param_shapes()` /
    `load_state_dict()`.

    The global CPU RNG is consumed exactly like the reference does when it builds and initialises the
    same network -- every torch layer constructor draws its default weight (kaiming_uniform) and bias
    (uniform) in construction order, then init_weights re-draws the weights in module-tree order -- so
    `torch.manual_seed(s); create_model(opt)` starts from the reference's weights, bit for bit
    (tests/test_models_api.py::test_seeded_init_equals_the_reference)."""
    print("initialize network with %s" % init_type)
    shapes = net.native_param_shapes()
    layers = OrderedDict()
    for name, shape in shapes.items():
        prefix, kind = name.rsplit(".", 1)
        layers.setdefault(prefix, {})[kind] = shape
    is_bn = lambda prefix: len(layers[prefix]["weight"]) == 1         # BatchNorm2d: a weight vector (convs: 4-D)
    for prefix in _construction_order(layers):                        # nn.Conv2d / nn.ConvTranspose2d.reset_parameters
        if is_bn(prefix):
            continue                                                  # BatchNorm2d.reset_parameters: ones / zeros, no draw
        init.kaiming_uniform_(torch.empty(layers[prefix]["weight"]), a=math.sqrt(5))
        if "bias" in layers[prefix]:
            torch.empty(layers[prefix]["bias"]).uniform_(-1.0, 1.0)
    sd = {}
    for name, shape in shapes.items():                                # module-tree order: conv and BatchNorm draws interleave
        if name.endswith(".bias"):
            sd[name] = torch.zeros(shape)
        elif is_bn(name.rsplit(".", 1)[0]):
            sd[name] = init.normal_(torch.empty(shape), 1.0, init_gain)        # modules/__init__.py:38-42, whatever init_type says
        else:
            sd[name] = init_tensor(torch.empty(shape), init_type, init_gain)
    # (BatchNorm's buffers are no parameters: they keep what the constructor gave them, so their keys are absent here)
    net.load_state_dict(sd, strict=not any(is_bn(prefix) for prefix in layers))


class Identity(torch.nn.Module):
    def forward(self, x):
        return x


def get_norm_layer(norm_type="instance"):
    """modules.get_norm_layer (modules/__init__.py:53-74).  The native networks take the layer by name: instance (the reference's
    default, base_gan.py:72-77), batch (BatchNorm2d, affine, running statistics) or none.  The discriminators and the
    TextureModule's U-Net implement all three (batch / none for the texture stage: device library only).  WarpModule exists
    under instance and the texture stage's plain U-Net (--netG unet_128, modules/pix2pix_modules.UnetGenerator) under batch --
    as the reference hard-codes them."""
    if norm_type in ("instance", "batch", "none"):
        return norm_type
    raise NotImplementedError("normalization layer [%s] is not found" % norm_type)
