"""Every convolution route on channel-slice views, as the networks call it, against float64.

swn_op_conv / swn_op_conv_produced run a conv on alloc_var buffers: cs == C, the view at the start of its allocation, accumulate 0, no
channel map.  swn_op_conv_views (include/swapnet_hip.h) runs the same layer on parent.batch(n_lead, n).slice(lead_c, C) of sentinel-
filled parents (0x7f in every byte of x, x.g, y, y.g), with the accumulate flag set by the planner (dx_old), the discriminators' channel
maps, x_is_input / dgrad_C and a fused activation in the backward calls.  One pytest case per ROWS entry and backend; each case runs
forward, input gradient (overwriting, and accumulating onto a random dx_old of the gradient's own magnitude) and weight gradient on
the dense layout and on two view combinations (lead_c / pad_c in {0, 4}, n_lead / n_pad in {0, 1}, the second the complement of the
first), the rows marked `real` also on the two halves of a concatenation (lead 0, pad C and lead C, pad 0).

On the MI355X every case proves from the route trace of the DENSE call that the launch took the route its row names (ROUTES: per
direction, substrings that must each occur in the trace -- the launch name with its M, N, K; taken from a trace of the dense calls);
the split-K rows also need a plan with more than one K split.  The simulator has no kernel names and asserts only that the call ran
and holds the bars.  Rows with slots=True (ring-128, ring-64, the pair-* rows; wino-f43-reflect-fold so that the simulator runs the
option too) give x and dY the external amax slots of a model's input buffers (operand_slots), which is what puts the launches on the
slot-scaled ring kernels (_as, _sxy) and the Winograd planes into pair form (_ap, _h2pp, _h2p1); every other row lets each launch
take the amax of its operand itself, with a pass over the view.  ring-transposed-72 runs with SWN_WINOGRAD=0: under the marker's
SWN_WINO_MINC=32 a 48 -> 72 transposed conv is a strided-Winograd layer.

Held in every call (Runner.call / _check_buffers / parity / compare_dense):
 1. two runs are bit-equal, outputs and whole buffers;
 2. every lead / pad channel and lead / pad image of the four parents still holds 0x7f7f7f7f; with a narrow gradient (dgrad_C on k4s2
    and k3 zero-pad) the channels of x.g at and above dgrad_C hold what they held before;
 3. the channels inside a view at and above its logical count, and the -1 entries of a channel map, are exactly 0 afterwards in all
    four buffers (ops.h, next to ConvFwdArgs);
 4. the weight gradient's packed rows (dw_rows) of those input channels are exactly 0;
 5. float64: |got - ref| < ELEM_BAR x scale (+ U |dx_old + ref| accumulating), scale = the same convolution of |a| and |b| (+ |dx_old|),
    ELEM_BAR = 1e-4 (derived in tests/test_produced_operands.py: 22-bit operands, Winograd gain <= 225); rel-L2 < 1e-5 for the
    Winograd and ring rows (the bar test_winograd_layers_of_129_to_192_channels and test_produced_operands.py hold those shapes to),
    1e-4 forward / 2e-4 gradients for the rest (test_conv_forward / test_conv_backward, now against float64); accumulating, the
    norm of U |dx_old + ref| is added.  With a fused activation the branch is the device's own forward y > 0;
 6. where the view call's trace equals the dense call's, the overwriting results are bit-equal to the dense ones.  On the MI355X no
    view of any row took another route than its dense call and none rounded differently: no kernel here depends on the pixel stride
    (a view whose trace differs would be printed as "ROUTE DIFFERS FROM DENSE" and held to the float64 bars alone);
 7. direct conv with fused LeakyReLU / ReLU (the first-layer rows): max(amax slot of y's buffer) == max |y| bit for bit.

Worst figures measured on the MI355X per family, over all views: rel-L2 / worst element in units of ELEM_BAR x scale
  family          forward           input gradient    ... accumulating  weight gradient      rel-L2 bar
  generic         2.4e-07 / 0.0021  2.4e-07 / 0.0027  2.4e-07 / 0.0027  2.8e-07 / 0.0016     1e-4, 2e-4
  tail (folded)   1.4e-07 / 0.0008  2.9e-07 / 0.0006  2.9e-07 / 0.0006  9.1e-08 / 0.0007     1e-4, 2e-4
  transposed      2.8e-07 / 0.0028  3.0e-07 / 0.0023  3.1e-07 / 0.0022  2.8e-07 / 0.0017     1e-4, 2e-4
  head (taps-N)   1.3e-07 / 0.0003  6.2e-08 / 0.0014  7.3e-08 / 0.0012  1.1e-07 / 0.0011     1e-4, 2e-4
  first-layer     3.3e-07 / 0.0026  2.8e-07 / 0.0032  2.8e-07 / 0.0026  2.9e-07 / 0.0028     1e-4, 2e-4
  split-k         2.2e-07 / 0.0004  2.3e-07 / 0.0004  2.3e-07 / 0.0003  1.4e-07 / 0.0044     1e-4, 2e-4
  ring            1.9e-07 / 0.0013  2.9e-07 / 0.0022  3.0e-07 / 0.0022  2.9e-07 / 0.0024     1e-5
  winograd        1.8e-06 / 0.030   1.8e-06 / 0.017   1.8e-06 / 0.016   8.9e-07 / 0.039      1e-5
  winograd-s2     1.5e-06 / 0.022   1.5e-06 / 0.013   1.5e-06 / 0.011   5.3e-07 / 0.28       1e-5
  winograd-tail   1.1e-06 / 0.016   2.7e-07 / 0.0008  2.7e-07 / 0.0007  6.7e-07 / 0.0053     1e-5
  winograd-pair   1.7e-06 / 0.013   1.6e-06 / 0.0093  1.6e-06 / 0.0081  1.8e-06 / 0.015      1e-5
(the 0.28: the one-tile weight gradient of wino-s2-transposed-48, a sum over a single 5 x 5 tile per plane).  All 39 device cases
run in 7 s together.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from swapnet_amd import engine
from tests import backends
from tests.test_ops import BACKENDS, K3REFL, K3ZERO, K4S1, K4S2, TAIL, _ctx, ref_conv
from tests.test_produced_operands import ELEM_BAR, FORMS, REL_BAR, tail_schedule

pytestmark = pytest.mark.small_channel_winograd
K1S1 = 5
NONE, LRELU, RELU = 0, 1, 2
U = 2.0 ** -24
SENT = engine.PAD_SENTINEL
DIRECT_BARS = {"fwd": 1e-4, "dgrad": 2e-4, "wgrad": 2e-4}       # test_conv_forward / test_conv_backward
TIGHT_BARS = {"fwd": REL_BAR, "dgrad": REL_BAR, "wgrad": REL_BAR}

# the discriminators' channel maps (nets.cpp / texture.cpp): 24 view channels, 22 logical
WARP_D_MAP = [3 + i for i in range(19)] + [-1] + [0, 1, 2] + [-1]
TEX_D_MAP = [19, 20, 21, -1] + list(range(19)) + [-1]
RGB8_MAP = [0, 1, 2, -1, -1, -1, -1, -1]


def _row(name, kind, tr, n, ci, h, w, co, family, route=None, gpu_only=False, tight=False, real=False, env=None, act=NONE, bias=True, **first):
    return dict(name=name, kind=kind, tr=tr, n=n, ci=ci, h=h, w=w, co=co, family=family, route=route or ROUTES[name], gpu_only=gpu_only, tight=tight,
                real=real, env=env or {}, act=act, bias=bias, first=first)


def _form(name, form, family, **kw):
    kind, tr, n, ci, h, w, co, env = FORMS[form]
    return _row(name, kind, tr, n, ci, h, w, co, family, gpu_only=True, tight=True, env=env, **kw)


# The kernel every direction of a row's DENSE call must show in the route trace (MI355X; from a trace of the dense calls): the launch
# name with its M, N, K (Winograd plane GEMMs: M = tiles, K = input channels, b = planes)
ROUTES = {
    'generic-k4s2': {"fwd": ('conv_fwd_narrow8_generic[M96,N8,K64,',), "dgrad": ('conv_fwd_narrow4_generic[M96,N4,K32,',), "wgrad": ('conv_wgrad_256x8[M96,N8,K64,',)},
    'generic-k4s1': {"fwd": ('conv_fwd_narrow8_generic[M96,N5,K128,',), "dgrad": ('conv_fwd_narrow8_generic[M126,N8,K128,',), "wgrad": ('conv_wgrad_256x8[M96,N5,K128,',)},
    'generic-k3zero': {"fwd": ('conv_fwd_narrow8_generic[M48,N8,K36,',), "dgrad": ('conv_fwd_narrow4_generic[M48,N4,K72,',), "wgrad": ('conv_wgrad_256x8[M48,N8,K36,',)},
    'folded-tail': {"fwd": ('conv_fwd_narrow20_generic[M24,N19,K48,', 'conv_fwd_narrow20_generic[M24,N19,K72,', 'conv_fwd_narrow20_generic[M24,N19,K108,'), "dgrad": ('conv_fwd_narrow16_generic[M24,N12,K500,',), "wgrad": ('conv_wgrad_128x32[M24,N19,K48,', 'conv_wgrad_128x32[M24,N19,K108,')},
    'transposed-8-12': {"fwd": ('conv_fwd_narrow16_generic[M30,N12,K32,',), "dgrad": ('conv_fwd_narrow8_generic[M30,N8,K192,',), "wgrad": ('conv_wgrad_128x32[M30,N12,K32,',)},
    'transposed-4-3': {"fwd": ('conv_fwd_narrow4_generic[M15,N3,K16,',), "dgrad": ('conv_fwd_narrow4_generic[M15,N4,K64,',), "wgrad": ('conv_wgrad_256x4[M15,N3,K16,',)},
    'k1s1': {"fwd": ('conv_fwd_narrow16_generic[M48,N16,K8,',), "dgrad": ('conv_fwd_narrow8_generic[M48,N8,K16,',), "wgrad": ('conv_wgrad_128x32[M48,N16,K8,',)},
    'wino-f23-reflect': {"fwd": ('conv_fwd_narrow32_fast[M30,N32,K32,',), "dgrad": ('conv_fwd_narrow32_fast[M30,N32,K32,',), "wgrad": ('conv_wgrad_128x32[M30,N32,K32,',)},
    'wino-f43-zero': {"fwd": ('conv_fwd_pc_256x64_as[M6,N64,K32,b36,',), "dgrad": ('conv_fwd_narrow32_fast[M6,N32,K64,',), "wgrad": ('conv_wgrad_128x64[M6,N64,K32,',)},
    'wino-f43-reflect-fold': {"fwd": ('conv_fwd_narrow32_fast[M4,N32,K32,',), "dgrad": ('conv_fwd_narrow32_fast[M4,N32,K32,',), "wgrad": ('conv_wgrad_128x32[M4,N32,K32,',)},
    'wino-f34-ragged': {"fwd": ('conv_fwd_narrow32_fast[M6,N32,K32,',), "dgrad": ('conv_fwd_narrow32_fast[M9,N32,K32,',), "wgrad": ('conv_wgrad_128x32[M6,N32,K32,',)},
    'head-tapn': {"fwd": ('conv_fwd_narrow16_fast[M60,N16,K32,',), "dgrad": ('conv_fwd_narrow32_generic[M60,N32,K16,',), "wgrad": ('conv_wgrad_128x32[M60,N16,K32,',)},
    'wino-s2': {"fwd": ('conv_fwd_narrow32_fast[M4,N32,K128,',), "dgrad": ('conv_fwd_pc_128x128_as[M4,N128,K32,b25,',), "wgrad": ('conv_wgrad_128x32[M4,N32,K128,',)},
    'wino-s2-ragged': {"fwd": ('conv_fwd_pc_256x64_as[M4,N64,K128,b25,',), "dgrad": ('conv_fwd_pc_128x128_as[M4,N128,K64,b25,',), "wgrad": ('conv_wgrad_128x64[M4,N64,K128,',)},
    'wino-s2-transposed': {"fwd": ('conv_fwd_pc_128x128_as[M4,N128,K32,b25,',), "dgrad": ('conv_fwd_narrow32_fast[M4,N32,K128,',), "wgrad": ('conv_wgrad_128x32[M4,N32,K128,',)},
    'wino-s2-transposed-48': {"fwd": ('conv_fwd_pc_128x128_as[M1,N128,K48,b25,',), "dgrad": ('conv_fwd_pc_256x64_as[M1,N48,K128,b25,',), "wgrad": ('conv_wgrad_128x64[M1,N48,K128,',)},
    'wino-tail': {"fwd": ('conv_fwd_pc_128x128_as[M12,N80,K32,b36,',), "dgrad": ('conv_fwd_narrow32_generic[M192,N32,K500,',), "wgrad": ('conv_wgrad_128x128[M12,N80,K32,',)},
    'wino-tail-ragged': {"fwd": ('conv_fwd_pc_128x128_as[M4,N80,K64,b36,',), "dgrad": ('conv_fwd_128x64_generic[M36,N64,K500,',), "wgrad": ('conv_wgrad_128x128[M4,N80,K64,',)},
    'warpD-model0-k4s2': {"fwd": ('conv_fwd_128x64_generic[M128,N64,K384,',), "dgrad": ('conv_fwd_phase4_narrow20[M128,N20,K256]',), "wgrad": ('conv_wgrad_128x64[M128,N64,K384,',)},
    'warpD-net0-k1s1': {"fwd": ('conv_fwd_128x64_generic[M512,N64,K24,',), "dgrad": ('conv_fwd_narrow24_fast[M512,N24,K64,',), "wgrad": ('conv_wgrad_128x64[M512,N64,K24,',)},
    'texD-model0-k4s2': {"fwd": ('conv_fwd_128x64_generic[M128,N64,K384,',), "dgrad": ('conv_fwd_phase4_narrow4[M128,N4,K256]',), "wgrad": ('conv_wgrad_128x64[M128,N64,K384,',)},
    'texD-net0-k1s1': {"fwd": ('conv_fwd_128x64_generic[M512,N64,K24,',), "dgrad": ('conv_fwd_narrow24_fast[M512,N24,K64,',), "wgrad": ('conv_wgrad_128x64[M512,N64,K24,',)},
    'texG-model0': {"fwd": ('conv_fwd_128x64_generic[M128,N64,K384,',), "dgrad": ('conv_fwd_phase4_narrow8[M128,N8,K256]',), "wgrad": ('conv_wgrad_128x64[M128,N64,K384,',)},
    'vgg-k3zero-3-64': {"fwd": ('conv_fwd_128x64_generic[M192,N64,K72,',), "dgrad": ('conv_fwd_narrow4_fast[M192,N4,K576,',), "wgrad": ('conv_wgrad_128x64[M192,N64,K72,',)},
    'ring-128': {"fwd": ('conv_fwd_pc_128x128_as[M512,N128,K1024,b1,',), "dgrad": ('conv_fwd_pc_256x64_as[M512,N64,K512,b4,',), "wgrad": ('conv_wgrad_dma_128x128_h2_sxy[M512,N128,K1024,',)},
    'ring-64': {"fwd": ('conv_fwd_pc_128x128_as[M512,N96,K768,b1,',), "dgrad": ('conv_fwd_pc_256x64_as[M512,N48,K384,b4,',), "wgrad": ('conv_wgrad_dma_128x128_h2_sxy[M512,N96,K768,',)},
    'ring-wide-k3zero-80': {"fwd": ('conv_fwd_pc_128x128[M288,N80,K432,',), "dgrad": ('conv_fwd_pc_256x64[M288,N48,K720,',), "wgrad": ('conv_wgrad_128x128[M288,N80,K432,',)},
    'ring-wide-k4s1-40': {"fwd": ('conv_fwd_pc_256x64[M192,N40,K768,',), "dgrad": ('conv_fwd_128x64_generic[M243,N48,K640,',), "wgrad": ('conv_wgrad_dma_256x64_h2[M192,N40,K768,',)},
    'register-staged-k4s2': {"fwd": ('conv_fwd_128x64_generic[M512,N48,K192,',), "dgrad": ('conv_fwd_phase4_narrow16[M512,N12,K192]',), "wgrad": ('conv_wgrad_128x64[M512,N48,K192,',)},
    'phase4-transposed-19': {"fwd": ('conv_fwd_phase4_narrow20[M512,N19,K256]',), "dgrad": ('conv_fwd_128x64_generic[M512,N64,K320,',), "wgrad": ('conv_wgrad_128x32[M512,N19,K256,',)},
    'phase4-transposed-8': {"fwd": ('conv_fwd_phase4_narrow8[M64,N8,K128]',), "dgrad": ('conv_fwd_narrow32_generic[M64,N32,K128,',), "wgrad": ('conv_wgrad_256x8[M64,N8,K128,',)},
    'ring-transposed-72': {"fwd": ('conv_fwd_pc_128x128[M36,N72,K192,b4,',), "dgrad": ('conv_fwd_128x64_generic[M36,N48,K1152,',), "wgrad": ('conv_wgrad_128x128[M36,N72,K192,',)},
    'splitk-k4s2': {"fwd": ('conv_fwd_pc_128x128[M32,N1024,K8192,b1,',), "dgrad": ('conv_fwd_pc_128x128[M32,N512,K4096,b4,',), "wgrad": ('conv_wgrad_dma_128x128_h2[M32,N1024,K8192,b1,',)},
    'splitk-transposed': {"fwd": ('conv_fwd_pc_128x128[M32,N512,K4096,b4,',), "dgrad": ('conv_fwd_pc_128x128[M32,N1024,K8192,b1,',), "wgrad": ('conv_wgrad_dma_128x128_h2[M32,N512,K4096,b4,',)},
    'pair-k3refl': {"fwd": ('conv_fwd_pc_128x128_ap[M128,N128,K128,b36,',), "dgrad": ('conv_fwd_pc_128x128_ap[M128,N128,K128,b36,',), "wgrad": ('conv_wgrad_dma_128x128_h2pp[M128,N128,K128,b36,',)},
    'pair-k4s1': {"fwd": ('conv_fwd_pc_128x128_ap[M160,N128,K128,b36,',), "dgrad": ('conv_fwd_pc_128x128_ap[M176,N128,K128,b36,',), "wgrad": ('conv_wgrad_dma_128x128_h2pp[M160,N128,K128,b36,',)},
    'pair-k4s2': {"fwd": ('conv_fwd_pc_256x64_ap[M32,N64,K256,b25,',), "dgrad": ('conv_fwd_pc_128x128_ap[M32,N256,K64,b25,',), "wgrad": ('conv_wgrad_dma_256x64_h2pp[M32,N64,K256,b25,',)},
    'pair-k4s2-transposed': {"fwd": ('conv_fwd_pc_128x128_ap[M32,N256,K64,b25,',), "dgrad": ('conv_fwd_pc_256x64_ap[M32,N64,K256,b25,',), "wgrad": ('conv_wgrad_dma_256x64_h2pp[M32,N64,K256,b25,',)},
    'pair-tail': {"fwd": ('conv_fwd_pc_128x128_ap[M32,N80,K128,b36,',), "dgrad": ('conv_fwd_128x128_generic[M512,N128,K500,',), "wgrad": ('conv_wgrad_dma_128x128_h2p1_sy[M32,N80,K128,b36,',)},
}

NO_WINO = {"SWN_WINOGRAD": "0"}
# route: {direction: (substrings that must each occur in the dense call's trace)}; device only
ROWS = [
    # ---- both backends
    _row("generic-k4s2", K4S2, 0, 2, 3, 16, 12, 8, "generic", real=True),
    _row("generic-k4s1", K4S1, 0, 2, 8, 9, 7, 5, "generic"),
    _row("generic-k3zero", K3ZERO, 0, 1, 3, 8, 6, 8, "generic"),
    _row("folded-tail", TAIL, 0, 1, 12, 6, 4, 19, "tail", real=True),
    _row("transposed-8-12", K4S2, 1, 2, 8, 5, 3, 12, "transposed", real=True),
    _row("transposed-4-3", K4S2, 1, 1, 4, 3, 5, 3, "transposed"),
    _row("k1s1", K1S1, 0, 2, 8, 6, 4, 16, "generic"),
    _row("wino-f23-reflect", K3REFL, 0, 2, 32, 6, 10, 32, "winograd", tight=True),
    _row("wino-f43-zero", K3ZERO, 0, 1, 32, 8, 12, 64, "winograd", tight=True, real=True),
    _row("wino-f43-reflect-fold", K3REFL, 0, 1, 32, 8, 8, 32, "winograd", tight=True, slots=True),
    _row("wino-f34-ragged", K4S1, 0, 1, 32, 8, 7, 32, "winograd", tight=True),
    _row("head-tapn", K4S1, 0, 2, 32, 6, 5, 1, "head", real=True),
    _row("wino-s2", K4S2, 0, 2, 32, 8, 12, 32, "winograd-s2", tight=True, real=True),
    _row("wino-s2-ragged", K4S2, 0, 1, 32, 12, 12, 64, "winograd-s2", tight=True, bias=False),
    _row("wino-s2-transposed", K4S2, 1, 2, 32, 4, 6, 32, "winograd-s2", tight=True),
    _row("wino-s2-transposed-48", K4S2, 1, 1, 48, 3, 3, 32, "winograd-s2", tight=True, bias=False),
    _row("wino-tail", TAIL, 0, 2, 32, 8, 12, 19, "winograd-tail", tight=True, real=True),
    _row("wino-tail-ragged", TAIL, 0, 1, 64, 6, 6, 19, "winograd-tail", tight=True),
    # ---- first-layer rows, as the models build them
    _row("warpD-model0-k4s2", K4S2, 0, 2, 22, 16, 16, 64, "first-layer", act=LRELU, cimap=WARP_D_MAP, x_is_input=True, dgrad_C=20, real=True),
    _row("warpD-net0-k1s1", K1S1, 0, 2, 22, 16, 16, 64, "first-layer", act=LRELU, cimap=WARP_D_MAP, x_is_input=True, dgrad_C=20),
    _row("texD-model0-k4s2", K4S2, 0, 2, 22, 16, 16, 64, "first-layer", act=LRELU, cimap=TEX_D_MAP, x_is_input=True, dgrad_C=4),
    _row("texD-net0-k1s1", K1S1, 0, 2, 22, 16, 16, 64, "first-layer", act=LRELU, cimap=TEX_D_MAP, x_is_input=True, dgrad_C=4),
    _row("texG-model0", K4S2, 0, 2, 24, 16, 16, 64, "first-layer", act=LRELU, x_is_input=True, dgrad_C=8, y_views=(0, 64)),
    _row("vgg-k3zero-3-64", K3ZERO, 0, 2, 3, 8, 12, 64, "first-layer", act=RELU, cimap=RGB8_MAP, x_is_input=True, dgrad_C=4),
    # ---- device only
    _form("ring-128", "ring-128", "ring", real=True, slots=True),
    _form("ring-64", "ring-64", "ring", slots=True),
    _row("ring-wide-k3zero-80", K3ZERO, 0, 2, 48, 12, 12, 80, "ring", gpu_only=True, tight=True),
    _row("ring-wide-k4s1-40", K4S1, 0, 3, 48, 9, 9, 40, "ring", gpu_only=True, tight=True),
    _row("register-staged-k4s2", K4S2, 0, 2, 12, 32, 32, 48, "generic", gpu_only=True),
    _row("phase4-transposed-19", K4S2, 1, 2, 64, 16, 16, 19, "transposed", gpu_only=True),
    _row("phase4-transposed-8", K4S2, 1, 1, 32, 8, 8, 8, "transposed", gpu_only=True, bias=False),
    _row("ring-transposed-72", K4S2, 1, 1, 48, 6, 6, 72, "ring", gpu_only=True, tight=True, env=NO_WINO),
    _row("splitk-k4s2", K4S2, 0, 2, 512, 8, 8, 1024, "split-k", gpu_only=True, bias=False, real=True),
    _row("splitk-transposed", K4S2, 1, 2, 1024, 4, 4, 512, "split-k", gpu_only=True, bias=False),
    _form("pair-k3refl", "k3refl", "winograd-pair", real=True, slots=True),
    _form("pair-k4s1", "k4s1", "winograd-pair", slots=True),
    _form("pair-k4s2", "k4s2", "winograd-pair", slots=True),
    _form("pair-k4s2-transposed", "k4s2-transposed", "winograd-pair", slots=True),
    _form("pair-tail", "tail", "winograd-pair", slots=True),
]


def _params():
    out = []
    for i, row in enumerate(ROWS):
        for b in BACKENDS:
            if row["gpu_only"] and b.values[0] != "gpu":
                continue
            out.append(pytest.param(i, b.values[0], id="%s-%s" % (row["name"], b.id), marks=b.marks))
    return out


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return (a is None and b is None) or torch.equal(_bits(a), _bits(b))


def _record(row, direction, view, **figs):
    print("CONVVIEWS %-24s %-9s %-12s %s" % (row["name"], direction, view, "  ".join("%s %.3g" % kv for kv in figs.items())))


def _conv64(row, x, w, b):
    if row["kind"] == K1S1:
        return F.conv2d(x, w, b)
    return ref_conv(x, w, b, row["kind"], row["tr"])


def _slope(row, positive):
    """d act / d pre on the branch the device took."""
    if row["act"] == NONE:
        return None
    return torch.where(positive, 1.0, 0.2 if row["act"] == LRELU else 0.0).double()


class Case:
    """The tensors of a row and its float64 references (computed once per branch pattern)."""

    def __init__(self, row, seed):
        self.row = row
        g = torch.Generator().manual_seed(seed)
        n, ci, h, w, co, kind, tr = (row[k] for k in ("n", "ci", "h", "w", "co", "kind", "tr"))
        k = {K3REFL: 3, K3ZERO: 3, K1S1: 1}.get(kind, 4)
        self.x = torch.randn(n, ci, h, w, generator=g)
        self.w = torch.randn((ci, co, k, k) if tr else (co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5
        self.b = torch.randn(co, generator=g) * 0.1 if row["bias"] else None
        ho, wo = engine.conv_out_hw(kind, tr, h, w)
        self.dy = torch.randn(n, co, ho, wo, generator=g)
        self.gen = g
        self._fwd = None
        self._bwd = {}
        self.dx_old = None

    def forward_ref(self, y_dev):
        """(ref, scale): act on the branch of the device's own output."""
        if self._fwd is None:
            b64 = self.b.double() if self.b is not None else None
            self._fwd = (_conv64(self.row, self.x.double(), self.w.double(), b64),
                         _conv64(self.row, self.x.abs().double(), self.w.abs().double(), b64.abs() if b64 is not None else None))
        pre, scale = self._fwd
        s = _slope(self.row, y_dev > 0)
        return (pre, scale) if s is None else (pre * s, scale * s)

    def backward_ref(self, y_fwd):
        """{"dgrad": (ref, scale), "wgrad": (ref, scale)} for the branch pattern of y_fwd (None without an activation)."""
        s = _slope(self.row, y_fwd > 0) if y_fwd is not None else None
        key = None if s is None else hash(s.numpy().tobytes())
        if key not in self._bwd:
            def two(a, b, d):
                a, b = a.double().requires_grad_(True), b.double().requires_grad_(True)
                gx, gw = torch.autograd.grad(_conv64(self.row, a, b, None), (a, b), d)
                return gx, gw
            d = self.dy.double() if s is None else self.dy.double() * s
            gx, gw = two(self.x, self.w, d)
            gxa, gwa = two(self.x.abs(), self.w.abs(), d.abs())
            self._bwd = {key: {"dgrad": (gx, gxa), "wgrad": (gw, gwa)}}
        return self._bwd[key]


def _view_sets(i, row):
    """[(label, {"x": (lead_c, pad_c, n_lead, n_pad), "y": ...})]: dense, a combination that changes with the row index, its complement,
    and for `real` rows the first and the second half of a concatenation."""
    j = (i * 37 + 11) % 256

    def combo(j):
        b = [(j >> k) & 1 for k in range(8)]
        return {"x": (4 * b[0], 4 * b[1], b[4], b[5]), "y": (4 * b[2], 4 * b[3], b[6], b[7])}
    sets = [("dense", {"x": (0, 0, 0, 0), "y": (0, 0, 0, 0)}), ("view-a", combo(j)), ("view-b", combo(255 - j))]
    cx = len(row["first"]["cimap"]) if row["first"].get("cimap") else -(-row["ci"] // 4) * 4
    cy = -(-row["co"] // 4) * 4
    if row["real"]:
        sets += [("first-half", {"x": (0, cx, 0, 0), "y": (0, cy, 0, 0)}), ("second-half", {"x": (cx, 0, 0, 0), "y": (cy, 0, 0, 0)})]
    if row["first"].get("y_views"):          # the layer's own output geometry (texture generator model.0: slice(0, 64) of 128 channels)
        lead, pad = row["first"]["y_views"]
        sets.append(("model", {"x": (0, 0, 0, 0), "y": (lead, pad, 0, 0)}))
    return sets


def _view_box(buf, geo, n, c):
    """The view's part of a whole parent buffer (n_tot, lead + c + pad, H, W) and a mask of everything else."""
    lead, _, n_lead, _ = geo
    outside = torch.ones(buf.shape[:2], dtype=torch.bool)
    outside[n_lead:n_lead + n, lead:lead + c] = False
    return buf[n_lead:n_lead + n, lead:lead + c], outside


class Runner:
    def __init__(self, ctx, backend, i, row, case, naive=False):
        self.ctx, self.backend, self.i, self.row, self.case, self.naive = ctx, backend, i, row, case, naive
        f = row["first"]
        self.cimap = f.get("cimap")
        self.kw = dict(cimap=self.cimap, x_is_input=f.get("x_is_input", False), dgrad_C=f.get("dgrad_C", 0), operand_slots=f.get("slots", False))
        self.cx = len(self.cimap) if self.cimap else -(-row["ci"] // 4) * 4
        self.cy = -(-row["co"] // 4) * 4
        # view channel -> logical channel of x (-1: not logical)
        self.xmap = list(self.cimap) if self.cimap else [c if c < row["ci"] else -1 for c in range(self.cx)]
        self.ymap = [c if c < row["co"] else -1 for c in range(self.cy)]
        narrow = f.get("dgrad_C", 0)
        self.narrow = narrow if (0 < narrow < self.cx and narrow % 4 == 0 and row["kind"] in (K4S2, K3ZERO) and not row["tr"]) else 0
        self.problems = []
        self.worst = {}

    def fail(self, *what):
        self.problems.append(what)

    def call(self, what, views, dx_old=None, want_slot=False):
        """One call, twice, traced; everything that holds in every call is checked here.  Returns (result dict, trace lines)."""
        row, c = self.row, self.case
        x = c.x if (what != 2 or row["act"] != NONE) else torch.zeros_like(c.x)
        args = dict(dy=None if what == 0 else c.dy, bias=c.b, act=row["act"], views=views,
                    dx_old=dx_old, want_slot=want_slot, naive=self.naive, **self.kw)
        wgt = c.w
        with backends.traced_route(self.ctx) as tr:
            r = engine.op_conv_views(self.ctx, row["kind"], row["tr"], what, x, wgt, **args)
        r2 = engine.op_conv_views(self.ctx, row["kind"], row["tr"], what, x, wgt, **args)
        self.ctx.sync()
        for k in r:
            if not _same(r[k], r2[k]):
                self.fail("two runs differ", what, views, k)
        r = {k: (v.cpu() if v is not None else None) for k, v in r.items()}
        self._check_buffers(what, views, r, dx_old)
        return r, tr.lines

    def _check_buffers(self, what, views, r, dx_old):
        row = self.row
        n = row["n"]
        for name, geo, c, cmap in (("x_buf", views["x"], self.cx, self.xmap), ("xg_buf", views["x"], self.cx, self.xmap),
                                   ("y_buf", views["y"], self.cy, self.ymap), ("yg_buf", views["y"], self.cy, self.ymap)):
            box, outside = _view_box(r[name], geo, n, c)
            ob = _bits(r[name])
            bad = (ob != SENT) & outside[:, :, None, None]
            if bool(bad.any()):
                self.fail("written outside the view", what, views, name, int(bad.sum()), "elements")
            pads = [j for j, m in enumerate(cmap) if m < 0]
            if pads and bool((box[:, pads] != 0).any()):
                self.fail("a non-logical channel inside the view is not exactly 0", what, views, name,
                          float(box[:, pads].abs().max()))
        # x.g: the logical channels the call leaves alone hold what they held before (the sentinel, or dx_old)
        box, _ = _view_box(r["xg_buf"], views["x"], n, self.cx)
        written = what == 2 or (what == 1 and not self.kw["x_is_input"])
        for j, m in enumerate(self.xmap):
            if m < 0 or (written and (not self.narrow or j < self.narrow)):
                continue
            if what == 2 and dx_old is not None:
                ok = torch.equal(_bits(box[:, j]), _bits(dx_old[:, m]))
            else:
                ok = bool((_bits(box[:, j]) == SENT).all())
            if not ok:
                self.fail("a channel of x.g the call must leave alone changed", what, views, "view channel", j)
        if what == 2:       # the returned tensor is the view's logical channels
            for j, m in enumerate(self.xmap):
                if m >= 0 and not torch.equal(_bits(box[:, j]), _bits(r["out"][:, m])):
                    self.fail("the returned dX is not the view's channel", what, views, j)
                    break
        if what == 0:
            box, _ = _view_box(r["y_buf"], views["y"], n, self.cy)
            if not torch.equal(_bits(box[:, :row["co"]]), _bits(r["out"])):
                self.fail("the returned y is not the view's logical channels", views)
        if what == 1:
            pads = [j for j, m in enumerate(self.xmap) if m < 0]
            rows_ = r["dw_rows"][pads] if row["tr"] else r["dw_rows"][:, pads]
            if pads and bool((rows_ != 0).any()):
                self.fail("weight-gradient rows of non-logical input channels are not exactly 0", views, float(rows_.abs().max()))
            logical = [(j, m) for j, m in enumerate(self.xmap) if m >= 0]
            jj, mm = [j for j, _ in logical], [m for _, m in logical]
            got = r["dw_rows"][jj] if row["tr"] else r["dw_rows"][:, jj]
            want = r["out"][mm] if row["tr"] else r["out"][:, mm]
            if not torch.equal(_bits(got), _bits(want)):
                self.fail("dw_rows and the unpacked weight gradient disagree", views)

    def parity(self, direction, label, got, ref, scale, old=None):
        """The float64 bars; the figures are printed before anything is asserted."""
        row = self.row
        rel_bar = (TIGHT_BARS if row["tight"] else DIRECT_BARS)[direction]
        got = got.double()
        want = ref if old is None else ref + old.double()
        sc = scale if old is None else scale + old.double().abs()
        extra = 0.0 if old is None else U * want.abs()
        err = (got - want).abs()
        elem = float((err / (ELEM_BAR * sc + extra).clamp_min(1e-300)).max())
        l2 = float(err.norm() / (rel_bar * ref.norm() + (0.0 if old is None else U * float(want.norm())) + 1e-300))
        rel = float(err.norm() / (ref.norm() + 1e-300))
        _record(row, direction + ("+acc" if old is not None else ""), label, rel_l2=rel, rel_over_bar=l2, elem_over_bar=elem)
        key = direction + ("+acc" if old is not None else "")
        w = self.worst.setdefault(key, [0.0, 0.0])
        w[0], w[1] = max(w[0], rel), max(w[1], elem)
        if not np.isfinite(elem) or not np.isfinite(l2):
            self.fail(direction, label, "not finite")
        if l2 >= 1.0:
            self.fail(direction, label, "rel-L2 %.3g over its bar %.1e" % (rel, rel_bar))
        if elem >= 1.0:
            self.fail(direction, label, "worst element %.3g x ELEM_BAR x scale" % elem)

    def route(self, direction, lines):
        if self.backend != "gpu":
            return
        if self.naive:          # (the checkers are not traced: no tiled launch may show)
            if any("conv_fwd_" in l or "conv_wgrad_" in l or "tail_" in l for l in lines):
                self.fail(direction, "a tiled kernel ran under naive = 1", lines)
            return
        want = self.row["route"].get(direction)
        print("CONVVIEWS %-24s %-9s trace %s" % (self.row["name"], direction, " | ".join(lines)))
        if not want:
            self.fail("no route marker in the table for", direction)
            return
        for m in want:
            if not any(m in l for l in lines):
                self.fail(direction, "the dense call did not take the route the row names", m, lines)
        if self.row["family"] == "split-k" and direction != "wgrad":        # the K split and its reduce kernel: a plan with tail_s > 1
            plan = tail_schedule(lines, "conv_fwd_pc")
            if not plan or plan[1] < 2:
                self.fail(direction, "the launch did not split K", plan, lines)

    def run(self):
        row, c = self.row, self.case
        dense = {}
        for label, views in _view_sets(self.i, row):
            is_dense = label == "dense"
            slot = row["act"] != NONE and row["family"] == "first-layer"
            # forward
            r, lines = self.call(0, views, want_slot=slot)
            ref, scale = c.forward_ref(r["out"])
            self.parity("fwd", label, r["out"], ref, scale)
            if slot and not torch.equal(_bits(r["y_slot"].max()), _bits(r["out"].abs().max())):
                self.fail("max(slot) %.9g != max |y| %.9g" % (float(r["y_slot"].max()), float(r["out"].abs().max())), label)
            self.compare_dense("fwd", label, r["out"], lines, dense)
            # input gradient, overwriting
            r, lines = self.call(2, views)
            refs = c.backward_ref(r["y_fwd"])
            if c.dx_old is None:          # a random gradient of the gradient's own magnitude, drawn once per row
                c.dx_old = torch.randn(c.x.shape, generator=c.gen) * float(refs["dgrad"][0].std())
            self.parity_dx("dgrad", label, r["out"], refs["dgrad"], None)
            self.compare_dense("dgrad", label, r["out"], lines, dense)
            # ... and accumulating
            r, lines_acc = self.call(2, views, dx_old=c.dx_old)
            refs = c.backward_ref(r["y_fwd"])
            self.parity_dx("dgrad", label, r["out"], refs["dgrad"], c.dx_old)
            # weight gradient
            r, lines = self.call(1, views)
            refs = c.backward_ref(r["y_fwd"])
            self.parity("wgrad", label, r["out"], *refs["wgrad"])
            self.compare_dense("wgrad", label, r["out"], lines, dense)
        assert not self.problems, self.problems

    def parity_dx(self, direction, label, got, ref_scale, old):
        """The input gradient on the logical channels the launch forms (all of them, or those below a narrow gradient's dgrad_C)."""
        formed = [m for j, m in enumerate(self.xmap) if m >= 0 and (not self.narrow or j < self.narrow)]
        ref, scale = ref_scale
        self.parity(direction, label, got[:, formed], ref[:, formed], scale[:, formed], None if old is None else old[:, formed])

    def compare_dense(self, direction, label, out, lines, dense):
        if label == "dense":
            dense[direction] = (out, lines)
            self.route(direction, lines)
            return
        out0, lines0 = dense[direction]
        if lines != lines0:
            print("CONVVIEWS %-24s %-9s %-12s ROUTE DIFFERS FROM DENSE: %s" % (self.row["name"], direction, label, " | ".join(lines)))
            return
        formed = slice(None)
        if direction == "dgrad":
            formed = [m for j, m in enumerate(self.xmap) if m >= 0 and (not self.narrow or j < self.narrow)]
        a, b = (out[:, formed], out0[:, formed]) if direction == "dgrad" else (out, out0)
        if not torch.equal(_bits(a), _bits(b)):
            self.fail(direction, label, "same route as the dense call, other bits", int((_bits(a) != _bits(b)).sum()), "elements")


@pytest.mark.parametrize("i,backend", _params())
def test_conv_route_on_views(i, backend, monkeypatch):
    row = ROWS[i]
    for k, v in row["env"].items():
        monkeypatch.setenv(k, v)
    ctx = _ctx(backend)
    Runner(ctx, backend, i, row, Case(row, 100 + i)).run()


@pytest.mark.parametrize("backend", BACKENDS)
def test_naive_checkers_on_views(backend):
    """naive = 1 routes every launch to the one-thread-per-output checker kernels (conv_fwd_naive / conv_wgrad_naive), which the
    tiled kernels are cross-checked against elsewhere: the same views and bars for them, on a generic and a first-layer row."""
    ctx = _ctx(backend)
    for name in ("generic-k4s1", "warpD-model0-k4s2"):
        i = [r["name"] for r in ROWS].index(name)
        Runner(ctx, backend, i, ROWS[i], Case(ROWS[i], 200 + i), naive=True).run()


def test_planner_refuses_a_partially_initialised_gradient_range():
    """Net::finalize: the conv writes the gradient range [4, 12) of x's parent buffer; with [0, 8) announced as existing the range is
    partly initialised and planning must fail, reported through swn_last_error.  A disjoint range, [0, 4), plans."""
    ctx = backends.hostsim_ctx()
    x, w = torch.zeros(1, 8, 4, 4), torch.zeros(8, 8, 1, 1)
    dy = torch.zeros(1, 8, 4, 4)
    views = {"x": (4, 0, 0, 0), "y": (0, 0, 0, 0)}
    engine.op_conv_views(ctx, K1S1, 0, 2, x, w, dy=dy, views=views, pre_range=(0, 4))
    with pytest.raises(ValueError, match="partially initialised gradient range"):
        engine.op_conv_views(ctx, K1S1, 0, 2, x, w, dy=dy, views=views, pre_range=(0, 8))
    assert "partially initialised gradient range" in ctx.lib.last_error()
