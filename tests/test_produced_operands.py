"""Producer-scaled convolution operands, held to float64 on the device.

Every GEMM of the step forms fp32 products from two fp16 planes of (operand x 2^k).  Inside a network k almost never comes from a pass
over the operand: it comes from the amax SLOT the operand's producer folded max |v| into, and the Winograd transforms cut their planes
("pair form") with a k derived from such a slot and a gain bound before the plane exists.  swn_op_conv fills its operands from outside
the tape, so no test built on it ever reaches those routes; swn_op_conv_produced (x0 -> pre -> x -> conv -> y -> post -> z) does, and
this file asserts from the route trace that each launch under test really took them.

On the MI355X the slot audit (swn_slot_audit: the simulator's sim_slot_check and pair-plane check applied by the HIP launchers) is on
in the parity, scale and zero tests; on the host simulator, which always checks, the same bodies run with SWN_SIM_PAIR=1.
"""
import re

import pytest
import torch
import torch.nn.functional as F

from swapnet_amd import _C
from tests import backends
from tests.test_ops import BACKENDS, K3REFL, K3ZERO, K4S1, K4S2, TAIL, _ctx, ref_conv, rel, run_conv

pytestmark = pytest.mark.small_channel_winograd
K1S1 = 5


# (kind, transposed, N, Ci, H, W, Co, environment).  Shapes on which the layer stores its Winograd planes in pair form in BOTH directions
# (engine.cpp: tiles % 16 == 0, Npad > 32, and a weight-gradient reduction that fills the ring kernel's k-tile -- 64 -> 64 channels
# does not, 128 -> 128 does), ragged and non-square maps included; and one direct ring shape per tile family.
FORMS = {
    "k3refl": (K3REFL, 0, 2, 128, 32, 32, 128, {}),                  # F(4,3) + reflect fold
    # (F(4,3) needs H % 4 == 0 and W % 4 == 0 -- a 30 x 30 map runs F(2,3), whose planes are fp32 -- so its tiles are never ragged)
    "k3refl-nonsquare": (K3REFL, 0, 2, 128, 16, 32, 128, {}),
    "k3zero": (K3ZERO, 0, 4, 128, 24, 40, 128, {}),                  # non-square
    "k4s1": (K4S1, 0, 2, 128, 31, 23, 128, {}),                      # F(3,4): 30 x 22 outputs, ragged tiles
    "k4s2": (K4S2, 0, 2, 64, 32, 32, 64, {}),                        # strided F(4,2)
    "k4s2-transposed": (K4S2, 1, 2, 64, 16, 16, 64, {}),
    "tail": (TAIL, 0, 2, 128, 16, 16, 19, {}),                       # the folded tail conv as four F(4,3) phases
    "ring-128": (K4S2, 0, 2, 64, 32, 32, 128, {"SWN_WINOGRAD": "0"}),   # direct, 128 x 128 tile
    "ring-64": (K4S2, 0, 2, 48, 32, 32, 96, {"SWN_WINOGRAD": "0"}),     # direct, Cin 48 -> 96
}
WINO = ("k3refl", "k3refl-nonsquare", "k3zero", "k4s1", "k4s2", "k4s2-transposed", "tail")


def form_params():
    return [pytest.param(f, b.values[0], id="%s-%s" % (f, b.id), marks=b.marks) for f in FORMS for b in BACKENDS]


@pytest.fixture
def audited(request, monkeypatch):
    """(ctx, backend) with the slot audit on for the test's duration (a no-op on the simulator, which runs with SWN_SIM_PAIR=1)."""
    backend = request.node.callspec.params["backend"]
    if backend == "sim":
        monkeypatch.setenv("SWN_SIM_PAIR", "1")
    ctx = _ctx(backend)
    ctx.lib.call("swn_slot_audit", 1)
    try:
        yield ctx
    finally:
        ctx.lib.call("swn_slot_audit", 0)


def make_case(form, seed):
    kind, tr, n, ci, h, w, co, env = FORMS[form]
    g = torch.Generator().manual_seed(seed)
    k = 3 if kind in (K3REFL, K3ZERO) else 4
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn((ci, co, k, k) if tr else (co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5
    y_shape = ref_conv(x[:1, :1], torch.zeros((1, 1, k, k)), None, kind, tr).shape[2:]
    dy = torch.randn((n, co) + tuple(y_shape), generator=g)
    return kind, tr, x, wt, dy, env


def refs64(kind, tr, x, wt, dy):
    """float64 forward, input gradient, weight gradient, and conv(|a|, |b|) of each: the scale of one term of every output element."""
    def three(a, b, d):
        a, b = a.double().requires_grad_(True), b.double().requires_grad_(True)
        y = ref_conv(a, b, None, kind, tr)
        gx, gw = torch.autograd.grad(y, (a, b), d.double())
        return y.detach(), gx, gw
    y, gx, gw = three(x, wt, dy)
    ya, gxa, gwa = three(x.abs(), wt.abs(), dy.abs())
    return {"fwd": (y, ya), "dgrad": (gx, gxa), "wgrad": (gw, gwa)}


KSCALE_UNSET = -(2 ** 30)           # run_conv's fill of the kscale output: entries past the layer's count keep it


def run_three(ctx, backend, form, kind, tr, x, wt, dy, which=("fwd", "dgrad", "wgrad"), bias=None, ks=None):
    """The three directions through swn_op_conv_produced with identity stages, each proven from the route trace (device) to have
    taken the producer-scaled form; returns {direction: result}.  ks (a dict) receives the layer's published scale exponents per
    direction."""
    out = {}
    y_shape = dy.shape
    for what, name in ((0, "fwd"), (2, "dgrad"), (1, "wgrad")):
        if name not in which:
            continue
        p = {"want": ("x_slot", "kscale") if what != 2 else ("dy_slot", "kscale")}
        with backends.traced_route(ctx) as r:
            if what == 0:
                out[name] = run_conv(ctx, kind, tr, 0, False, x, wt, bias, 0, y_shape, produced=p)
            elif what == 2:
                out[name] = run_conv(ctx, kind, tr, 2, False, torch.zeros_like(x), wt, None, 0, dy=dy, produced=p)
            else:
                out[name] = run_conv(ctx, kind, tr, 1, False, x, torch.zeros_like(wt), None, 0, dy=dy, produced=p)
        assert_producer_scaled(r.lines, backend, form, name)
        # the engine reserves one kscale entry per pair-form plane tensor of the layer and none for a direct conv: on the simulator,
        # whose trace has no kernel names, this is what shows that the pair form was announced (and its plane check ran)
        reserved = p["kscale"] != KSCALE_UNSET
        assert bool(reserved.any()) == (form in WINO), (form, name, "kscale entries reserved", p["kscale"].tolist())
        assert not reserved[int(reserved.sum()):].any(), (form, name, "reserved entries are not the leading ones", p["kscale"].tolist())
        if ks is not None:
            ks[name] = p["kscale"]
        # the slot the launch scaled by is the one its producer left: max |operand|, to the bit (both backends)
        if what != 2:
            assert float(p["x_slot"].max()) == float(x.abs().max()), (form, name, float(p["x_slot"].max()), float(x.abs().max()))
        else:
            assert float(p["dy_slot"].max()) == float(dy.abs().max()), (form, name)
    return out


def assert_producer_scaled(lines, backend, form, direction):
    """A test that silently fell back to the launch's own amax pass proves nothing: fail unless the route trace shows the
    producer-scaled kernel.  _ap = forward-type ring GEMM on pair-form planes; _h2pp / _h2p1 = weight-gradient ring GEMM with both /
    one operand in pair form; _as / _sx, _sy, _sxy = ring launches whose scale comes from the producers' amax slots (conv_ring.hip)."""
    if backend != "gpu":
        return          # (the simulator has one kernel; its slot use is checked by its own sim_slot_check on every launch)
    gemms = [l for l in lines if ("conv_fwd" in l or "conv_wgrad" in l) and (direction == "fwd" or " b " in l)]
    if form == "tail" and direction == "dgrad":
        # the tail conv's input gradient is a 5 x 5 stride-2 conv over dY with 20 channels: a register-staged kernel on fp32 operands,
        # which has no scale to take from anywhere.  Held to the same bars; what must not happen is a two-plane launch with a pass.
        assert gemms and not any("_pc_" in l or "_dma_" in l for l in gemms), (form, direction, lines)
        return
    if direction == "wgrad":
        gemms = [l for l in gemms if "conv_wgrad" in l]
        want = ("_h2pp", "_h2p1") if form in WINO else ("_sxy",)
    else:
        gemms = [l for l in gemms if "conv_fwd" in l]
        want = ("_ap[",) if form in WINO else ("_as[",)
    assert gemms and all(any(m in l for m in want) for l in gemms), (form, direction, "not the producer-scaled route", want, lines)


# rel-L2 bar: the one the project already holds these forms to against float64 (test_winograd_layers_of_129_to_192_channels).
REL_BAR = 1e-5
# Element-wise bar, in units of conv(|a|, |b|) (the sum of the absolute values of the element's terms): an operand element enters the
# MFMAs with 22 bits (2^-22 relative), and a Winograd transform combines up to gain = 225 (A of F(4,3), the largest) such elements of
# one sign pattern into a plane element, so a correct kernel can be off by 225 x 2^-22 = 5.4e-5 of that sum; the bar is 1.9 x that.
# One dropped or doubled term of AVERAGE size -- the signature of a wrong border, tile edge or tap -- is 1 / (taps x channels) >=
# 1 / 2048 = 4.9e-4 of the sum at these shapes, five times the bar; a term much smaller than average can still sit under it, which is
# why the scale test above compares bit for bit.  Measured against float64 on the MI355X (worst element of fwd / dgrad / wgrad over
# the parity and gain-bound cases): 3.4e-6 for the Winograd forms
# (k3zero input gradient at the gain bound; 2.0e-6 on Gaussian data), a margin of 29; 1.3e-7 for the direct ring forms, a margin of 780.
ELEM_BAR = 1e-4


def check_parity(got, ref, what):
    for name, res in got.items():
        r, ra = ref[name]
        e = rel(res, r)
        worst = float(((res.double() - r).abs() / ra.clamp_min(1e-300)).max())
        print("%s %s: rel-L2 %.2e  worst |err| / conv(|a|,|b|) %.2e" % (what, name, e, worst))
        assert e < REL_BAR, (what, name, "rel-L2", e)
        assert worst < ELEM_BAR, (what, name, "worst element / conv(|a|,|b|)", worst)


@pytest.mark.parametrize("form,backend", form_params())
def test_parity_against_float64(form, backend, audited, monkeypatch):
    """(a) forward, input gradient and weight gradient of every producer-scaled form against float64, identity stages."""
    ctx = audited
    kind, tr, x, wt, dy, env = make_case(form, 5)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = run_three(ctx, backend, form, kind, tr, x, wt, dy)
    check_parity(got, refs64(kind, tr, x, wt, dy), form)


@pytest.mark.parametrize("form,backend", form_params())
def test_scaling_the_input_by_a_power_of_two_scales_the_result_exactly(form, backend, audited, monkeypatch):
    """(c) x0 (forward, weight gradient) or z.g (input gradient, weight gradient) times 2^s: every slot shifts by exactly 2^s, every
    scale exponent by -s, and nothing else in the arithmetic sees the factor -- the result is 2^s times the unscaled one to the bit.
    No tolerance: a scale taken from the wrong slot, a stale slot, or a k published to the wrong launch all show here."""
    ctx = audited
    kind, tr, x, wt, dy, env = make_case(form, 6)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    k0 = {}
    base = run_three(ctx, backend, form, kind, tr, x, wt, dy, ks=k0)
    for s in (-40, 20):
        f = 2.0 ** s
        kx, kd = {}, {}
        fw = run_three(ctx, backend, form, kind, tr, x * f, wt, dy, which=("fwd", "wgrad"), ks=kx)
        bw = run_three(ctx, backend, form, kind, tr, x, wt, dy * f, which=("dgrad", "wgrad"), ks=kd)
        # the published exponents: the same entries reserved, the rest untouched, and the planes of the scaled operand cut with
        # k - s (the tail conv's dY is never a pair-form operand: its input gradient is an fp32 launch and its weight gradient takes
        # only V in pair form, _h2p1, so scaling dY moves no k there)
        for label, kn, name in (("x", kx, "fwd"), ("x", kx, "wgrad"), ("dY", kd, "dgrad"), ("dY", kd, "wgrad")):
            assert torch.equal(kn[name] == KSCALE_UNSET, k0[name] == KSCALE_UNSET), (form, name, kn[name].tolist(), k0[name].tolist())
            if form in WINO and not (form == "tail" and label == "dY"):
                shifted = (kn[name] - k0[name])[k0[name] != KSCALE_UNSET]
                assert (shifted == -s).any(), (form, name, label + " x 2^%d" % s, "no published k moved by -s", k0[name].tolist(), kn[name].tolist())
        for name, res in (("fwd", fw["fwd"]), ("wgrad (x scaled)", fw["wgrad"]), ("dgrad", bw["dgrad"]), ("wgrad (dY scaled)", bw["wgrad"])):
            ref = base[name.split()[0]] * f
            assert torch.isfinite(res).all(), (form, name, s)
            assert torch.equal(res, ref), (form, name, "2^%d" % s, "elements that differ", int((res != ref).sum()), "rel-L2", rel(res, ref))


@pytest.mark.parametrize("form,backend", form_params())
def test_an_all_zero_operand_gives_exact_zeros(form, backend, audited, monkeypatch):
    """(c) slot 0, k 0: the forward result is exactly the bias, both gradients exactly zero, everything finite."""
    ctx = audited
    kind, tr, x, wt, dy, env = make_case(form, 7)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    co = dy.shape[1]
    bias = torch.randn(co, generator=torch.Generator().manual_seed(8))
    kz = {}
    fw = run_three(ctx, backend, form, kind, tr, torch.zeros_like(x), wt, dy, which=("fwd",), bias=bias, ks=kz)
    if form in WINO:
        assert (kz["fwd"] == 0).any(), (form, "a zero operand publishes k = 0", kz["fwd"].tolist())
    assert torch.equal(fw["fwd"], bias.view(1, co, 1, 1).expand_as(fw["fwd"])), (form, "forward of a zero input is not the bias")
    bw = run_three(ctx, backend, form, kind, tr, x, wt, torch.zeros_like(dy), which=("dgrad", "wgrad"))
    for name, res in bw.items():
        assert torch.isfinite(res).all() and not res.any(), (form, name, "gradient of a zero dY is not zero")
    zw = run_three(ctx, backend, form, kind, tr, torch.zeros_like(x), wt, dy, which=("wgrad",))
    assert torch.isfinite(zw["wgrad"]).all() and not zw["wgrad"].any(), (form, "weight gradient of a zero input is not zero")


# ---- (b) fold exactness: max(slot) == max |tensor the kernel wrote|, per producer kernel --------------------------------------------
PRE = {"identity": 0, "instnorm-lrelu": 1, "relu": 2, "upsample": 3, "maxpool": 4}
POST = {"identity": 0, "instnorm-lrelu": 1}
# x0 shapes (N, C, H, W): 33 x 32 (> 1024 pixels: the chunked InstanceNorm path) and 20 x 20 (the register-resident kernels, C % 32 == 0),
# ragged for every block size; 256 channels for the paired-workgroup InstanceNorm; 62 logical channels in a 64-channel buffer
FOLD_SHAPES = ((2, 64, 33, 32), (2, 64, 20, 20), (2, 256, 20, 20), (3, 62, 20, 20))
# the resampling stages, sized so that the larger of x0 and x stays within 4 x 64 x 32 x 32 elements
UPSAMPLE_SHAPES = ((2, 64, 17, 15), (2, 64, 10, 10), (1, 256, 10, 10), (3, 62, 10, 10))        # x = 2 H x 2 W
MAXPOOL_SHAPES = ((2, 64, 34, 30), (2, 64, 20, 20), (1, 256, 20, 20), (3, 62, 20, 20))         # x = H / 2 x W / 2


def plant_positions(shape):
    n, c, h, w = shape
    return {"first element": (0, 0, 0, 0), "last pixel of the last image": (n - 1, 0, h - 1, w - 1),
            "last logical channel": (n // 2, c - 1, h // 2, w // 2), "ragged last block": (n - 1, c - 2, h - 1, w - 3)}


def identity_1x1(c):
    return torch.eye(c).view(c, c, 1, 1).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("pre", list(PRE))
def test_every_producer_of_x_folds_all_it_writes(pre):
    """(b) The slot a producer leaves must equal the maximum of the tensor it wrote, exactly (floats compare exactly; an atomic max on
    the bit pattern is order-independent).  The maximum is planted where a fold loses it: the first element, the last pixel of the
    last image, the last logical channel, a pixel of the ragged last block -- a fold that skips its last wave, its tail rows or one
    template variant reports a smaller slot.  Two outputs of one kernel are compared: no reference run is needed."""
    ctx = _ctx("gpu")
    g = torch.Generator().manual_seed(31)
    for shape in {"upsample": UPSAMPLE_SHAPES, "maxpool": MAXPOOL_SHAPES}.get(pre, FOLD_SHAPES):
        n, c, h, w = shape
        for where, pos in plant_positions(shape).items():
            x0 = torch.randn(shape, generator=g)
            x0[pos] = 1000.0            # (survives InstanceNorm as its plane's -- and the tensor's -- maximum: sqrt(H W - 1) >> 4 sigma)
            p = {"pre": PRE[pre], "want": ("x", "x_slot")}
            co = 64
            wt = torch.zeros(co, c, 1, 1)
            hx, wx = (2 * h, 2 * w) if pre == "upsample" else ((h // 2, w // 2) if pre == "maxpool" else (h, w))
            run_conv(ctx, K1S1, 0, 0, False, x0, wt, None, 0, (n, co, hx, wx), produced=p)
            assert torch.isfinite(p["x"]).all() and torch.isfinite(p["x_slot"]).all()
            top = float(p["x"].abs().max())
            assert top > 5.0, (pre, shape, where, top)
            assert float(p["x_slot"].max()) == top, (pre, shape, where, "slot", float(p["x_slot"].max()), "max |x|", top)


@pytest.mark.gpu
@pytest.mark.parametrize("post", list(POST))
def test_every_producer_of_dy_and_z_folds_all_it_writes(post):
    """(b) the post stage: its forward folds max |z| and its backward max |y.g| -- the conv's dY operand.  A 1 x 1 identity conv carries
    the planted maximum from x0 to the stage's input."""
    ctx = _ctx("gpu")
    g = torch.Generator().manual_seed(32)
    for shape in FOLD_SHAPES[:3]:
        n, c, h, w = shape
        wt = identity_1x1(c)
        for where, pos in plant_positions(shape).items():
            x0 = torch.randn(shape, generator=g)
            x0[pos] = 1000.0
            p = {"post": POST[post], "want": ("z_slot",)}
            z = run_conv(ctx, K1S1, 0, 0, False, x0, wt, None, 0, shape, produced=p)
            top = float(z.abs().max())
            assert top > 5.0 and torch.isfinite(z).all()
            assert float(p["z_slot"].max()) == top, (post, shape, where, "forward", float(p["z_slot"].max()), top)
            # (an unplanted x0: the InstanceNorm's backward projects a gradient spike out where the activation has one too)
            x0 = torch.randn(shape, generator=g)
            dz = torch.randn(shape, generator=g)
            dz[pos] = -1000.0
            p = {"post": POST[post], "want": ("dy", "dy_slot")}
            # (the weight-gradient call: its forward runs on x0 and the weights it is given, so the InstanceNorm's backward works
            # with the statistics of a real plane)
            run_conv(ctx, K1S1, 0, 1, False, x0, wt, None, 0, dy=dz, produced=p)
            assert torch.isfinite(p["dy"]).all()
            top = float(p["dy"].abs().max())
            assert top > 5.0, (post, shape, where, top)
            assert float(p["dy_slot"].max()) == top, (post, shape, where, "backward", float(p["dy_slot"].max()), top)


def tail_schedule(lines, kernel):
    """(tail tiles, splits) of the first launch of `kernel` in a route trace (the [.., tail<tiles>x<splits>] detail)."""
    for l in lines:
        m = re.search(kernel + r"\S*tail(\d+)x(\d+)\]", l)
        if m:
            return int(m.group(1)), int(m.group(2))
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ring-epilogue", "split-tile-reduce", "pass-behind-a-register-staged-kernel", "winograd-output-transform"])
def test_the_conv_folds_the_amax_of_its_own_output(case, monkeypatch):
    """(b) a conv with a fused activation feeds the next GEMM directly and folds max |y| itself: in the ring kernel's epilogue, in the
    reduce kernel of its split tiles (a plan with tail_s > 1, asserted from the route detail), by a pass behind every other kernel
    family, and in the 6-point Winograd output transform (K3ZERO + ReLU: VGG16).  z = y through the identity post stage."""
    ctx = _ctx("gpu")
    # (ring epilogue: K = 128 is 8 stages, too few for the planner to split, so every tile runs whole)
    kind, n, ci, h, co, act, direct = {"ring-epilogue": (K1S1, 2, 128, 32, 128, 1, True), "split-tile-reduce": (K4S2, 2, 256, 8, 128, 1, True),
                                       "pass-behind-a-register-staged-kernel": (K4S2, 2, 20, 16, 64, 1, True),
                                       "winograd-output-transform": (K3ZERO, 2, 128, 32, 128, 2, False)}[case]
    if direct:
        monkeypatch.setenv("SWN_WINOGRAD", "0")
    g = torch.Generator().manual_seed(33)
    k = {K3ZERO: 3, K1S1: 1}.get(kind, 4)
    x = torch.randn(n, ci, h, h, generator=g)
    wt = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    ref = F.conv2d(x.double(), wt.double(), b.double()) if kind == K1S1 else ref_conv(x.double(), wt.double(), b.double(), kind, 0)
    ref = F.leaky_relu(ref, 0.2) if act == 1 else F.relu(ref)
    p = {"want": ("y_slot", "z_slot")}
    with backends.traced_route(ctx) as r:
        z = run_conv(ctx, kind, 0, 0, False, x, wt, b, act, ref.shape, produced=p)
    if case == "ring-epilogue":
        sched = tail_schedule(r.lines, "conv_fwd_pc")
        assert sched is not None and (sched[0] == 0 or sched[1] == 1), ("tiles of the launch are split: the reduce kernel folds, not the epilogue", r.lines)
    elif case == "split-tile-reduce":
        sched = tail_schedule(r.lines, "conv_fwd_pc")
        assert sched is not None and sched[0] > 0 and sched[1] > 1, ("the plan does not split its tail tiles", r.lines)
    elif case == "pass-behind-a-register-staged-kernel":
        assert not any("conv_fwd_pc" in l or "conv_fwd_dma" in l for l in r.lines) and any("conv_fwd_" in l for l in r.lines), r.lines
    else:
        assert any("_ap[" in l for l in r.lines), r.lines
    assert rel(z, ref) < REL_BAR, (case, rel(z, ref))
    top = float(z.abs().max())
    assert float(p["y_slot"].max()) == top, (case, "conv's fold", float(p["y_slot"].max()), top)
    assert float(p["z_slot"].max()) == top, (case, "post stage's fold", float(p["z_slot"].max()), top)


# ---- (d) the gain bound of the pair form, attained ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["input", "dy"])
@pytest.mark.parametrize("wform", ["F43", "F34", "F42"])
def test_gain_constants_bound_the_planes_and_are_attained(wform, which):
    """The constants 100 / 9 (input transforms) and 225 / 49 / 16 (output-gradient transforms) that wino.hip hands its kernels, checked
    in numpy against the transform matrices restated in oracle/split_model.py: no tile of magnitude amax can exceed gain x amax (the
    bound is the squared largest absolute row sum, and 2000 random sign tiles stay inside it), and the tile-periodic sign pattern the
    device test below feeds attains at least 0.9 of it -- a gain that were too large by a binade would fail the second, one that
    were too small the first."""
    import numpy as np
    from oracle import split_model as S
    gain = (S.WINO_INPUT_GAIN if which == "input" else S.WINO_DY_GAIN)[wform]
    M, amax = S.wino_matrix(wform, which), 3.0
    assert S.wino_true_gain(wform, which) <= gain
    rng = np.random.default_rng(0)
    for _ in range(2000):
        tile = amax * rng.choice([-1.0, 1.0], size=(M.shape[1], M.shape[1]))
        assert np.abs(S.wino_plane(wform, which, tile)).max() <= gain * amax
    p, _ = S.wino_periodic_signs(wform, which)
    full = p[np.arange(M.shape[1]) % S.WINO_M[wform]]
    top = np.abs(S.wino_plane(wform, which, amax * np.outer(full, full))).max()
    assert 0.9 * gain * amax <= top <= gain * amax, (wform, which, top, gain * amax)


# per conv form: (transform, matrix, image row -> tile index) of its x operand and of its dY operand.  Input tiles start `pad` = 1 rows
# above the image; the strided form transforms the polyphase components (row 2 i - 1 + s is index i of phase s); the tail conv's dY is
# transformed per sub-pixel phase (row 2 i + a is index i of phase a).
GAIN_PATTERNS = {
    "k3refl": (("F43", "input", lambda r: r + 1), ("F43", "dy", lambda r: r)),
    "k3zero": (("F43", "input", lambda r: r + 1), ("F43", "dy", lambda r: r)),
    "k4s1": (("F34", "input", lambda r: r + 1), ("F34", "dy", lambda r: r)),
    "k4s2": (("F42", "input", lambda r: (r + 1) // 2), ("F42", "dy", lambda r: r)),
    "k4s2-transposed": (("F42", "dy", lambda r: r), ("F42", "input", lambda r: (r + 1) // 2)),
    "tail": (("F43", "input", lambda r: r + 1), ("F43", "dy", lambda r: r // 2)),
}


def tile_rows(form, role, t):
    """Image rows (or columns) that tile t of the operand's Winograd transform gathers, per polyphase component -- written from the
    geometry of each convolution, independently of the index maps above: a stride-1 conv with padding 1 reads input rows
    m t - 1 .. m t + A - 2 for output tile t; the 4 x 4 stride-2 conv y[i] = sum_k w[k] x[2 i - 1 + k] is two 2-tap stride-1 convs
    over the components x_s[j] = x[2 j - 1 + s]; the tail conv's output phase a holds rows 2 i + a.  Rows outside the image are zero
    (or, for the reflecting conv, their mirror images)."""
    strided = lambda: [[2 * (4 * t + j) - 1 + s for j in range(5)] for s in (0, 1)]
    plain = lambda m: [[m * t + j for j in range(m)]]
    if role == "x":
        return {"k3refl": lambda: [[4 * t - 1 + j for j in range(6)]], "k3zero": lambda: [[4 * t - 1 + j for j in range(6)]],
                "tail": lambda: [[4 * t - 1 + j for j in range(6)]], "k4s1": lambda: [[3 * t - 1 + j for j in range(6)]],
                "k4s2": strided, "k4s2-transposed": lambda: plain(4)}[form]()
    return {"k3refl": lambda: plain(4), "k3zero": lambda: plain(4), "k4s1": lambda: plain(3), "k4s2": lambda: plain(4),
            "k4s2-transposed": strided, "tail": lambda: [[2 * (4 * t + j) + a for j in range(4)] for a in (0, 1)]}[form]()


def plane_top(form, role, spec, img):
    """max |plane element| of the transform of channel 0 of image 0, the tiles gathered as tile_rows says."""
    import numpy as np
    from oracle import split_model as S
    a = img[0, 0].double().numpy()
    h, w = a.shape
    if form == "k3refl" and role == "x":
        fix = lambda r, n: -r if r < 0 else (2 * n - 2 - r if r >= n else r)
    else:
        fix = lambda r, n: r
    ext = np.zeros((h + 1, w + 1))
    ext[:h, :w] = a                                   # (row h / column w: the zero that out-of-range indices read)
    pick = lambda rows, n: [r if 0 <= r < n else n for r in (fix(r, n) for r in rows)]
    top = 0.0
    for ty in range(h):
        for rows in tile_rows(form, role, ty):
            if not any(0 <= r < h for r in rows):
                continue
            for tx in range(w):
                for cols in tile_rows(form, role, tx):
                    if not any(0 <= c < w for c in cols):
                        continue
                    tile = ext[np.ix_(pick(rows, h), pick(cols, w))]
                    top = max(top, float(np.abs(S.wino_plane(spec[0], spec[1], tile)).max()))
    return top


def sign_image(spec, shape, amax, seed):
    """The top-left quarter of every channel holds +-amax, the sign of pixel (r, c) = s(r) s(c) with the tile-periodic signs of
    wino_periodic_signs: every tile inside it reaches the plane maximum.  The rest is Gaussian at amax / 4, clamped to amax -- a
    pattern over the whole map sums to (nearly) zero in the weight gradient, and rel-L2 against a cancelled reference says nothing."""
    from oracle import split_model as S
    wform, which, index = spec
    p, _ = S.wino_periodic_signs(wform, which)
    n, c, h, w = shape
    sh = torch.tensor([p[index(r) % len(p)] for r in range(h)], dtype=torch.float32)
    sw = torch.tensor([p[index(r) % len(p)] for r in range(w)], dtype=torch.float32)
    img = (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * (amax / 4)).clamp(-amax, amax)
    img[:, :, :h // 2, :w // 2] = (amax * sh.view(h, 1) * sw.view(1, w))[:h // 2, :w // 2]
    return img


@pytest.mark.parametrize("form,backend", [p for p in form_params() if p.values[0] in GAIN_PATTERNS])
def test_planes_at_the_gain_bound_stay_finite_and_accurate(form, backend, audited):
    """(d) on the device: operands whose Winograd planes reach gain x amax -- where Gaussian data sits 2-3 binades lower and an
    understated gain is invisible.  The audit (pair planes below 65504 at the published scale) stays silent and the results meet
    the float64 bars of the parity test."""
    ctx = audited
    kind, tr, x, wt, dy, env = make_case(form, 9)
    xs, ds = GAIN_PATTERNS[form]
    x, dy = sign_image(xs, x.shape, 3.0, 10), sign_image(ds, dy.shape, 0.37, 11)
    # the planes of THESE images reach the bound, and do not pass it: without this a wrong row -> tile-index map in GAIN_PATTERNS
    # would turn the test into one more parity test
    from oracle import split_model as S
    for role, spec, img, amax in (("x", xs, x, 3.0), ("dy", ds, dy, 0.37)):
        gain = (S.WINO_INPUT_GAIN if spec[1] == "input" else S.WINO_DY_GAIN)[spec[0]]
        top = plane_top(form, role, spec, img)
        assert 0.9 * gain * amax <= top <= gain * amax * (1 + 1e-6), (form, role, "plane maximum", top, "bound", gain * amax)
    got = run_three(ctx, backend, form, kind, tr, x, wt, dy)
    for name, res in got.items():
        assert torch.isfinite(res).all(), (form, name)
    check_parity(got, refs64(kind, tr, x, wt, dy), form + " at the gain bound")


# ---- (e) heavy tails through the pair form ----------------------------------------------------------------------------------------------
HEAVY_SHAPE = (2, 128, 32, 32, 128)               # N, Ci, H, W, Co of a K3ZERO layer: F(4,3), pair form in both directions
HEAVY_X_AT, HEAVY_DY_AT = (1, 7, 12, 21), (0, 100, 5, 9)      # (row 12: the pixel lies in the input patches of two tile rows)


@pytest.fixture(scope="module")
def heavy():
    """Operands with one element at 2^18 x the bulk, their float64 results, and the numpy model of the pair-form route
    (oracle/split_model.py wino_pair_conv_*) with its bound -- computed once, shared by the CPU and the device test, never changed."""
    from oracle import split_model as S
    n, ci, h, w, co = HEAVY_SHAPE
    g = torch.Generator().manual_seed(41)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (ci * 9)) ** 0.5
    dy = torch.randn(n, co, h, w, generator=g)
    x[HEAVY_X_AT], dy[HEAVY_DY_AT] = 2.0 ** 18, -2.0 ** 18
    ref = {k: v[0].numpy() for k, v in refs64(K3ZERO, 0, x, wt, dy).items()}
    wr = wt.transpose(0, 1).flip(2, 3).contiguous()              # the input gradient is the same conv of dY with these weights
    xn, wn, dn, wrn = x.numpy(), wt.numpy(), dy.numpy(), wr.numpy()
    model = {"fwd": S.wino_pair_conv_fwd(xn, wn), "dgrad": S.wino_pair_conv_fwd(dn, wrn), "wgrad": S.wino_pair_conv_wgrad(xn, dn)}
    exact = {"fwd": S.wino_pair_conv_fwd(xn, wn, cut=False), "dgrad": S.wino_pair_conv_fwd(dn, wrn, cut=False),
             "wgrad": S.wino_pair_conv_wgrad(xn, dn, cut=False)}
    bound = {"fwd": S.wino_pair_conv_fwd_bound(xn, wn), "dgrad": S.wino_pair_conv_fwd_bound(dn, wrn), "wgrad": S.wino_pair_conv_wgrad_bound(xn, dn)}
    # the outputs no outlier reaches: in the transform domain an element reaches every output of the tiles whose input patch holds it;
    # the weight gradient sums over all tiles, and an outlier reaches the whole input (output) channel it sits in
    import numpy as np
    far = {k: np.ones(v.shape, bool) for k, v in ref.items()}
    far["fwd"][HEAVY_X_AT[0]] &= ~S.wino_tiles_reached((h, w), HEAVY_X_AT[2:])
    far["dgrad"][HEAVY_DY_AT[0]] &= ~S.wino_tiles_reached((h, w), HEAVY_DY_AT[2:])
    far["wgrad"][:, HEAVY_X_AT[1]] = False
    far["wgrad"][HEAVY_DY_AT[1]] = False
    return dict(x=x, wt=wt, dy=dy, ref=ref, model=model, exact=exact, bound=bound, far=far)


def far_errors(res, ref, bound, far):
    """(worst |err| / bound, rel-L2) over the outputs no outlier reaches."""
    import numpy as np
    d = (np.asarray(res, np.float64) - ref)[far]
    return float((np.abs(d) / bound[far]).max()), float(np.linalg.norm(d) / np.linalg.norm(ref[far]))


def test_the_pair_form_model_is_winograd_and_stays_inside_its_bound(heavy):
    """(e) on the CPU: with the cuts off the model IS the convolution (so its matrices and tiling are right); with them on, its error
    on the outputs no outlier reaches stays inside the element-wise bar (twice the analytic bound of the format's error) for the
    chosen seed, and the price of the shared scale is there to be seen: rel-L2 above 2e-6, eight times the 2^-22 = 2.4e-7 that the
    format gives every element of a tensor without an outlier."""
    import numpy as np
    for name in ("fwd", "dgrad", "wgrad"):
        ref, far = heavy["ref"][name], heavy["far"][name]
        assert np.abs(heavy["exact"][name] - ref).max() <= 1e-9 * np.abs(ref).max(), name
        assert 0.9 < far.mean() < 1.0, (name, far.mean())
        worst, l2 = far_errors(heavy["model"][name], ref, heavy["bound"][name], far)
        print("model %s: worst |err| / bar %.3f  rel-L2 %.2e" % (name, worst, l2))
        assert worst < 1.0, (name, worst)
        assert l2 > 2e-6, (name, l2)


@pytest.mark.parametrize("backend", BACKENDS)
def test_pair_form_on_heavy_tailed_operands(backend, audited, heavy):
    """(e) The Winograd twin of test_two_plane_form_on_heavy_tailed_operands: one activation and one dY element at 2^18 x the bulk,
    through the pair-form F(4,3) route with the audit on.  A pair-form plane has ONE scale, fixed from gain x amax before the plane
    exists, so an outlier pushes every other element's low half into fp16's subnormals: the element keeps an ABSOLUTE error of
    gain x amax x 2^-39 (oracle/split_model.py pair_abs_err), and a transform that lost more than that -- a cut before the last
    butterfly, a truncating conversion, an l half dropped -- shows on the outputs no outlier reaches, where rel-L2 1e-5 on Gaussian
    data cannot see it.  Two bars, both from the numpy model of the route and neither from the kernel:
      * element-wise, twice the analytic bound of the model's error (wino_pair_conv_*_bound);
      * rel-L2 over those outputs, twice the model's own (1.2e-5 forward, so 2.4e-5): a sum of 36 x 128 independent cut errors is
        far inside its worst case, and only the norm notices a loss of a few bits.
    Measured on the MI355X, as a fraction of each bar (profiles/produced_operands.txt): element-wise 0.021 (forward), 0.021 (input
    gradient), 0.031 (weight gradient); rel-L2 0.505, 0.502, 0.500 -- the kernels lose what the format loses and nothing more (the
    simulator's rounding model: 0.501, 0.499, 0.500)."""
    ctx = audited
    x, wt, dy = heavy["x"], heavy["wt"], heavy["dy"]
    got = run_three(ctx, backend, "k3zero", K3ZERO, 0, x, wt, dy)
    for name, res in got.items():
        assert torch.isfinite(res).all(), name
        ref, far = heavy["ref"][name], heavy["far"][name]
        worst, l2 = far_errors(res.numpy(), ref, heavy["bound"][name], far)
        _, model_l2 = far_errors(heavy["model"][name], ref, heavy["bound"][name], far)
        print("heavy tail %s %s: worst |err| / bar %.3f  rel-L2 %.3e = %.3f of its bar (2 x model %.3e)" % (backend, name, worst, l2, l2 / (2 * model_l2), model_l2))
        assert worst < 1.0, (name, "element-wise", worst)
        assert l2 < 2 * model_l2, (name, "rel-L2", l2, "bar", 2 * model_l2)


# ---- (f) the audit on whole training steps ----------------------------------------------------------------------------------------------
STEP_CASES = ["warp-64", "texture-64", "warp-64-wgan-gp", "warp-128x64"]
STEP_PARAMS = [pytest.param(c, b.values[0], id="%s-%s" % (c, b.id), marks=b.marks) for c in STEP_CASES for b in BACKENDS]


@pytest.mark.parametrize("case,backend", STEP_PARAMS)
def test_training_steps_pass_the_slot_audit(case, backend, audited):
    """(f) one eager training step at batch size 2 with the audit on -- every slot a launch of the step trusts is at least the amax of
    what the launch gathers and at most 4096 x it, every pair-form plane fits fp16 -- and a second step whose loss gradients are
    2^-12 of the first one's (grad_scale), which a slot left standing from the step before would fail from above."""
    from oracle import swapnet_oracle as O
    from swapnet_amd import engine
    ctx = audited
    torch.manual_seed(0)
    B, H, W = 2, (128 if case == "warp-128x64" else 64), 64
    if case.startswith("warp"):
        G, D = O.warp_module_params(), O.patchgan_params(22)
        batch = O.synth_warp_batch(B, H, W, seed=1234)
        m = backends.get_model(ctx, "warp", B, H) if H == W else engine.NativeModel(ctx, "warp", B, H, W, is_train=True)
        backends.reset_state(m, {engine.NET_G: G, engine.NET_D: D})
    else:
        from tests.test_texture_step import vgg_state_dict
        G, D, vgg = O.texture_module_params(img_size=H), O.patchgan_params(22), O.vgg16_feature_params()
        batch = O.synth_texture_batch(B, H, W, seed=4321)
        m = backends.get_model(ctx, "texture", B, H)
        backends.reset_state(m, {engine.NET_G: G, engine.NET_D: D})
        m.load_state_dict(engine.NET_VGG, vgg_state_dict(m, vgg))
    hyper = dict(gan_mode=2, gp_mode=1) if case.endswith("wgan-gp") else {}
    try:
        for i, t in enumerate(batch):
            m.set_input(i, t)
        for grad_scale in (1.0, 2.0 ** -12):
            m.set_hyper(grad_scale=grad_scale, **hyper)
            m.step((0.9, 0.8, 1.0), training=False, seed=3)          # (an audit failure raises here, naming the launch)
            ctx.sync()
            L = m.losses()
            assert all(v == v and abs(v) < float("inf") for v in L.values()), (case, grad_scale, L)
    finally:
        if H != W:
            m.close()
