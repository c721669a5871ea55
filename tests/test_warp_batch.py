"""SURVEY.md 8(f) rank 3, the warp half: a warp batch handed over in compact form -- the decoded uint8 HWC body image, the uint8 input
and target label maps, the per-channel map table of gpu_augment -- and expanded into every buffer the step reads by ONE device launch
(csrc/warp_batch.hip; the host loop of engine.cpp on the simulator).  The oracle is the host chain of the reference's
WarpDataset.__getitem__ (datasets/warp_dataset.py:139-183), written out below with numpy and torch: one-hot, gpu_augment.apply_maps
(pinned to Pillow by tests/test_augment.py), F.interpolate nearest, crop; for the body a numpy float32 restatement of torch's published
bilinear formula.  Every comparison with that chain is an equality: each step is an integer gather or one correctly rounded fp32
operation.  The body is additionally held against torch's float64 bilinear kernel within a bound derived from the formula."""
import argparse
import functools
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import swapnet_oracle as O
from swapnet_amd import engine
from swapnet_amd.datasets import gpu_augment as GA
from swapnet_amd.datasets import gpu_warp_batch as WB
from tests import backends

BACKENDS = [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)]

# body statistics in the range of the reference's norm_stats.json (nothing special about the digits: three inexact divisors)
MEAN = (0.7361263252139642, 0.6969182556788952, 0.6853540012984733)
STD = (0.3225722505292399, 0.3375028333422175, 0.3416956811706011)
LS = 32                                      # load size of the op-level cases: 23 x 19 sources grow to it, 40 x 30 shrink
MAP_KINDS = ("identity", "flips", "affine", "perspective", "chain4", "none")
f32 = np.float32


def _ctx(kind):
    return backends.gpu_ctx() if kind == "gpu" else backends.hostsim_ctx()


# ---- the reference chain, in this file's own words ---------------------------------------------------------------------------
def ref_onehot(labels, C):
    """to_onehot_tensor on (B,H,W) labels: label 0 and labels >= C give the all-zero vector."""
    lab = torch.from_numpy(labels.astype(np.int64))
    out = torch.zeros((lab.shape[0], C) + tuple(lab.shape[1:]), dtype=torch.float32)
    fg = (lab > 0) & (lab < C)
    out.scatter_(1, lab.clamp(0, C - 1)[:, None], fg[:, None].float())
    return out


def ref_texels(img_u8):
    """Normalize(ToTensor(img)) as (H,W,3) float32: three correctly rounded operations (numpy rounds each ufunc once)."""
    return (img_u8.astype(f32) / f32(255) - np.array(MEAN, dtype=f32)) / np.array(STD, dtype=f32)


def ref_axis(n_in, n_out):
    """torch's bilinear source positions along one axis (UpSample.h, align_corners False), in float32."""
    scale = f32(n_in) / f32(n_out)
    d = np.arange(n_out, dtype=f32)
    src = np.maximum(scale * (d + f32(0.5)) - f32(0.5), f32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(f32)
    return i0, i1, f32(1) - l1, l1


def ref_bilinear(t, ls):
    """F.interpolate(size=ls, mode="bilinear") of (H,W,3) float32 texels by the published formula, one float32 operation per step."""
    y0, y1, h0, h1 = ref_axis(t.shape[0], ls)
    x0, x1, w0, w1 = ref_axis(t.shape[1], ls)
    h0, h1, w0, w1 = h0[:, None, None], h1[:, None, None], w0[None, :, None], w1[None, :, None]
    a, b, c, d = t[y0][:, x0], t[y0][:, x1], t[y1][:, x0], t[y1][:, x1]
    out = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)
    assert out.dtype == f32
    return out


def ref_body(img_u8, ls):
    """(B,Hb,Wb,3) uint8 -> (B,3,ls,ls) float32."""
    return torch.from_numpy(np.stack([ref_bilinear(ref_texels(i), ls) for i in img_u8])).permute(0, 3, 1, 2).contiguous()


def ref_cloth(labels, C, maps, ls, backend="sim"):
    """one-hot, the per-channel chains at label resolution (swn_op_affine_gather of the backend at hand, which tests/test_augment.py
    holds to Pillow on both), F.interpolate's default nearest resize to the load size."""
    t = ref_onehot(labels, C)
    if maps is not None:
        t = GA.apply_maps(_ctx(backend), t, maps).cpu()
    return F.interpolate(t, size=ls)


def make_maps(kind, B, C, W, H, seed):
    """(B, C, nmaps, 9) table of one kind; None for "none"."""
    r = random.Random(seed)
    if kind == "none":
        return None
    if kind == "identity":
        return np.array([[[GA.IDENTITY] for _ in range(C)] for _ in range(B)], dtype=np.float64)
    if kind == "flips":             # both flips on even channels, one of them on odd ones (a chain of two either way)
        return np.array([[[GA.vflip_map(W, H), GA.hflip_map(W, H)] if c % 2 == 0 else [GA.hflip_map(W, H), GA.IDENTITY] if c % 4 == 1
                          else [GA.IDENTITY, GA.vflip_map(W, H)] for c in range(C)] for _ in range(B)], dtype=np.float64)
    if kind == "affine":            # RandomAffine's own draws per (sample, channel): rotation, shift, zoom out and shear leave the map
        center = (W * 0.5 + 0.5, H * 0.5 + 0.5)
        return np.array([[[GA.affine_map(GA.inverse_affine_matrix(center, *GA.random_affine_params(W, H, rng=r)))] for _ in range(C)]
                         for _ in range(B)], dtype=np.float64)
    if kind == "perspective":
        return np.array([[[[GA.KIND_PERSPECTIVE] + GA.perspective_coeffs(*GA.random_perspective_points(W, H, rng=r))] for _ in range(C)]
                         for _ in range(B)], dtype=np.float64)
    assert kind == "chain4"
    return GA.GpuPerChannelTransform("all", rng=r).draw_maps(B, C, W, H)


def make_labels(g, B, C, Hl, Wl):
    """Blocky label maps over 0 .. C - 1 with every label present, plus one value >= C (and 255) that must expand to nothing."""
    lab = g.randint(0, C, (B, Hl // 3 + 1, Wl // 3 + 1)).repeat(3, 1).repeat(3, 2)[:, :Hl, :Wl].astype(np.uint8)
    lab[:, 0, :C] = np.arange(C, dtype=np.uint8)               # (C <= Wl in every case here)
    lab[:, 1, 1], lab[:, 2, 3:5], lab[:, Hl - 1, Wl - 1] = C, 255, 0
    return lab


@functools.lru_cache(maxsize=None)
def op_case(Hl, Wl, Hb, Wb, cropped, C, backend="sim"):
    """Compact arrays of one B = 2 case and its reference tensors per (map kind, aliased) -- computed once, shared, never changed."""
    B = 2
    g = np.random.RandomState(1000 * Hl + 100 * Hb + 10 * C + cropped)
    body = g.randint(0, 256, (B, Hb, Wb, 3)).astype(np.uint8)
    body[0, 0, 0], body[0, 0, 1] = 0, 255                      # both ends of the byte range are present
    tgt, other = make_labels(g, B, C, Hl, Wl), make_labels(g, B, C, Hl, Wl)
    x_min, y_min, W, H = (3, 5, 20, 24) if cropped else (0, 0, LS, LS)
    crop = lambda t: t[:, :, y_min:y_min + H, x_min:x_min + W].contiguous()
    bodys, targets = crop(ref_body(body, LS)), crop(ref_cloth(tgt, C, None, LS))
    maps = {k: make_maps(k, B, C, Wl, Hl, seed=Hl + C + i) for i, k in enumerate(MAP_KINDS)}
    inputs = {(k, aliased): crop(ref_cloth(tgt if aliased else other, C, maps[k], LS, backend)) for k in MAP_KINDS for aliased in (True, False)}
    return dict(body=body, tgt=tgt, other=other, window=(x_min, y_min, W, H), C=C, maps=maps, bodys=bodys, targets=targets, inputs=inputs)


OP_CASES = [(hl, wl, hb, wb, cropped, C) for (hl, wl) in ((23, 19), (40, 30)) for (hb, wb) in ((23, 19), (40, 30)) for cropped in (1, 0)
            for C in (19, 6)]


def test_the_reference_chain_covers_the_edge_cases():
    """On the reference chain alone: the affine and perspective tables push part of the window outside the map and keep part of it
    inside, every kind changes the input, labels >= C and label 0 expand to nothing, and the pad channel case (C = 19) is there."""
    c = op_case(23, 19, 40, 30, 1, 19)
    ones = torch.ones(2, 19, 23, 19)
    for kind in ("affine", "perspective", "chain4"):
        hit = GA.apply_maps(backends.hostsim_ctx(), ones, c["maps"][kind]).cpu()
        assert 0.02 < float((hit == 0).float().mean()) < 0.9, kind            # some of every image comes from outside, some from inside
    for kind in ("flips", "affine", "perspective", "chain4"):
        assert not torch.equal(c["inputs"][kind, True], c["inputs"]["none", True]), kind
    assert torch.equal(c["inputs"]["identity", True], c["inputs"]["none", True]) and torch.equal(c["inputs"]["none", True], c["targets"])
    assert not torch.equal(c["inputs"]["none", False], c["targets"])
    t = ref_onehot(c["tgt"], 19)
    assert (c["tgt"] >= 19).any() and (c["tgt"] == 0).any()
    assert float(t[:, 0].abs().sum()) == 0 and float(t.sum(1)[torch.from_numpy(c["tgt"] >= 19)].sum()) == 0
    assert set(np.unique(c["tgt"])) >= set(range(19))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("Hl,Wl,Hb,Wb,cropped,C", OP_CASES)
def test_op_is_bit_identical_to_the_reference_chain(backend, Hl, Wl, Hb, Wb, cropped, C):
    ctx = _ctx(backend)
    c = op_case(Hl, Wl, Hb, Wb, cropped, C, backend)
    x_min, y_min, W, H = c["window"]
    tgt = torch.from_numpy(c["tgt"])
    for kind in MAP_KINDS:
        for aliased in (True, False):
            inp = tgt if aliased else torch.from_numpy(c["other"])
            bodys, inputs, targets = engine.op_warp_batch(ctx, c["body"], inp, tgt, c["maps"][kind], MEAN, STD, LS, x_min, y_min, H, W, C)
            for name, got, want in (("bodys", bodys, c["bodys"]), ("inputs", inputs, c["inputs"][kind, aliased]), ("targets", targets, c["targets"])):
                got = got.cpu()
                assert got.shape == want.shape, (kind, aliased, name, got.shape, want.shape)
                assert torch.equal(got, want), (kind, aliased, name, int((got != want).sum()), float((got - want).abs().max()))
    # without targets (an inference batch): the other two are what they were
    bodys, inputs, targets = engine.op_warp_batch(ctx, c["body"], tgt, None, c["maps"]["chain4"], MEAN, STD, LS, x_min, y_min, H, W, C)
    assert targets is None and torch.equal(bodys.cpu(), c["bodys"]) and torch.equal(inputs.cpu(), c["inputs"]["chain4", True])


# ---- the body arithmetic against torch -----------------------------------------------------------------------------------------
def _nchw(t):
    return torch.from_numpy(t).permute(2, 0, 1)[None].contiguous()


def body_bound(Hb, Wb, top):
    """3 roundings in each src, hence in each weight, times at most 2 max|texel| of slope, on two axes, plus four roundings of
    the blend."""
    return (12 * max(Hb, Wb) + 4) * 2.0 ** -24 * top


def test_the_restated_bilinear_formula_against_torch():
    """CPU: where every weight is 0 or 1 (size == load size) the restatement IS Normalize(ToTensor), and equals F.interpolate bit
    for bit; elsewhere it stays within the derived bound of torch's float64 kernel on the same float32 texels."""
    g = np.random.RandomState(5)
    t = ref_texels(g.randint(0, 256, (16, 16, 3)).astype(np.uint8))
    same = ref_bilinear(t, 16)
    assert np.array_equal(same, t)
    assert torch.equal(torch.from_numpy(same).permute(2, 0, 1)[None], F.interpolate(_nchw(t), size=16, mode="bilinear", align_corners=False))
    for hb, wb in ((23, 19), (40, 30), (100, 90)):
        t = ref_texels(g.randint(0, 256, (hb, wb, 3)).astype(np.uint8))
        for ls in (32, 72):
            want = F.interpolate(_nchw(t).double(), size=ls, mode="bilinear", align_corners=False)
            err = float((_nchw(ref_bilinear(t, ls)).double() - want).abs().max())
            bound = body_bound(hb, wb, float(np.abs(t).max()))
            print("restatement %dx%d -> %d: max |err| %.3e, bound %.3e" % (hb, wb, ls, err, bound))
            assert err <= bound, (hb, wb, ls, err, bound)


@pytest.mark.parametrize("backend", BACKENDS)
def test_body_against_torch_float64(backend):
    ctx = _ctx(backend)
    g = np.random.RandomState(9)
    lab = np.zeros((2, 8, 8), dtype=np.uint8)
    for hb, wb, ls in ((16, 16, 16), (23, 19, 32), (40, 30, 32), (100, 90, 72)):
        img = g.randint(0, 256, (2, hb, wb, 3)).astype(np.uint8)
        got = engine.op_warp_batch(ctx, img, lab, None, None, MEAN, STD, ls, 0, 0, ls, ls, 19)[0].cpu()
        tex = torch.from_numpy(np.stack([ref_texels(i) for i in img])).permute(0, 3, 1, 2).contiguous()
        if hb == ls and wb == ls:
            assert torch.equal(got, tex)                                # Normalize(ToTensor) exactly: every weight is 0 or 1
            continue
        want = F.interpolate(tex.double(), size=ls, mode="bilinear", align_corners=False)
        err, bound = float((got.double() - want).abs().max()), body_bound(hb, wb, float(tex.abs().max()))
        print("%s body %dx%d -> %d: max |err| %.3e, bound %.3e" % (backend, hb, wb, ls, err, bound))
        assert err <= bound, (hb, wb, ls, err, bound)


# ---- model hand-over -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_case(cropped, seed=0, backend="sim"):
    """B = 2 at 64 x 64 (the smallest the warp generator accepts): the compact batch dict + the reference tensors.  Cropped: a 72 x 72
    resized sample cut to 64 x 64 at (4, 4), sources of other sizes, a 4-map chain, another frame's map as the input (video mode).
    Uncropped: 64 x 64 sources, load size 64, no augmentation, the target map as the input (image mode)."""
    B, C = 2, 19
    g = np.random.RandomState(31 + cropped + 7 * seed)
    ls, (Hl, Wl), (Hb, Wb) = (72, (60, 80), (90, 70)) if cropped else (64, (64, 64), (64, 64))
    body = g.randint(0, 256, (B, Hb, Wb, 3)).astype(np.uint8)
    tgt = make_labels(g, B, C, Hl, Wl)
    inp = make_labels(g, B, C, Hl, Wl) if cropped else tgt
    maps = make_maps("chain4", B, C, Wl, Hl, seed=3 + seed) if cropped else None
    x_min, y_min = (4, 4) if cropped else (0, 0)
    crop = lambda t: t[:, :, y_min:y_min + 64, x_min:x_min + 64].contiguous()
    floats = (crop(ref_body(body, ls)), crop(ref_cloth(inp, C, maps, ls, backend)), crop(ref_cloth(tgt, C, None, ls)))
    t_tgt = torch.from_numpy(tgt)
    compact = {"bodys_u8": torch.from_numpy(body), "input_labels_u8": torch.from_numpy(inp) if cropped else t_tgt, "target_labels_u8": t_tgt,
               "maps": None if maps is None else torch.from_numpy(maps), "load_size": ls, "crop": (x_min, y_min, 64, 64),
               "norm_stats": (MEAN, STD), "cloth_paths": ["c0", "c1"], "body_paths": ["b0", "b1"]}
    return compact, floats


@functools.lru_cache(maxsize=None)
def warp_weights():
    torch.manual_seed(21)
    return O.warp_module_params(), O.patchgan_params(22)


def _poison(m):
    """Other values in every input slot, so that a buffer the hand-over under test fails to write cannot pass by inheritance."""
    for slot, t in enumerate(O.synth_warp_batch(2, 64, 64, seed=77)[: 3 if m.is_train else 2]):
        m.set_input(slot, t)


def _hand_over(m, compact_path, compact, floats):
    if compact_path:
        m.set_input_warp_batch(compact)
    else:
        for slot, t in enumerate(floats[: 3 if m.is_train else 2]):
            m.set_input(slot, t)


INPUT_TAPS = ("body", "cloth", "Dx", "slot_body", "slot_cloth", "slot_dx")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cropped", [1, 0])
def test_model_handover_equals_the_three_set_input_calls(backend, cropped):
    ctx = _ctx(backend)
    compact, floats = model_case(cropped, 0, backend)
    G, D = warp_weights()
    m = backends.get_model(ctx, "warp", 2, 64)
    runs = []
    ctx.lib.call("swn_slot_audit", 1)               # every launch of the step checks the slot it trusts against its operand
    try:
        for compact_path in (False, True):
            backends.reset_state(m, {engine.NET_G: G, engine.NET_D: D})
            _poison(m)
            _hand_over(m, compact_path, compact, floats)
            m.forward(False, 0)                     # (the fakes' slice of the conditional-D buffer is the generator's from here on)
            taps = [m.tap(engine.NET_G, k).cpu() for k in INPUT_TAPS]
            m.step([0.9, 0.8, 1.0], training=True, seed=3)
            ctx.sync()
            runs.append((taps, m.losses(), m.grad_arena(engine.NET_D).cpu().clone(), m.output().cpu()))
    finally:
        ctx.lib.call("swn_slot_audit", 0)
    (ta, la, ga, oa), (tb, lb, gb, ob) = runs
    for name, a, b in zip(INPUT_TAPS, ta, tb):
        assert a.shape == b.shape and torch.equal(a, b), (name, int((a != b).sum()))
    body, cloth, dx = tb[:3]
    assert torch.equal(body[:, :3], floats[0]) and float(body[:, 3:].abs().sum()) == 0          # the reference tensors, pads zero
    assert torch.equal(cloth[:, :19], floats[1]) and float(cloth[:, 19:].abs().sum()) == 0
    assert torch.equal(dx[2:, :19], floats[2]) and torch.equal(dx[2:, 20:23], floats[0]) and torch.equal(dx[:2, 20:23], floats[0])
    assert float(tb[3].max()) == float(floats[0].abs().max()) and float(tb[4].max()) == 1.0     # the slots hold the operands' amax
    assert la == lb and all(np.isfinite(v) for v in la.values()), (la, lb)
    assert torch.equal(ga, gb) and float(ga.abs().sum()) > 0
    assert torch.equal(oa, ob)


@pytest.mark.parametrize("backend", BACKENDS)
def test_inference_model_takes_a_batch_without_targets(backend):
    ctx = _ctx(backend)
    compact, floats = model_case(1, 0, backend)
    G, _ = warp_weights()
    mi = backends.get_model(ctx, "warp", 2, 64, is_train=False)
    mi.load_state_dict(engine.NET_G, G)
    runs = []
    for compact_path in (False, True):
        _poison(mi)
        _hand_over(mi, compact_path, dict(compact, target_labels_u8=None), floats)
        mi.forward(False, 0)
        runs.append([mi.tap(engine.NET_G, k).cpu() for k in INPUT_TAPS] + [mi.output().cpu()])
    for name, a, b in zip(INPUT_TAPS + ("fakes",), *runs):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert runs[1][2].shape[0] == 2                 # the conditional buffer has no target half: nothing of a target is written


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_batch_handed_over_between_the_phases_of_a_step(backend):
    """forward, backward_D, AdamW(D), a NEW batch, backward_G, AdamW(G): the cross-entropy term taken early (behind the
    discriminator's backward pass) was taken against the old targets and must be taken again -- the hand-over resets it like
    set_input(2, ...) does."""
    ctx = _ctx(backend)
    first, second = model_case(1, 0, backend), model_case(1, 1, backend)
    assert not torch.equal(first[1][2], second[1][2])
    G, D = warp_weights()
    m = backends.get_model(ctx, "warp", 2, 64)
    runs = []
    for compact_path in (False, True):
        backends.reset_state(m, {engine.NET_G: G, engine.NET_D: D})
        _hand_over(m, compact_path, *first)
        m.forward(True, 3)
        m.backward_D(0.9, 0.8)
        m.optimizer_step(engine.NET_D)
        _hand_over(m, compact_path, *second)
        m.backward_G(1.0)
        ctx.sync()
        grads = m.grad_arena(engine.NET_G).cpu().clone()
        m.optimizer_step(engine.NET_G)
        ctx.sync()
        runs.append((m.losses(), grads, m.arena(engine.NET_G, engine.W_WEIGHT).cpu().clone()))
    (la, ga, wa), (lb, gb, wb) = runs
    assert la == lb and all(np.isfinite(v) for v in la.values()), (la, lb)
    assert torch.equal(ga, gb) and float(ga.abs().sum()) > 0 and torch.equal(wa, wb)


# ---- Python surface ------------------------------------------------------------------------------------------------------------
def _opt(**kw):
    o = dict(input_transforms=("hflip", "vflip", "affine", "perspective"), load_size=72, crop_size=64, crop_bounds=None,
             body_norm_stats=(MEAN, STD), cloth_channels=19, is_train=True)
    o.update(kw)
    return argparse.Namespace(**o)


def _samples(cropped, own_input=None, backend="sim"):
    compact, _ = model_case(cropped, 0, backend)
    own_input = bool(cropped) if own_input is None else own_input
    out = []
    for b in range(2):
        s = {"body_u8": compact["bodys_u8"][b].numpy(), "target_labels_u8": compact["target_labels_u8"][b].numpy(), "paths": ("c%d" % b, "b%d" % b)}
        if own_input:
            s["input_labels_u8"] = compact["input_labels_u8"][b].numpy()
        out.append(s)
    return out


class RecordingRandom(random.Random):
    """random.Random that logs every public draw with its arguments."""

    def __init__(self, seed):
        super().__init__(seed)
        self.log = []

    def random(self):
        self.log.append(("random",))
        return super().random()

    def uniform(self, a, b):
        self.log.append(("uniform", a, b))
        return super().uniform(a, b)

    def randint(self, a, b):
        self.log.append(("randint", a, b))
        return super().randint(a, b)

    def shuffle(self, x):
        self.log.append(("shuffle", len(x)))
        return super().shuffle(x)


def test_collate_draws_the_maps_with_the_reference_rng_call_for_call():
    rng = RecordingRandom(7)
    batch = WB.GpuWarpBatch(_opt(), rng=rng).collate(_samples(1))
    ref = RecordingRandom(7)
    want = GA.GpuPerChannelTransform(("hflip", "vflip", "affine", "perspective"), rng=ref).draw_maps(2, 19, 80, 60)     # (B, C, Wl, Hl)
    assert rng.log == ref.log and sum(1 for e in rng.log if e[0] == "shuffle") == 2 * 19       # one RandomOrder per (sample, channel)
    assert rng.random() == ref.random()
    assert batch["maps"].dtype == torch.float64 and tuple(batch["maps"].shape) == (2, 19, 4, 9)
    assert np.array_equal(batch["maps"].numpy(), want)
    # no transforms, and an inference batch: nothing is drawn
    for opt in (_opt(input_transforms="none"), _opt(is_train=False)):
        rng = RecordingRandom(7)
        assert WB.GpuWarpBatch(opt, rng=rng).collate(_samples(1))["maps"] is None and rng.log == []
    # a given table is used as it is
    rng = RecordingRandom(7)
    assert np.array_equal(WB.GpuWarpBatch(_opt(), rng=rng).collate(_samples(1), maps=want)["maps"].numpy(), want) and rng.log == []
    wb = WB.GpuWarpBatch(_opt())
    assert wb.crop_bounds == ((4, 4), (68, 68)) and WB.GpuWarpBatch(_opt(load_size=64)).crop_bounds is None
    from swapnet_amd.datasets.gpu_texture_batch import GpuTextureBatch
    assert WB.GpuWarpBatch._parse_crop_bounds is GpuTextureBatch._parse_crop_bounds             # shared, not copied


@pytest.mark.parametrize("backend", BACKENDS)
def test_collate_and_expand_give_the_reference_form(backend):
    ctx = _ctx(backend)
    compact, floats = model_case(1, 0, backend)
    wb = WB.GpuWarpBatch(_opt(), ctx=ctx)
    batch = wb.collate(_samples(1, backend=backend), maps=compact["maps"].numpy())
    assert set(batch) == {"bodys_u8", "input_labels_u8", "target_labels_u8", "maps", "load_size", "crop", "norm_stats", "cloth_paths", "body_paths"}
    for k in ("bodys_u8", "input_labels_u8", "target_labels_u8", "maps"):
        assert torch.equal(batch[k], compact[k]) and batch[k].dtype == compact[k].dtype, k
    assert batch["crop"] == compact["crop"] and batch["load_size"] == 72 and batch["cloth_paths"] == ["c0", "c1"] and batch["body_paths"] == ["b0", "b1"]
    ref = wb.expand(batch)
    assert set(ref) == {"body_paths", "bodys", "cloth_paths", "input_cloths", "target_cloths"}                 # warp_dataset.py:177-183
    for k, want in zip(("bodys", "input_cloths", "target_cloths"), floats):
        assert ref[k].dtype == torch.float32 and ref[k].shape == want.shape and torch.equal(ref[k].cpu(), want), k
    # image mode: no input map of its own -> the target's tensor itself, and the uncropped window is the whole resized sample
    image = WB.GpuWarpBatch(_opt(load_size=64, input_transforms="none"), ctx=ctx).collate(_samples(0))
    assert image["input_labels_u8"] is image["target_labels_u8"] and image["crop"] == (0, 0, 64, 64) and image["maps"] is None
    for k, want in zip(("bodys", "input_cloths", "target_cloths"), model_case(0)[1]):
        assert torch.equal(WB.expand_batch(ctx, image)[k].cpu(), want), k


@pytest.mark.small_channel_winograd
@pytest.mark.parametrize("backend", BACKENDS)
def test_create_model_trains_on_compact_batches_like_on_their_expansion(backend, tmp_path):
    from swapnet_amd.models import create_model
    from tests.test_models_api import make_opt
    batches = [model_case(1, 0, backend)[0], model_case(1, 1, backend)[0]]
    floats = model_case(1, 1, backend)[1]
    losses, models = [], []
    for form in ("compact", "reference"):
        opt = make_opt(tmp_path, backend, body_norm_stats=(MEAN, STD), load_size=72)
        torch.manual_seed(11)
        model = create_model(opt)
        model.eval()
        wb = WB.GpuWarpBatch(opt, ctx=model.backend.ctx)
        torch.manual_seed(5)
        per_step = []
        for compact in batches:                                     # two steps
            model.set_input(compact if form == "compact" else wb.expand(compact))
            model.optimize_parameters()
            per_step.append(model.get_current_losses())
        losses.append(per_step)
        models.append(model)
    assert losses[0] == losses[1] and all(np.isfinite(v) for s in losses[0] for v in s.values()), losses
    assert torch.equal(models[0].fakes.cpu(), models[1].fakes.cpu())
    m = models[0]
    assert m.get_image_paths() == (("c0", "b0"), ("c1", "b1"))
    assert m._bodys is None and m._inputs is None and m._targets is None          # nothing was expanded on the training path
    m.compute_visuals()
    vis = m.get_current_visuals()
    assert set(vis) == {"inputs_decoded", "bodys_unnormalized", "fakes_decoded", "targets_decoded"}
    assert torch.equal(m.bodys.cpu(), floats[0]) and torch.equal(m.inputs.cpu(), floats[1]) and torch.equal(m.targets.cpu(), floats[2])
    assert torch.equal(vis["inputs_decoded"].cpu(), O.decode_cloth_labels(floats[1]))
    # ... and the float hand-over afterwards is today's path: plain attributes again
    m.set_input(wb.expand(batches[0]))
    assert m._compact is None and torch.equal(m.bodys.cpu(), model_case(1, 0, backend)[1][0])


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(backend):
    ctx = _ctx(backend)
    c = op_case(23, 19, 23, 19, 1, 19, backend)
    tgt = torch.from_numpy(c["tgt"])
    args = (c["body"], tgt, tgt, None, MEAN, STD, LS)
    for x_min, y_min, H, W in ((13, 5, 24, 20), (3, 9, 24, 20), (-1, 0, 24, 20), (0, 0, 33, 32)):          # a 32 x 32 resized sample
        with pytest.raises(ValueError, match="crop window"):
            engine.op_warp_batch(ctx, *args, x_min, y_min, H, W, 19)
    for channels in (1, 65):
        with pytest.raises(ValueError, match="cloth channels"):
            engine.op_warp_batch(ctx, *args, 3, 5, 24, 20, channels)
    # a table announced (nmaps 4) but not handed over -- at the C boundary, where it can happen
    dev = [torch.as_tensor(t).to(ctx.device).contiguous() for t in (c["body"], tgt)]
    out = [torch.empty((2, n, 24, 20), dtype=torch.float32, device=ctx.device) for n in (3, 19, 19)]
    C, ptr = engine.C, engine._C.ptr
    with pytest.raises(ValueError, match="NULL map table"):
        ctx.lib.call("swn_op_warp_batch", ctx.handle, ptr(dev[0]), 2, 23, 19, ptr(dev[1]), ptr(dev[1]), 23, 19, None, 4, (C.c_float * 3)(*MEAN),
                     (C.c_float * 3)(*STD), LS, 3, 5, 24, 20, 19, ptr(out[0]), ptr(out[1]), ptr(out[2]))
    compact, _ = model_case(1, 0, backend)
    tex = backends.get_model(ctx, "texture", 2, 64, is_train=False)
    with pytest.raises(ValueError, match="only the warp model takes a warp batch"):
        tex.set_input_warp_batch(compact)
    m = backends.get_model(ctx, "warp", 2, 64, is_train=False)
    with pytest.raises(ValueError, match="batch"):
        m.set_input_warp_batch({k: (v[:1] if torch.is_tensor(v) else v) for k, v in compact.items()})
    with pytest.raises(ValueError, match="crop window"):
        m.set_input_warp_batch(dict(compact, crop=(4, 4, 32, 32)))                 # not the model's window
    with pytest.raises(ValueError, match="crop window"):
        m.set_input_warp_batch(dict(compact, crop=(9, 4, 64, 64)))                 # 9 + 64 > 72
    with pytest.raises(ValueError, match="crop window"):
        m.set_input_warp_batch(dict(compact, load_size=32))                        # the window does not fit the resized sample at all
    with pytest.raises(ValueError, match="maps must be"):
        m.set_input_warp_batch(dict(compact, maps=compact["maps"][:, :6]))
    with pytest.raises(ValueError, match="RGB"):
        m.set_input_warp_batch(dict(compact, bodys_u8=compact["bodys_u8"][..., :2]))
    four = engine.NativeModel(ctx, "warp", 2, 64, 64, is_train=False, body_channels=4)
    try:
        with pytest.raises(ValueError, match="4 body channels"):
            four.set_input_warp_batch(compact)
    finally:
        four.close()
    samples = _samples(1, backend=backend)
    samples[1] = dict(samples[1], target_labels_u8=samples[1]["target_labels_u8"][:-1])
    with pytest.raises(ValueError, match="label maps"):
        WB.GpuWarpBatch(_opt()).collate(samples)
