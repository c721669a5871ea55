"""Every SWN_* route switch, held to its contract.

The library picks kernels and launch order per layer; shape decides most of it, the SWN_* environment switches the rest.  A
switch selects a TESTED configuration only if some test runs it, so SWITCHES below has one row per switch:

  values    the non-default values that matter
  read      when the library reads it: "launch" (every launch), "layer" (when a layer / net is built), "model" (when a model is
            built), "context" (when a context is created) or "process" (once per process: a `static const`)
  contract  "numerics"  another kernel or another summation order, held to float64 at the bars of the default route
            "bit"       the same arithmetic in another order or place, held to the default step with torch.equal
            "diagnostic" the simulator's own report switches (no arithmetic)
  tests     the tests that enforce it ("file::name")

test_registry_* (CPU) keep the table complete: its keys are conftest.ROUTING_SWITCHES, every getenv("SWN_...") of the library
and of the host simulator is in it, and every test it names exists.  A switch read once per process or per context runs in a
child process (tests/switch_child.py): one at a time, each under its own timeout; a child that ends on a signal or a timeout
fails the test at once and no further child starts.
"""
import ast
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import split_model as S
from oracle import swapnet_oracle as O
from swapnet_amd import engine
from tests import backends
from tests.conftest import ROUTING_SWITCHES
from tests.switch_child import conv_call, phased_step, run_conv_case

REPO = backends.REPO
HERE = "tests/test_route_switches.py::"

SWITCHES = {
    # ---- kernel and algorithm routes: numerics ----
    "SWN_WINO_MINC": dict(values=("32",), read="layer", contract="numerics",
                          tests=("tests/test_warp_step.py::test_warp_forward_levels",
                                 "tests/test_train_parity.py::test_warp_c2_full_batch_step_with_winograd_forms_on_every_level")),
    "SWN_WINOGRAD": dict(values=("0",), read="layer", contract="numerics",
                         tests=("tests/test_warp_step.py::test_resblock_conv_variants_match_oracle",
                                "tests/test_warp_step.py::test_fast_algorithms_track_the_direct_kernels_over_training_steps")),
    "SWN_WINO_M": dict(values=("2",), read="layer", contract="numerics",
                       tests=("tests/test_warp_step.py::test_resblock_conv_variants_match_oracle",)),
    "SWN_WINO_S2": dict(values=("0", "2"), read="layer", contract="numerics",
                        tests=(HERE + "test_winograd_switches_against_the_pinned_float64_oracle",)),
    "SWN_TAIL4": dict(values=("0",), read="launch", contract="numerics",
                      tests=("tests/test_warp_step.py::test_fast_algorithms_track_the_direct_kernels_over_training_steps",)),
    "SWN_HEAD_TAPN": dict(values=("0",), read="layer", contract="numerics",
                          tests=("tests/test_warp_step.py::test_fast_algorithms_track_the_direct_kernels_over_training_steps",)),
    "SWN_NARROW": dict(values=("0",), read="launch", contract="numerics",
                       tests=("tests/test_warp_step.py::test_fast_algorithms_track_the_direct_kernels_over_training_steps",)),
    "SWN_SPLIT": dict(values=("0",), read="launch", contract="numerics",
                      tests=("tests/test_ops.py::test_split_main_loop_is_as_accurate_as_the_f32_mfma",
                             "tests/test_ops.py::test_two_plane_form_on_heavy_tailed_operands")),
    "SWN_DMA": dict(values=("0",), read="process", contract="numerics",
                    tests=(HERE + "test_once_per_process_kernel_routes_against_float64",)),
    "SWN_DMA_WIDE": dict(values=("0", "2"), read="launch", contract="numerics",
                         tests=("tests/test_ops.py::test_conv_wide_ring_tile", HERE + "test_per_launch_kernel_routes_against_float64")),
    "SWN_PRECUT": dict(values=("0",), read="process", contract="numerics",
                       tests=(HERE + "test_once_per_process_kernel_routes_against_float64",
                              HERE + "test_precut_switch_is_read_once_in_a_running_process",
                              HERE + "test_model_level_switches_on_the_host_simulator")),
    "SWN_PAIR": dict(values=("0",), read="process", contract="numerics",
                     tests=(HERE + "test_winograd_switches_against_the_pinned_float64_oracle",)),
    "SWN_TAIL_SPLIT": dict(values=("0", "2"), read="launch", contract="numerics",
                           tests=(HERE + "test_per_launch_kernel_routes_against_float64",)),
    "SWN_PHASE4": dict(values=("0",), read="launch", contract="numerics",
                       tests=(HERE + "test_per_launch_kernel_routes_against_float64",)),
    "SWN_AMAX_FUSED": dict(values=("0",), read="launch", contract="numerics",      # (and "layer": no pair-form planes are planned)
                           tests=(HERE + "test_winograd_switches_against_the_pinned_float64_oracle",)),
    "SWN_PC_PLANES": dict(values=("1",), read="process", contract="numerics",
                          tests=(HERE + "test_one_plane_form_element_bound_on_the_mi355x",
                                 "tests/test_pattern_replay.py::test_one_plane_configuration_tolerance_study")),
    "SWN_WGRAD_PLANES": dict(values=("1",), read="launch", contract="numerics",
                             tests=(HERE + "test_one_plane_form_element_bound_on_the_mi355x",
                                    "tests/test_split_numerics.py::test_one_plane_form_element_bound",
                                    "tests/test_pattern_replay.py::test_one_plane_configuration_tolerance_study")),
    "SWN_CONV_STATS": dict(values=("0",), read="model", contract="numerics",
                           tests=("tests/test_train_parity.py::test_conv_epilogue_instance_norm_statistics_match_the_statistics_pass",)),
    "SWN_ROI_WAVE": dict(values=("0",), read="launch", contract="bit",
                         tests=("tests/test_ops.py::test_wavefront_gather_roi_align_is_bit_identical",)),
    # ---- scheduling: the same arithmetic in another order or place ----
    "SWN_PREFETCH": dict(values=("0", "3"), read="process", contract="bit",
                         tests=(HERE + "test_scheduling_switches_are_bit_identical_on_the_mi355x",
                                HERE + "test_model_level_switches_on_the_host_simulator")),
    "SWN_PREFETCH_AHEAD": dict(values=("1",), read="process", contract="bit",
                               tests=(HERE + "test_scheduling_switches_are_bit_identical_on_the_mi355x",
                                      HERE + "test_model_level_switches_on_the_host_simulator")),
    "SWN_BIAS_MAIN": dict(values=("0",), read="process", contract="bit",
                          tests=(HERE + "test_scheduling_switches_are_bit_identical_on_the_mi355x",
                                 HERE + "test_model_level_switches_on_the_host_simulator")),
    "SWN_VT_EARLY": dict(values=("0",), read="process", contract="bit",
                         tests=(HERE + "test_scheduling_switches_are_bit_identical_on_the_mi355x",
                                HERE + "test_model_level_switches_on_the_host_simulator")),
    "SWN_OVERLAP": dict(values=("0",), read="context", contract="bit",
                        tests=(HERE + "test_scheduling_switches_are_bit_identical_on_the_mi355x",)),
    "SWN_PHASE_ZFAST": dict(values=("0",), read="launch", contract="bit",
                            tests=(HERE + "test_scheduling_switches_are_bit_identical_on_the_mi355x",)),
    "SWN_IN_PAIR_XCD": dict(values=("0",), read="launch", contract="bit",
                            tests=(HERE + "test_scheduling_switches_are_bit_identical_on_the_mi355x",)),
    "SWN_CE_EARLY": dict(values=("0",), read="model", contract="bit",
                         tests=("tests/test_warp_step.py::test_early_cross_entropy_term_is_the_same_step",
                                HERE + "test_new_targets_between_backward_d_and_backward_g")),
    "SWN_STREAM_ADAMW": dict(values=("0", "1", "2"), read="launch", contract="bit",
                             tests=("tests/test_captured_step.py::test_adamw_streamed_behind_each_bucket_is_the_same_step",)),
    # ---- the host simulator's own switches ----
    "SWN_SIM_PAIR": dict(values=("1",), read="launch", contract="numerics",
                         tests=("tests/test_ops.py::test_two_plane_form_on_heavy_tailed_operands",
                                "tests/test_pattern_replay.py::test_gradients_with_pinned_pattern_under_the_simulated_16_bit_operand_formats")),
    "SWN_SIM_SLOT_REPORT": dict(values=("1e30",), read="launch", contract="diagnostic",
                                tests=("tests/test_pattern_replay.py::test_gradients_with_pinned_pattern_under_the_simulated_16_bit_operand_formats",)),
}
# read by the library but selecting no computation: detailed launch labels, the simulator's per-operation timings
DIAGNOSTICS = ("SWN_PROF_DETAIL", "SWN_SIM_TIMES")


# ---- the registry -------------------------------------------------------------------------------------------------------------
def test_registry_covers_exactly_the_switches_the_suite_scrubs():
    assert set(SWITCHES) == set(ROUTING_SWITCHES), (sorted(set(ROUTING_SWITCHES) - set(SWITCHES)), sorted(set(SWITCHES) - set(ROUTING_SWITCHES)))
    for k, row in SWITCHES.items():
        assert row["values"] and row["tests"], k
        assert row["read"] in ("launch", "layer", "model", "context", "process"), k
        assert row["contract"] in ("numerics", "bit", "diagnostic"), k


def test_registry_knows_every_switch_the_library_reads():
    read = set()
    for d in (os.path.join(REPO, "swapnet_amd", "csrc"), os.path.join(REPO, "tests", "hostsim")):
        for f in sorted(os.listdir(d)):
            if f.endswith((".cpp", ".hip", ".h")):
                with open(os.path.join(d, f)) as fh:
                    read |= set(re.findall(r'getenv\(\s*"(SWN_[A-Z0-9_]+)"', fh.read()))
    assert read >= {"SWN_DMA", "SWN_PRECUT", "SWN_PREFETCH"}          # (the pattern still finds the reads)
    unknown = sorted(read - set(SWITCHES) - set(DIAGNOSTICS))
    assert not unknown, ("switches read by the library without a row in SWITCHES (and so without a test)", unknown)


def test_registry_names_tests_that_exist():
    defs = {}
    for row in SWITCHES.values():
        for t in row["tests"]:
            path, name = t.split("::")
            if path not in defs:
                with open(os.path.join(REPO, path)) as fh:
                    defs[path] = {n.name for n in ast.walk(ast.parse(fh.read())) if isinstance(n, ast.FunctionDef)}
            assert name in defs[path], t


def test_every_switch_is_set_by_some_test():
    """Each non-default value of every switch appears in a test that sets it (monkeypatch.setenv, a child's env, or the
    small_channel_winograd marker for SWN_WINO_MINC)."""
    text = ""
    tdir = os.path.join(REPO, "tests")
    for f in sorted(os.listdir(tdir)):
        if f.startswith("test_") and f.endswith(".py"):
            with open(os.path.join(tdir, f)) as fh:
                src = fh.read()
            if f == "test_route_switches.py":                       # (the table itself sets nothing)
                src = src[:src.index("\nSWITCHES = {")] + src[src.index("\nDIAGNOSTICS = "):]
            text += src
    for k, row in SWITCHES.items():
        if k == "SWN_WINO_MINC":
            assert "@pytest.mark.small_channel_winograd" in text
            continue
        assert '"%s"' % k in text, (k, "no test sets it")


# ---- helpers ----------------------------------------------------------------------------------------------------------------
K4S2, K3REFL, K4S1, K3ZERO = 0, 1, 2, 3
CHILD_TIMEOUT_S = 240


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def run_child(tmp_path, name, job, spec, env, sim=False):
    """One child process with exactly `env`'s SWN_* switches; its results.  A signal or a timeout fails the test at once."""
    src, dst = str(tmp_path / (name + ".in.pt")), str(tmp_path / (name + ".out.pt"))
    torch.save(spec, src)
    full = {k: v for k, v in os.environ.items() if not k.startswith("SWN_")}
    full.update(env)
    cmd = [sys.executable, "-m", "tests.switch_child", job, src, dst] + (["sim"] if sim else [])
    try:
        p = subprocess.run(cmd, cwd=REPO, env=full, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        pytest.fail("child %s (%s) timed out after %d s" % (name, env, CHILD_TIMEOUT_S))
    if p.returncode < 0:
        pytest.fail("child %s (%s) ended on signal %d:\n%s" % (name, env, -p.returncode, p.stderr[-3000:]))
    assert p.returncode == 0, (name, env, p.stdout[-2000:], p.stderr[-3000:])
    return torch.load(dst, weights_only=False)


def ref_conv64(kind, tr, x, w, b=None):
    x, w = x.double(), w.double()
    b = b.double() if b is not None else None
    if tr:
        return F.conv_transpose2d(x, w, b, stride=2, padding=1)
    if kind == K4S2:
        return F.conv2d(x, w, b, stride=2, padding=1)
    if kind == K3REFL:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)
    return F.conv2d(x, w, b, stride=1, padding=1)          # K4S1 (4x4, pad 1) and K3ZERO (3x3, pad 1)


def make_case(seed, kind, tr, n, ci, h, co, bias):
    g = torch.Generator().manual_seed(seed)
    k = 3 if kind in (K3REFL, K3ZERO) else 4
    x = torch.randn(n, ci, h, h, generator=g)
    w = torch.randn((ci, co, k, k) if tr else (co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5
    b = torch.randn(co, generator=g) * 0.1 if bias else None
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = ref_conv64(kind, tr, xr, wr, b)
    dy = torch.randn(y.shape, generator=g)
    gx, gw = torch.autograd.grad(y, (xr, wr), dy.double())
    return dict(kind=kind, tr=tr, x=x, w=w, b=b, dy=dy, y_shape=tuple(y.shape), desc=(kind, tr, n, ci, h, co),
                ref=dict(y=y.detach(), dx=gx, dw=gw))


# the bars test_ops.py holds the default route to: forward 1e-4, both gradients 2e-4 (rel-L2 against the reference)
BARS = dict(y=1e-4, dx=2e-4, dw=2e-4)


def check_route_case(case, base, got, switch):
    """float64 errors of the default route (`base`) and the switched one (`got`) at the test_ops bars; prints both."""
    for what, bar in BARS.items():
        e0, e1 = rel(base[what], case["ref"][what]), rel(got[what], case["ref"][what])
        print("%-22s %-28s %-3s  float64 rel-L2: default %.2e  switched %.2e" % (switch, case["desc"], what, e0, e1))
        assert e1 < bar, (switch, case["desc"], what, e1)


def assert_route_changed(switch, base_lines, got_lines, removed=(), added=()):
    """The switch took effect: the launch list differs from the default one, the family it removes is gone (and was there by
    default), the family it adds is present."""
    assert base_lines != got_lines, (switch, "launch list identical to the default route: the switch changed nothing")
    only0 = [l for l in base_lines if l not in got_lines]
    only1 = [l for l in got_lines if l not in base_lines]
    print("%s route: %d default-only launches, e.g. %s; %d switched-only, e.g. %s" % (switch, len(only0), only0[:2], len(only1), only1[:2]))
    if removed:
        assert any(fam in l for fam in removed for l in base_lines), (switch, removed, "not in the default route: pick a case where the switch acts")
    for fam in removed:
        assert not any(fam in l for l in got_lines), (switch, fam, "still launched under the switch")
    for fam in added:
        assert any(fam in l for l in got_lines), (switch, fam, "not launched under the switch")


# operator cases the product runs (Ci 256 .. 1024, N 64 .. 1024, ragged M, four-phase transposed convs, Winograd layers)
PRODUCT_CASES = [
    (K4S2, 0, 2, 512, 8, 1024, False),        # Ci 512 -> N 1024, split-K
    (K4S1, 0, 2, 256, 16, 512, True),         # PatchGAN model.8: 15 x 15 outputs (ragged M)
    (K4S2, 1, 2, 256, 8, 128, False),         # four-phase transposed conv, N 128
    (K4S2, 0, 2, 128, 32, 64, True),          # N 64 (256 x 64 tiles)
    (K4S2, 0, 1, 64, 32, 96, True),           # N 96
    (K3REFL, 0, 1, 256, 32, 256, True),       # resblock conv on the product's Winograd form F(4x4,3x3): 64 tiles, pair-form planes
    (K3REFL, 0, 1, 1024, 16, 256, False),     # the same from Ci 1024 (16 tiles)
]


@pytest.fixture(scope="module")
def product_cases():
    return [make_case(100 + i, *c) for i, c in enumerate(PRODUCT_CASES)]


def _default_runs(ctx, cases):
    return [run_conv_case(ctx, c) for c in cases]


def _strip(cases):
    return dict(cases=[{k: v for k, v in c.items() if k != "ref"} for c in cases])


# ---- 2. kernel routes against float64 --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_once_per_process_kernel_routes_against_float64(product_cases, tmp_path):
    """SWN_DMA=0 (no LDS-DMA / pre-cut ring kernels: the register-staged kernels), SWN_PRECUT=0 (no pre-cut ring kernel: the
    LDS-DMA kernel cuts both operands in its loop) are read once per process:
    each runs the product cases in its own child process; forward, input gradient and weight gradient against float64 at the
    bars of the default route, and the route must show the switch took effect."""
    ctx = backends.gpu_ctx()
    base = _default_runs(ctx, product_cases)
    spec = _strip(product_cases)
    for env, removed, added in (({"SWN_DMA": "0"}, ("conv_fwd_dma_", "conv_fwd_pc_", "conv_wgrad_dma_"), ("conv_fwd_",)),
                                ({"SWN_PRECUT": "0"}, ("conv_fwd_pc_",), ("conv_fwd_dma_",))):
        name = "_".join("%s%s" % kv for kv in env.items())
        got = run_child(tmp_path, name, "ops", spec, env)
        assert_route_changed(name, sum((b["route"] for b in base), []), sum((g["route"] for g in got), []), removed, added)
        for case, b, g in zip(product_cases, base, got):
            check_route_case(case, b, g, name)


@pytest.mark.gpu
def test_precut_switch_is_read_once_in_a_running_process(product_cases, monkeypatch):
    """SWN_PRECUT decides at build time which weight operands exist only in pre-cut form; a launch that re-read it later would run
    the fall-back on operands prepared for the pre-cut kernel.  So the device reads it once per process (conv_gemm.hip pc_on):
    set in a running process it must change neither the route nor a single bit (the child-process test runs the fall-back)."""
    ctx = backends.gpu_ctx()
    cases = product_cases[:3]
    base = _default_runs(ctx, cases)
    monkeypatch.setenv("SWN_PRECUT", "0")
    got = _default_runs(ctx, cases)
    for b, g in zip(base, got):
        assert b["route"] == g["route"]
        assert any("conv_fwd_pc_" in l for l in g["route"])
        for what in ("y", "dx", "dw"):
            assert torch.equal(b[what], g[what]), what


# per-launch switches: (env, cases, families removed, families added)
TAIL_CASES = [(K3ZERO, 0, 1, 64, 384, 64, False),     # 576 tiles of 256 x 64 on 512 slots: one whole round + a ragged tail
              (K3ZERO, 0, 3, 128, 160, 64, False)]    # 300 tiles: more than half a round, no whole one
PHASE4_CASES = [(K4S2, 1, 1, 128, 32, 3, True),      # the texture U-Net's outermost up conv (3 columns)
                (K4S2, 1, 2, 64, 16, 19, True)]      # 19 columns (20 padded)
WIDE_CASES = [(K3ZERO, 0, 1, 16, 160, 512, False)]   # 800 tiles of 128 x 128 on 768 slots, 400 of 128 x 256 on 512


@pytest.fixture(scope="module")
def launch_cases():
    return dict(tail=[make_case(200 + i, *c) for i, c in enumerate(TAIL_CASES)],
                phase4=[make_case(210 + i, *c) for i, c in enumerate(PHASE4_CASES)],
                wide=[make_case(220 + i, *c) for i, c in enumerate(WIDE_CASES)])


@pytest.mark.gpu
def test_per_launch_kernel_routes_against_float64(product_cases, launch_cases, monkeypatch):
    """Switches read per launch, set in-process:
      SWN_TAIL_SPLIT=0 splits every ragged last round along K, =2 only one that runs behind no whole round (the launch labels
      carry the split under a route trace: full / tail N x s);
      SWN_PHASE4=0 runs the narrow four-phase transposed conv as one launch per phase (no conv_fwd_phase4_narrow);
      SWN_DMA_WIDE=0 never takes the 128 x 256 ring tile -- which the cost model picks only on the f32-MFMA form, so both sides run
      under SWN_SPLIT=0.
    (SWN_PAIR and SWN_AMAX_FUSED change the storage of Winograd planes, which an operator-level net does not plan in pair form:
    test_winograd_switches_against_the_pinned_float64_oracle holds them at model level.)"""
    ctx = backends.gpu_ctx()
    direct = {"SWN_WINOGRAD": "0"}          # (both sides: the tail cases are Winograd-eligible 3x3 convs)
    plans = [("SWN_TAIL_SPLIT=0", {"SWN_TAIL_SPLIT": "0"}, direct, launch_cases["tail"][:1], (), (), "tail"),
             ("SWN_TAIL_SPLIT=2", {"SWN_TAIL_SPLIT": "2"}, direct, launch_cases["tail"][1:], (), (), "tail"),
             ("SWN_PHASE4=0", {"SWN_PHASE4": "0"}, {}, launch_cases["phase4"], ("conv_fwd_phase4_narrow",), ("conv_fwd_narrow",), None),
             ("SWN_DMA_WIDE=0", {"SWN_DMA_WIDE": "0"}, dict(direct, SWN_SPLIT="0"), launch_cases["wide"], ("conv_fwd_dma_128x256",),
              ("conv_fwd_dma_128x128",), None)]
    for name, env, common, cases, removed, added, split in plans:
        for k, v in common.items():
            monkeypatch.setenv(k, v)
        base = _default_runs(ctx, cases)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = _default_runs(ctx, cases)
        for k in list(env) + list(common):
            monkeypatch.delenv(k)
        b_lines, g_lines = sum((b["route"] for b in base), []), sum((g["route"] for g in got), [])
        assert_route_changed(name, b_lines, g_lines, removed, added)
        if split:
            # the default runs the forward launch's tiles whole; the switch splits its ragged tail along K
            fb, fg = [l for l in b_lines if l.startswith("fwd ")], [l for l in g_lines if l.startswith("fwd ")]
            assert not [l for l in fb if re.search(r"tail\d+x([2-9]|\d\d)", l)], (name, fb)
            assert [l for l in fg if re.search(r"tail\d+x([2-9]|\d\d)", l)], (name, fg)
        for case, b, g in zip(cases, base, got):
            check_route_case(case, b, g, name)


def _warp_oracle(B, H, seed):
    torch.manual_seed(seed)
    G, D = O.warp_module_params(), O.patchgan_params(22)
    batch = O.synth_warp_batch(B, H, H, seed=1234)
    st = O.WarpStepOracle(G, D)
    s64 = st.astype(torch.float64)
    torch.manual_seed(seed + 1)
    st.step(*batch)
    s64.step(*batch, labels=st.labels)
    return G, D, batch, st, s64


def _texture_oracle(B, H, seed):
    torch.manual_seed(seed)
    G, D = O.texture_module_params(img_size=H), O.patchgan_params(22)
    vgg = O.vgg16_feature_params()
    batch = O.synth_texture_batch(B, H, H, seed=4321)
    st = O.TextureStepOracle(G, D, vgg)
    s64 = st.astype(torch.float64)
    torch.manual_seed(seed + 1)
    st.step(*batch)
    s64.step(*batch, labels=st.labels)
    return G, D, vgg, batch, st, s64


WINO_PLANE_CASES = [
    pytest.param("sim", "warp", {"SWN_WINO_S2": "0"}, (), id="hostsim-warp-SWN_WINO_S2=0"),
    pytest.param("sim", "texture", {"SWN_WINO_S2": "2"}, (), id="hostsim-texture-SWN_WINO_S2=2"),
    pytest.param("gpu", "warp", {"SWN_WINO_S2": "0"}, (), id="mi355x-warp-SWN_WINO_S2=0", marks=pytest.mark.gpu),
    pytest.param("gpu", "texture", {"SWN_WINO_S2": "2"}, (), id="mi355x-texture-SWN_WINO_S2=2", marks=pytest.mark.gpu),
    pytest.param("gpu", "warp", {"SWN_AMAX_FUSED": "0"}, ("_ap[",), id="mi355x-warp-SWN_AMAX_FUSED=0", marks=pytest.mark.gpu),
    pytest.param("gpu", "warp", {"SWN_PAIR": "0"}, ("_ap[",), id="mi355x-warp-SWN_PAIR=0", marks=pytest.mark.gpu),
]


@pytest.mark.small_channel_winograd
@pytest.mark.parametrize("backend,kind,env,removed", WINO_PLANE_CASES)
def test_winograd_switches_against_the_pinned_float64_oracle(backend, kind, env, removed, tmp_path, monkeypatch):
    """Switches that change the Winograd forms of a model, one 64 x 64 training step on the small-channel Winograd routing:
      SWN_WINO_S2 (read when a layer is built): =0 runs the warp stage's k4 s2 convs / transposed convs direct instead of strided
      Winograd F(4x4,2x2), =2 puts the texture U-Net's strided layers on it too;
      SWN_AMAX_FUSED=0 (per launch, and per layer built: no pair-form planes are planned) and SWN_PAIR=0 (once per process: a child)
      store the Winograd planes in fp32 instead of the producer-cut pair form.
    Each step is held to the float64 oracle with the native pass's activation pattern replayed (tests/test_pattern_replay.py: every
    gradient within 1e-4; un-pinned, one LeakyReLU branch taken differently near zero moves a U-Net gradient by ~1e-2 between ANY
    two fp32 evaluations), and the launch list must differ from the same step without the switch."""
    from tests.test_pattern_replay import _texture_replay, _warp_replay
    ctx = backends.gpu_ctx() if backend == "gpu" else backends.hostsim_ctx()

    def run():
        with backends.traced_route(ctx) as r:
            if kind == "warp":
                res = _warp_replay(ctx, 2, 64, 0, True)
            else:
                res = _texture_replay(ctx, 2, 64, True)
        return res, r.lines

    (f0, d0, g0), base = run()
    if "SWN_PAIR" in env:
        got = run_child(tmp_path, "pair0", "replay", dict(kind=kind), dict(env, SWN_WINO_MINC="32"))
        (f1, d1, g1), lines = got["res"], got["route"]
    else:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        (f1, d1, g1), lines = run()
    name = " ".join("%s=%s" % kv for kv in env.items())
    assert_route_changed(name, base, lines, removed)
    print("%s %s: pinned gradient error D %.2e G %.2e (default route D %.2e G %.2e)" % (kind, name, d1, g1, d0, g0))


# ---- 3. the one-plane arithmetic, element by element --------------------------------------------------------------------
def one_plane_bound(absA, amaxA, topA, absB, amaxB, topB, f):
    """Per-element error bound of the one-plane form (oracle/split_model.py matmul_one_plane, derived there), twice the analytic one."""
    ones_a, ones_b = torch.ones_like(absA), torch.ones_like(absB)
    return 2.0 * (2.0 ** -10 * f(absA, absB) + amaxA * 2.0 ** -(24 + topA) * f(ones_a, absB) + amaxB * 2.0 ** -(24 + topB) * f(absA, ones_b))


@pytest.mark.gpu
def test_one_plane_form_element_bound_on_the_mi355x(tmp_path, monkeypatch):
    """`bench.py --precision f16`: every operand of a ring-kernel GEMM is ONE fp16 plane of x 2^k, rounded to nearest.  Per output
    element against float64 (oracle/split_model.py matmul_one_plane derives the constants):
        |err| <= 2 (2^-10 conv(|a|, |b|) + amax_a 2^-(24+top_a) conv(1, |b|) + amax_b 2^-(24+top_b) conv(|a|, 1))
    top = 12 for activations and gradients (PC_TOP_A), 10 for weights (PC_TOP_B).  Checked on the forward pass (outlier 2^18 x the
    bulk in the activations) and the input gradient (outlier in dY) -- SWN_PC_PLANES=1, read once per process: a child -- and on
    the weight gradient (outliers in both) -- SWN_WGRAD_PLANES=1, per launch: in-process.  One-signed operands (post-ReLU
    activations, a positive filter) must leave no mean relative bias beyond 2^-12: round-to-nearest is unbiased, a truncating cut
    would sit near -2^-10."""
    ctx = backends.gpu_ctx()
    g = torch.Generator().manual_seed(31)
    n, ci, h, co, k = 3, 64, 64, 128, 4
    x = torch.randn(n, ci, h, h, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
    big = float(2 ** 18)
    xo = x.clone(); xo[1, 7, 33, 21] = big
    y_shape = ref_conv64(K4S2, 0, x, w).shape
    dyo = torch.randn(y_shape, generator=g); dyo[2, 100, 5, 9] = -big
    xp = torch.relu(torch.randn(n, ci, h, h, generator=g)) + 0.01            # one-signed operands
    wp = torch.randn(co, ci, k, k, generator=g).abs() * (2.0 / (ci * k * k)) ** 0.5
    dyp = torch.rand(y_shape, generator=g) + 0.1
    c = dict(kind=K4S2, tr=0, b=None, y_shape=tuple(y_shape))
    cases = [dict(c, x=xo, w=w, dy=dyo, whats=(0, 2)), dict(c, x=xp, w=wp, dy=dyp, whats=(0, 2))]
    got = run_child(tmp_path, "pc_planes_1", "ops", dict(cases=cases), {"SWN_PC_PLANES": "1", "SWN_WINOGRAD": "0"})
    monkeypatch.setenv("SWN_WGRAD_PLANES", "1")
    monkeypatch.setenv("SWN_WINOGRAD", "0")
    wg = [conv_call(ctx, K4S2, 0, 1, xo, w, None, dy=dyo), conv_call(ctx, K4S2, 0, 1, xp, w, None, dy=dyp)]
    with backends.traced_route(ctx) as r:
        conv_call(ctx, K4S2, 0, 1, xo, w, None, dy=dyo)
    assert any("_h1[" in l for l in r.lines), r.lines                       # the one-plane weight-gradient kernel ran

    def fwd64(a, b):
        return F.conv2d(a.double(), b.double(), None, stride=2, padding=1)

    def dgrad64(a, b):
        return F.conv_transpose2d(a.double(), b.double(), None, stride=2, padding=1)

    def wgrad64(a, d):
        wz = torch.zeros(co, ci, k, k, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(F.conv2d(a.double(), wz, None, stride=2, padding=1), wz, d.double())[0]

    am = lambda t: float(t.abs().max())
    for tag, (X, Wt, DY), res, wgt in (("outlier", (xo, w, dyo), got[0], wg[0]), ("one-signed", (xp, wp, dyp), got[1], wg[1])):
        checks = (("fwd", res["y"], fwd64(X, Wt), one_plane_bound(X.abs(), am(X), 12, Wt.abs(), am(Wt), 10, fwd64)),
                  ("dgrad", res["dx"], dgrad64(DY, Wt), one_plane_bound(DY.abs(), am(DY), 12, Wt.abs(), am(Wt), 10, dgrad64)),
                  ("wgrad", wgt, wgrad64(X, DY), one_plane_bound(X.abs(), am(X), 12, DY.abs(), am(DY), 12, wgrad64)))
        for what, out, ref, tol in checks:
            err = out.double() - ref
            worst = float((err.abs() / tol).max())
            e = rel(out, ref)
            print("one plane %-10s %-5s: worst |err| / bound %.3f  rel-L2 %.2e" % (tag, what, worst, e))
            assert worst <= 1.0, (tag, what, worst)
            assert e > 1e-5, (tag, what, "two-plane accuracy: the one-plane form did not run", e)
            if tag == "one-signed":
                bias = float((err / ref).mean())
                print("one plane one-signed %-5s: mean relative bias %+.2e" % (what, bias))
                assert abs(bias) < 2.0 ** -12, (what, bias)


# ---- 4. scheduling switches: the same step, bit for bit ------------------------------------------------------------------
def _step_specs(H, warp_B, tex_B, seed=3):
    torch.manual_seed(seed)
    G, D = O.warp_module_params(), O.patchgan_params(22)
    warp = dict(kind="warp", B=warp_B, H=H, G=G, D=D, inputs=list(O.synth_warp_batch(warp_B, H, H, seed=11)), labels=[0.9, 0.8, 1.0])
    from tests.test_texture_step import vgg_state_dict
    TG, TD = O.texture_module_params(img_size=H), O.patchgan_params(22)
    vgg = O.vgg16_feature_params()
    tex = dict(kind="texture", B=tex_B, H=H, G=TG, D=TD, VGGraw=vgg, inputs=list(O.synth_texture_batch(tex_B, H, H, seed=12)),
               labels=[0.9, 0.8, 1.0])
    return dict(models=dict(warp=warp, texture=tex)), vgg_state_dict


def _finish_specs(spec, ctx, vgg_state_dict):
    t = spec["models"]["texture"]
    if "VGG" not in t:
        m = engine.NativeModel(ctx, "texture", t["B"], t["H"], t["H"])
        t["VGG"] = vgg_state_dict(m, t.pop("VGGraw"))
        m.close()
    return spec


def assert_same_step(a, b, what):
    for kind in a:
        x, y = a[kind], b[kind]
        assert x["losses"] == y["losses"], (what, kind, "losses", x["losses"], y["losses"])
        for k in ("output", "gD", "gG", "wD", "wG"):
            assert torch.equal(x[k], y[k]), (what, kind, k, float((x[k] - y[k]).abs().max()))
        assert float(x["gG"].abs().max()) > 0 and float(x["gD"].abs().max()) > 0


SCHEDULING_CHILDREN = [("no switch", {}),
                       ("scheduling switches", {"SWN_PREFETCH": "3", "SWN_PREFETCH_AHEAD": "1", "SWN_BIAS_MAIN": "0",
                                                "SWN_VT_EARLY": "0", "SWN_OVERLAP": "0"}),
                       ("SWN_PREFETCH=0", {"SWN_PREFETCH": "0"})]


@pytest.mark.gpu
def test_scheduling_switches_are_bit_identical_on_the_mi355x(tmp_path, monkeypatch):
    """Switches that move work to another place or time, not another arithmetic: one phased training step (forward in training
    mode, backward_D, AdamW(D), backward_G, AdamW(G)) of the warp stage at 256 x 256 bs 2 and of the texture stage at 256 x 256 bs 1,
    losses / both gradient arenas / both post-step weight arenas / the output equal (torch.equal) to the default step.
      in-process (read per launch): SWN_PHASE_ZFAST=0, SWN_IN_PAIR_XCD=0.
      (Not SWN_AMAX_FUSED=0: a producer's slot may hold a BOUND of its tensor's amax -- the conditioned PatchGAN input's slot is
      floored at 1, a Winograd plane's is the transform's gain times its input's -- and a launch that takes the amax itself can pick
      a scale one power of two apart: measured on the MI355X, the discriminator loss moved in its last bit.  It is a numerics
      switch, held to float64 by test_winograd_switches_against_the_pinned_float64_oracle.)
      child processes (read once per process or per context): a child with no switch -- a difference across processes fails
      as its own finding -- then SWN_PREFETCH=3 + SWN_PREFETCH_AHEAD=1 + SWN_BIAS_MAIN=0 + SWN_VT_EARLY=0 + SWN_OVERLAP=0 together,
      then SWN_PREFETCH=0."""
    ctx = backends.gpu_ctx()
    spec, vsd = _step_specs(256, 2, 1)
    spec = _finish_specs(spec, ctx, vsd)
    base = {}
    models = {name: engine.NativeModel(ctx, s["kind"], s["B"], s["H"], s["H"]) for name, s in spec["models"].items()}
    try:
        base = {name: phased_step(m, spec["models"][name]) for name, m in models.items()}
        for env in ({"SWN_PHASE_ZFAST": "0"}, {"SWN_IN_PAIR_XCD": "0"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = {name: phased_step(m, spec["models"][name]) for name, m in models.items()}
            for k in env:
                monkeypatch.delenv(k)
            assert_same_step(base, got, env)
            print("bit-identical in-process:", env)
    finally:
        for m in models.values():
            m.close()
    for what, env in SCHEDULING_CHILDREN:
        got = run_child(tmp_path, what.replace(" ", "_").replace("=", ""), "steps", spec, env)
        assert_same_step(base, got, "child process, " + what)
        print("bit-identical in a child process:", what, env)


@pytest.mark.small_channel_winograd
def test_model_level_switches_on_the_host_simulator(tmp_path, monkeypatch):
    """The engine-level switches on the host simulator (CPU): one phased step of both stages at 64 x 64 (small-channel Winograd
    routing, so that the Winograd forms exist at that size).  SWN_PREFETCH=0 / =3, SWN_PREFETCH_AHEAD=1, SWN_BIAS_MAIN=0 and
    SWN_VT_EARLY=0 are read once per process: child processes, against a child with no switch, bit for bit.  SWN_PRECUT=0 (read
    per call by the simulator, whose panels are the fp32 operand itself) must be bit-identical there too.  (SWN_WINO_S2 changes
    the arithmetic, not the order: test_winograd_switches_against_the_pinned_float64_oracle holds it to float64 here as well.)"""
    env_minc = {"SWN_WINO_MINC": "32"}
    spec, vsd = _step_specs(64, 1, 1)
    ctx = backends.hostsim_ctx()
    spec = _finish_specs(spec, ctx, vsd)
    ref = run_child(tmp_path, "sim_none", "steps", spec, env_minc, sim=True)
    for name, env in (("sim_sched", {"SWN_PREFETCH": "3", "SWN_PREFETCH_AHEAD": "1", "SWN_BIAS_MAIN": "0", "SWN_VT_EARLY": "0"}),
                      ("sim_prefetch0", {"SWN_PREFETCH": "0"})):
        got = run_child(tmp_path, name, "steps", spec, dict(env_minc, **env), sim=True)
        assert_same_step(ref, got, name)

    def in_process(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = {}
        for name, s in spec["models"].items():
            m = engine.NativeModel(ctx, s["kind"], s["B"], s["H"], s["H"])
            try:
                out[name] = phased_step(m, s)
            finally:
                m.close()
        for k in env:
            monkeypatch.delenv(k)
        return out

    here = in_process({})
    assert_same_step(ref, here, "host simulator, child against in-process")
    assert_same_step(here, in_process({"SWN_PRECUT": "0"}), "SWN_PRECUT=0")


# ---- 5. new targets between backward_D and backward_G -------------------------------------------------------------------
_CE_ORACLE = {}


def _ce_oracle(B, H):
    """The warp step with new targets handed over between backward_D and backward_G (float64 and fp32), and without (float64)."""
    if (B, H) not in _CE_ORACLE:
        torch.manual_seed(5)
        G, D = O.warp_module_params(), O.patchgan_params(22)
        bodys, inputs, targets = O.synth_warp_batch(B, H, H, seed=41)
        lab_new = torch.randint(1, 19, (B, H, H), generator=torch.Generator().manual_seed(42))
        new = O.labels_to_onehot(lab_new, 19).float()
        labels = [0.9, 0.8, 1.0]
        st, st32, st_old = (O.WarpStepOracle(G, D, dtype=dt) for dt in (torch.float64, torch.float32, torch.float64))
        st.step(bodys, inputs, targets, labels=labels, targets_G=new)
        st32.step(bodys, inputs, targets, labels=labels, targets_G=new)
        st_old.step(bodys, inputs, targets, labels=labels)
        _CE_ORACLE[(B, H)] = (G, D, (bodys, inputs, targets), lab_new, new, labels, st, st32, st_old)
    return _CE_ORACLE[(B, H)]


@pytest.mark.parametrize("backend", [pytest.param("sim", id="hostsim"), pytest.param("gpu", id="mi355x", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("early", ["1", "0"])
def test_new_targets_between_backward_d_and_backward_g(backend, early, monkeypatch):
    """A phased caller may hand new targets -- set_input(2, ..) or set_input_labels(2, ..) -- after backward_D.  The early
    cross-entropy term (SWN_CE_EARLY, default on, read when a model is built) is taken inside backward_D against the targets of
    that time; backward_G must take it again against the new ones (WarpModel resets ce_done_ in both setters).  G_ce, G and the
    generator's gradients are held to the oracle's step whose backward_G sees the new targets (backward_D the old ones)."""
    from tests.test_warp_step import noise_bias
    monkeypatch.setenv("SWN_CE_EARLY", early)
    ctx = backends.gpu_ctx() if backend == "gpu" else backends.hostsim_ctx()
    B, H = 1, 64
    G, D, batch, lab_new, new, labels, st, st32, st_old = _ce_oracle(B, H)
    last = "upsample_and_pad.2.weight"
    assert rel(st_old.grads_G[last], st.grads_G[last]) > 0.1          # (the new targets change the generator's gradient)
    m = engine.NativeModel(ctx, "warp", B, H, H)
    try:
        for form in ("tensor", "labels"):
            backends.reset_state(m, {engine.NET_G: G, engine.NET_D: D})
            for i, t in enumerate(batch):
                m.set_input(i, t)
            m.forward(False, 0)
            m.backward_D(labels[0], labels[1])
            m.optimizer_step(engine.NET_D)
            if form == "tensor":
                m.set_input(2, new)
            else:
                m.set_input_labels(2, lab_new.int())
            m.backward_G(labels[2])
            got = m.losses()
            gG = m.state_dict(engine.NET_G, which=engine.W_GRAD, to_cpu=True)
            for k in ("G_ce", "G"):
                assert abs(got[k] - st.losses[k]) <= 2e-5 * abs(st.losses[k]), (form, k, got[k], st.losses[k], "old targets", st_old.losses[k])
            backends.assert_grads_vs_fp64(gG, st32.grads_G, st.grads_G, noise_bias, "new targets (%s), SWN_CE_EARLY=%s" % (form, early))
    finally:
        m.close()
