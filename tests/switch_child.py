"""Child-process side of tests/test_route_switches.py.

Several SWN_* switches are read once per process (a `static const` in the library) or when a context is created, so the
parent test starts a fresh interpreter with the switch in its environment and runs this module:

    python -m tests.switch_child ops   IN.pt OUT.pt [sim]     operator-level convolutions (swn_op_conv) of the cases in IN.pt
    python -m tests.switch_child steps IN.pt OUT.pt [sim]     one phased training step of each model described in IN.pt
    python -m tests.switch_child replay IN.pt OUT.pt [sim]    one pinned-pattern step of IN.pt's kind against the float64 oracle

Everything the child computes from is read from IN.pt (inputs, weights), and everything it measured goes to OUT.pt; the parent
compares.  `sim` runs on the host simulator instead of the MI355X.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

from swapnet_amd import _C, engine  # noqa: E402


def context(sim):
    if sim:
        from tests import backends
        return engine.Context(lib=_C.Lib(backends.build_hostsim()), workspace_mb=256)
    return engine.Context(workspace_mb=1024)


def conv_call(ctx, kind, tr, what, x, w, b, y_shape=None, dy=None):
    """swn_op_conv, one direction: what 0 = forward (y), 1 = weight gradient (dW), 2 = input gradient (dX)."""
    dev = ctx.device
    xd = (x if what != 2 else torch.zeros_like(x)).to(dev).contiguous()
    wd = (w if what != 1 else torch.zeros_like(w)).to(dev).contiguous()
    bd = b.to(dev).contiguous() if (b is not None and what == 0) else None
    n, ci, h, ww = x.shape
    co = w.shape[1] if tr else w.shape[0]
    yd = torch.empty(y_shape, device=dev) if what == 0 else dy.to(dev).contiguous()
    ctx.lib.call("swn_op_conv", ctx.handle, kind, int(tr), what, 0, _C.ptr(xd), n, ci, h, ww, _C.ptr(wd), co, _C.ptr(bd), 0,
                 _C.ptr(yd))
    ctx.sync()
    return {0: yd, 1: wd, 2: xd}[what].cpu()


def run_conv_case(ctx, case, whats=(0, 2, 1)):
    """The three directions of one case, each under a route trace: {"y"/"dx"/"dw": tensor, "route": [launch lines]}."""
    from tests.backends import traced_route
    out = {"route": []}
    for what in whats:
        with traced_route(ctx) as r:
            t = conv_call(ctx, case["kind"], case["tr"], what, case["x"], case["w"], case.get("b"), case["y_shape"], case["dy"])
        out[{0: "y", 1: "dw", 2: "dx"}[what]] = t
        out["route"] += ["%s %s" % ({0: "fwd", 1: "wgrad", 2: "dgrad"}[what], l) for l in r.lines]
    return out


def build_model(ctx, spec):
    kind, B, H = spec["kind"], spec["B"], spec["H"]
    m = engine.NativeModel(ctx, kind, B, H, H, is_train=True)
    return m


def load_state(m, spec):
    nets = {engine.NET_G: spec["G"], engine.NET_D: spec["D"]}
    if spec["kind"] == "texture":
        nets[engine.NET_VGG] = spec["VGG"]
    for net, sd in nets.items():
        m.load_state_dict(net, sd)
        if net != engine.NET_VGG:
            m.arena(net, engine.W_EXP_AVG).zero_()
            m.arena(net, engine.W_EXP_AVG_SQ).zero_()
            m.ctx.sync()
            m.optim_step_count(net, 0)
    m.set_hyper()
    for i, t in enumerate(spec["inputs"]):
        m.set_input(i, t)


def phased_step(m, spec):
    """forward (training mode, fixed dropout seed) -> backward_D -> AdamW(D) -> backward_G -> AdamW(G), each result copied out."""
    from tests.backends import traced_route
    lab = spec["labels"]
    load_state(m, spec)
    with traced_route(m.ctx) as r:
        m.forward(True, 5)
        out = m.output().cpu()
        m.backward_D(lab[0], lab[1])
        gD = m.grad_arena(engine.NET_D).clone()
        m.optimizer_step(engine.NET_D)
        m.backward_G(lab[2])
        gG = m.grad_arena(engine.NET_G).clone()
        m.optimizer_step(engine.NET_G)
        m.ctx.sync()
    return dict(losses=m.losses(), output=out, gD=gD.cpu(), gG=gG.cpu(), wD=m.weight_arena(engine.NET_D).clone().cpu(),
                wG=m.weight_arena(engine.NET_G).clone().cpu(), route=r.lines)


def main(argv):
    job, src, dst = argv[:3]
    sim = len(argv) > 3 and argv[3] == "sim"
    spec = torch.load(src, weights_only=False)
    ctx = context(sim)
    if job == "ops":
        res = [run_conv_case(ctx, c, c.get("whats", (0, 2, 1))) for c in spec["cases"]]
    elif job == "steps":
        res = {}
        for name, s in spec["models"].items():
            m = build_model(ctx, s)
            try:
                res[name] = phased_step(m, s)
            finally:
                m.close()
    elif job == "replay":          # one pinned-pattern 64 x 64 training step against the float64 oracle (tests/test_pattern_replay.py)
        from tests.backends import traced_route
        from tests.test_pattern_replay import _texture_replay, _warp_replay
        with traced_route(ctx) as r:
            out = _warp_replay(ctx, 2, 64, 0, True) if spec["kind"] == "warp" else _texture_replay(ctx, 2, 64, True)
        res = dict(res=out, route=r.lines)
    else:
        raise SystemExit("unknown job " + job)
    torch.save(res, dst)
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
