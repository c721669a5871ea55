"""optimizers of the reference (optimizers/__init__.py): option modifiers and `define_optimizer`,
returning an object with the torch.optim.Optimizer surface the reference uses (zero_grad / step /
state_dict / load_state_dict / param_groups) backed by a fused HIP update over the network's flat
arena: AdamW (default) or AdaBound, chosen per network by --optimizer_G / --optimizer_D.  AdaBound
restates the published update (Luo et al., ICLR 2019) as adabound 0.0.5 executes it; the package
itself is not a dependency and is never imported."""
from argparse import ArgumentParser
from collections import OrderedDict

from .. import engine


def get_options_modifier(optimizer_name):
    optimizer_name = optimizer_name.lower()
    if "adam" in optimizer_name:
        return adam_modifier
    if "adabound" in optimizer_name:
        return adabound_modifier
    raise NotImplementedError


def adam_modifier(parser: ArgumentParser, *_):
    parser.add_argument("--b1", type=float, default=0.9, help="Adam b1")
    parser.add_argument("--b2", type=float, default=0.999, help="Adam b2")
    return parser


def adabound_modifier(parser: ArgumentParser, *_):
    parser = adam_modifier(parser)
    parser.add_argument("--final_lr", type=float, default=0.1, help="AdaBound final_lr")
    return parser


class NativeAdamW:
    """torch.optim.AdamW(lr, betas, eps=1e-8, weight_decay, amsgrad=False) over one arena."""

    def __init__(self, backend, net, lr, weight_decay, betas):
        self.backend, self.net = backend, net
        self.param_groups = [dict(lr=lr, weight_decay=weight_decay, betas=tuple(betas), eps=1e-8, amsgrad=False)]
        self._pushed = None
        self.sync()

    def sync(self):
        """param_groups is live like torch's: a scheduler (or the user) editing param_groups[0]["lr"] /
        ["weight_decay"] / ["betas"] takes effect at the next step.  Each optimizer owns its own hyper-parameters
        (G: lr, weight_decay, b1, b2; D: d_lr, d_weight_decay, d_b1, d_b2), so loading optimizer_D's state never
        touches G's betas."""
        g = self.param_groups[0]
        cur = (float(g["lr"]), float(g["weight_decay"]), float(g["betas"][0]), float(g["betas"][1]))
        if cur != self._pushed:
            key = "d_" if self.net == engine.NET_D else ""
            self.backend.set_hyper(**{key + "lr": cur[0], key + "weight_decay": cur[1], key + "b1": cur[2], key + "b2": cur[3]})
            self._pushed = cur

    def zero_grad(self, set_to_none=False):
        # every backward pass overwrites the whole gradient arena (each parameter has exactly one
        # producer and the planner's first write is a plain store), so there is nothing to clear
        pass

    def step(self, closure=None):
        self.sync()
        self.backend.cur.optimizer_step(self.net)

    def state_dict(self):
        """torch.optim.AdamW.state_dict() layout: state[i] = {step, exp_avg, exp_avg_sq}."""
        m = self.backend.any_model()
        names = list(m.param_infos(self.net).keys())
        avg = m.state_dict(self.net, which=engine.W_EXP_AVG, to_cpu=True)
        sq = m.state_dict(self.net, which=engine.W_EXP_AVG_SQ, to_cpu=True)
        step = m.optim_step_count(self.net)
        import torch
        state = OrderedDict()
        if step > 0:
            for i, n in enumerate(names):
                state[i] = dict(step=torch.tensor(float(step)), exp_avg=avg[n], exp_avg_sq=sq[n])
        groups = [dict(self.param_groups[0], params=list(range(len(names))))]
        return dict(state=state, param_groups=groups)

    def load_state_dict(self, sd):
        m = self.backend.any_model()
        names = list(m.param_infos(self.net).keys())
        state = sd["state"]
        if state:
            avg = {n: state[i]["exp_avg"] for i, n in enumerate(names)}
            sq = {n: state[i]["exp_avg_sq"] for i, n in enumerate(names)}
            m.load_state_dict(self.net, avg, which=engine.W_EXP_AVG)
            m.load_state_dict(self.net, sq, which=engine.W_EXP_AVG_SQ)
            m.optim_step_count(self.net, int(float(state[0]["step"])))
        g = sd["param_groups"][0]
        self.param_groups[0].update(lr=g["lr"], weight_decay=g["weight_decay"], betas=tuple(g["betas"]))
        self.sync()


class NativeAdaBound(NativeAdamW):
    """adabound.AdaBound(lr, betas, final_lr, gamma=1e-3, eps=1e-8, weight_decay, amsbound=False) over one arena:
    weight_decay is the coupled L2 term, and the bounds close in on final_lr * lr / base_lr, base_lr being the lr of
    construction (the package's `base_lrs`, which is not part of its state dict either)."""

    def __init__(self, backend, net, lr, weight_decay, betas, final_lr, gamma=1e-3):
        if not backend.ctx.lib.is_device:
            raise NotImplementedError("AdaBound is a HIP kernel only: the host simulator library has no AdaBound update")
        self.backend, self.net = backend, net
        self.base_lr = float(lr)
        self.param_groups = [dict(lr=lr, betas=tuple(betas), final_lr=final_lr, gamma=gamma, eps=1e-8,
                                  weight_decay=weight_decay, amsbound=False)]
        self._pushed = self._pushed_bound = None
        self.sync()

    def sync(self):
        """As NativeAdamW.sync, plus final_lr / gamma: edits take effect at the next step."""
        super().sync()
        g = self.param_groups[0]
        if g.get("amsbound"):
            raise NotImplementedError("AdaBound with amsbound=True is not implemented natively")
        cur = (float(g["final_lr"]), float(g["gamma"]))
        if cur != self._pushed_bound:
            self.backend.set_optimizer(self.net, kind=engine.OPT_ADABOUND, final_lr=cur[0], base_lr=self.base_lr, gamma=cur[1])
            self._pushed_bound = cur

    def state_dict(self):
        """adabound.AdaBound.state_dict() layout: state[i] = {step (int), exp_avg, exp_avg_sq}."""
        sd = super().state_dict()
        for st in sd["state"].values():
            st["step"] = int(st["step"])
        return sd

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        if "final_lr" not in g:
            raise ValueError("not an AdaBound state dict: its param_groups carry no final_lr")
        if g.get("amsbound", False):
            raise NotImplementedError("AdaBound with amsbound=True is not implemented natively")
        self.param_groups[0].update(final_lr=g["final_lr"], gamma=g.get("gamma", 1e-3))
        super().load_state_dict(sd)


def define_optimizer(parameters, opt, net: str):
    """optimizers.define_optimizer (:37-60).  `parameters` is the NativeNet (or its
    .parameters() generator is ignored): the optimizer binds to the net's backend."""
    if net != "D" and net != "G":
        raise ValueError(f"net arg must be 'D' or 'G', received {net}")
    choice = getattr(opt, "optimizer_" + net)
    if choice not in ("AdamW", "AdaBound"):
        raise NotImplementedError("optimizer %s is not implemented natively (AdamW | AdaBound)" % choice)
    lr = opt.d_lr if net == "D" else opt.lr
    wd = opt.d_weight_decay if net == "D" else opt.weight_decay
    backend = getattr(parameters, "_backend", None)
    if backend is None:
        raise ValueError("define_optimizer expects the swapnet_amd network object (not .parameters())")
    which = engine.NET_D if net == "D" else engine.NET_G
    if choice == "AdaBound":
        return NativeAdaBound(backend, which, lr, wd, (opt.b1, opt.b2), opt.final_lr)
    return NativeAdamW(backend, which, lr, wd, (opt.b1, opt.b2))
