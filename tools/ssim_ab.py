"""SSIM forward + backward on the device: the fused kernels (csrc/ssim.hip) against the torch composition of the same formula (the
module's CPU-branch code, SSIM._torch_forward, run on the same device with torch's autograd), B 16, C 3, 256 x 256, window 11, reduction
'mean'.  HIP events around each call, warm, the two paths alternating call by call, median of --iters.

  native, ops     engine.op_ssim twice (value; value + both gradients), what _SsimFn enqueues, no host read in between
  native, module  SSIM(11, 'mean')(a, b) then loss.backward(): the same plus autograd and the host read of the upstream scalar
  torch           the composition: five depthwise 11 x 11 convolutions and the element-wise passes, autograd's backward

It also holds both paths to the float64 composition on the same device at the timed size (rel-L2 of the loss and of both gradients),
and prints the HBM bytes the fused path moves per call, computed from the shape (not measured).

`python tools/ssim_ab.py [--out FILE]` on the MI355X; the lines it prints are the record (profiles/ssim.txt)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swapnet_amd import engine                  # noqa: E402
from swapnet_amd.modules.losses import SSIM     # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=4, default=[16, 3, 256, 256])
    ap.add_argument("--window", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_ab: no GPU visible; this tool measures on the device only")
    ctx = engine.default_context()
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(args.shape, generator=g) * 2 - 1)
    y = (x + 0.25 * torch.randn(args.shape, generator=g)).cuda()
    x = x.cuda()
    n = x.numel()
    crit = SSIM(args.window, "mean")
    res = {}

    def native_ops():
        engine.op_ssim(ctx, x, y, args.window, 1.0)
        res["ops"] = engine.op_ssim(ctx, x, y, args.window, 1.0, grad=1.0 / n, want_grad=(True, True))

    def native_module():
        a, b = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
        loss = crit(a, b)
        loss.backward()
        res["module"] = (loss.detach(), a.grad, b.grad)

    def torch_path():
        a, b = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
        loss = crit._torch_forward(a, b)
        loss.backward()
        res["torch"] = (loss.detach(), a.grad, b.grad)

    def native_fwd():
        engine.op_ssim(ctx, x, y, args.window, 1.0)

    def torch_fwd():
        with torch.no_grad():
            crit._torch_forward(x, y)

    paths = [("native, ops", native_ops), ("native, module", native_module), ("torch", torch_path), ("native forward only", native_fwd),
             ("torch forward only", torch_fwd)]
    for _ in range(args.warmup):
        for _, fn in paths:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in paths}
    for _ in range(args.iters):
        for name, fn in paths:
            times[name].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    total, _, d1, d2 = res["ops"]
    ml, m1, m2 = res["module"]
    # Both paths against the float64 composition on the same device.  The gradient is discontinuous where 1 - S crosses 0 or 1, and a
    # float32 evaluation may take the other branch there (among 3 M random elements a few have |S| below float32's resolution, and one
    # such element moves a whole gradient by 1e-4 .. 1e-3): the comparison runs under an upstream map that is 1 / n everywhere except
    # on the elements whose float64 index lies within 1e-4 of a clamp point, where it is 0 for every path alike.
    c = x.shape[1]
    k64 = crit.window.to(x.device).double().repeat(c, 1, 1, 1)
    a64, b64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    mu1, mu2 = crit.filter2D(a64, k64, c), crit.filter2D(b64, k64, c)
    s1, s2 = crit.filter2D(a64 * a64, k64, c) - mu1 * mu1, crit.filter2D(b64 * b64, k64, c) - mu2 * mu2
    s12 = crit.filter2D(a64 * b64, k64, c) - mu1 * mu2
    S = ((2 * mu1 * mu2 + crit.C1) * (2 * s12 + crit.C2)) / ((mu1 * mu1 + mu2 * mu2 + crit.C1) * (s1 + s2 + crit.C2))
    near = ((S.detach().abs() < 1e-4) | ((1 - S.detach()).abs() < 1e-4))
    gm = (~near).double() / n
    l64 = torch.clamp(1 - S, 0, 1) / 2
    (l64 * gm).sum().backward()
    l64, r1, r2 = l64.detach(), a64.grad, b64.grad
    a32, b32 = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
    t32 = SSIM(args.window, "none")._torch_forward(a32, b32)
    (t32 * gm.float()).sum().backward()
    tl, t1, t2 = t32.detach(), a32.grad, b32.grad
    _, nl, d1g, d2g = engine.op_ssim(ctx, x, y, args.window, 1.0, want_map=True, grad=gm.float(), want_grad=(True, True))
    torch.cuda.synchronize()
    lines = ["ssim_ab: %s (%s), %s, torch %s, shape %s, window %d, reduction mean, HIP events, median of %d after %d warm-up rounds, paths alternating"
             % (torch.cuda.get_device_name(ctx.device), getattr(torch.cuda.get_device_properties(ctx.device), "gcnArchName", "?"),
                time.strftime("%Y-%m-%d"), torch.__version__, tuple(args.shape), args.window, args.iters, args.warmup)]
    for name, _ in paths:
        v = sorted(times[name])
        lines.append("%-22s %8.3f ms   (min %.3f, max %.3f)" % (name, med[name], v[0], v[-1]))
    lines += ["forward + backward:  torch / native ops = %.2f,  torch / native module = %.2f;  forward only: torch / native = %.2f"
              % (med["torch"] / med["native, ops"], med["torch"] / med["native, module"], med["torch forward only"] / med["native forward only"]),
              "results at this size, rel-L2 against the float64 composition on the same device (loss map; gradients with %d of %d elements "
              "within 1e-4 of a clamp point masked out of the upstream gradient):  native  loss %.2e  d img1 %.2e  d img2 %.2e;  "
              "torch float32  loss %.2e  d img1 %.2e  d img2 %.2e;  module path equals the ops: %s"
              % (int(near.sum()), n, rel(nl, l64), rel(d1g, r1), rel(d2g, r2), rel(tl, l64), rel(t1, r1), rel(t2, r2),
                 bool(torch.equal(d1, m1) and torch.equal(d2, m2) and torch.equal(total[0] / n, ml))),
              "HBM bytes of the fused path, from the shape (not measured): value 8 B/element = %.1f MB; value + gradients 8 + (8 + 16) + (16 + 8 + 8) "
              "= 64 B/element = %.1f MB per forward + backward (halo re-reads come from cache); %.0f GB/s at the native-ops time"
              % (8 * n / 1e6, 64 * n / 1e6, 64 * n / 1e9 / (med["native, ops"] * 1e-3))]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
