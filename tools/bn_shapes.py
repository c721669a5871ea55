"""BatchNorm + LeakyReLU against InstanceNorm + LeakyReLU at the three norm sites of C2's discriminator (batch 2 x 32 = 64 images:
model.2's output 64 x 64^2 x 128, model.5's 64 x 32^2 x 256, model.8's 64 x 31^2 x 512), forward and backward, groups = 2.

Both layers are timed in this process on the same tensors through swn_op_norm_act_time: HIP events around each of `--iters`
back-to-back runs of the pass alone, after `--warmup` untimed ones; the median is reported with the bytes the pass has to move
(computed here from the shapes and the kernels' pass structure) and the rate that gives.

    python tools/bn_shapes.py [--out profiles/batch_norm_shapes.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("model.2", 64, 128, 64, 64), ("model.5", 64, 256, 32, 32), ("model.8", 64, 512, 31, 31)]      # name, N, C, H, W
LRELU = 1


def pass_bytes(kind, what, n, c, h, w):
    """fp32 bytes over HBM by pass structure.  BatchNorm: statistics pass (x; backward x, dy) + apply pass (x -> y; backward
    x, dy -> dx).  InstanceNorm: the same above 1024 pixels per image, ONE pass with the image's slab in registers up to 1024
    (C % 32 == 0).  Statistics, partial sums and coefficients are O(N C) and left out."""
    e = 4 * n * c * h * w
    one_pass = kind == "instance" and h * w <= 1024 and c % 32 == 0
    if what == "fwd":
        return e * (2 if one_pass else 3)
    return e * (3 if one_pass else 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    import torch
    from swapnet_amd import _C, engine
    ctx = engine.Context(workspace_mb=512)
    lines = ["# %s" % torch.cuda.get_device_name(0),
             "# median of %d HIP-event timings after %d warm-up runs; groups = 2; act = LeakyReLU(0.2); fp32 NHWC" % (args.iters, args.warmup),
             "%-8s %-18s %-4s %-9s %10s %10s %9s %9s" % ("site", "N x HxW x C", "pass", "norm", "MB moved", "median us", "GB/s", "vs IN")]
    g = torch.Generator().manual_seed(0)
    for name, n, c, h, w in SHAPES:
        x = (torch.randn(n, c, h, w, generator=g) * 2 + 0.5).to(ctx.device)
        dy = torch.randn(n, c, h, w, generator=g).to(ctx.device)
        for wi, what in enumerate(("fwd", "bwd")):
            med = {}
            for ki, kind in enumerate(("instance", "batch")):
                ms = (C.c_float * args.iters)()
                ctx.lib.call("swn_op_norm_act_time", ctx.handle, ki, wi, _C.ptr(x), _C.ptr(dy), n, c, h, w, 2, LRELU, args.warmup,
                             args.iters, ms)
                med[kind] = statistics.median(ms) * 1e-3
            for kind in ("instance", "batch"):
                b = pass_bytes(kind, what, n, c, h, w)
                lines.append("%-8s %-18s %-4s %-9s %10.1f %10.1f %9.0f %9.2f" % (
                    name, "%d x %dx%d x %d" % (n, h, w, c), what, kind, b / 1e6, med[kind] * 1e6, b / med[kind] / 1e9,
                    med[kind] / med["instance"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
