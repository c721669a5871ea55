"""Cost of handing one warp batch to the model, three ways, on the device (a record, not a gate).

  (a) float hand-over: bodys, input_cloths and target_cloths as float32 NCHW tensors through set_input -- the reference's form;
  (b) label hand-over: bodys as a float32 tensor, both cloth maps as int32 label maps through set_input_labels -- the cheapest form
      the model took before the compact batch existed; it cannot carry the per-channel augmentation;
  (c) compact hand-over: uint8 HWC body images, uint8 label maps and the map table through set_input_warp_batch (one launch,
      csrc/warp_batch.hip), without augmentation (c), with a 4-map chain per channel (c'), and with the same chains whose perspective
      rows are kind 3, Pillow's BICUBIC (c'': set_input_warp_batch_ex, the kernel's other instantiation).

All from pinned host memory, each timed from the call to a synchronised device INCLUDING its host-to-device copies, interleaved in
one process (a, b, c, c', c'', a, ...), median over the repetitions.  Only the hand-over is timed: what the host pays to BUILD the float
tensors (two one-hot expansions, 19 x 4 PIL resamplings, three resizes and a crop per sample) is not part of (a) here.  --pillow adds
that cost's largest part as a CPU figure: the chains of (c'') through Pillow, one PIL call per row and channel, single process.

    python tools/warp_batch_time.py [--batch 32] [--size 256] [--reps 30] [--pillow] [--out profiles/warp_batch_handover.txt]
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swapnet_amd import engine  # noqa: E402
from swapnet_amd.datasets import gpu_augment as GA  # noqa: E402
from swapnet_amd.datasets import gpu_warp_batch as WB  # noqa: E402

MEAN = (0.7361263252139642, 0.6969182556788952, 0.6853540012984733)
STD = (0.3225722505292399, 0.3375028333422175, 0.3416956811706011)


def pillow_chains(labels, maps):
    """What a reference loader pays for the chains of (c''): per (sample, channel) the float32 one-hot channel through one PIL call per
    row -- AFFINE NEAREST for kind 1 (the flips too: their rows are affine ones here, where torchvision transposes), PERSPECTIVE BICUBIC
    for kind 3 -- in this process, on one CPU core.  One pass over the batch."""
    from PIL import Image
    B, C = maps.shape[:2]
    t0 = time.perf_counter()
    calls = 0
    for b in range(B):
        for c in range(C):
            img = Image.fromarray((labels[b] == c).astype(np.float32) if c else np.zeros(labels[b].shape, np.float32))
            for row in maps[b, c]:
                if row[0] == GA.KIND_AFFINE:
                    f = row[1:7] / 65536.0                # out of Pillow's 16.16 fixed point, the half-pixel terms taken out again
                    co = (f[0], f[1], f[2] - 0.5 * f[0] - 0.5 * f[1], f[3], f[4], f[5] - 0.5 * f[3] - 0.5 * f[4])
                    img = img.transform(img.size, Image.AFFINE, co, Image.NEAREST); calls += 1
                elif row[0] == GA.KIND_PERSPECTIVE_BICUBIC:
                    img = img.transform(img.size, Image.PERSPECTIVE, tuple(row[1:9]), Image.BICUBIC); calls += 1
            np.array(img)
    ms = (time.perf_counter() - t0) * 1e3
    return "(host, CPU figure) the chains of (c'') through Pillow, %d PIL calls, one process, one pass: %.1f ms" % (calls, ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256, help="crop size = load size = size of the stored label maps and body images")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pillow", action="store_true", help="also time the bicubic chains through Pillow on this host's CPU")
    a = ap.parse_args()
    B, S = a.batch, a.size
    ctx = engine.Context(workspace_mb=1024)
    m = engine.NativeModel(ctx, "warp", B, S, S, is_train=True)
    g = np.random.RandomState(0)
    opt = argparse.Namespace(input_transforms="all", load_size=S, crop_size=S, crop_bounds=None, body_norm_stats=(MEAN, STD), cloth_channels=19,
                             is_train=True)
    wb = WB.GpuWarpBatch(opt, ctx=ctx, rng=random.Random(0))
    blocky = lambda: g.randint(0, 19, (S // 8, S // 8)).repeat(8, 0).repeat(8, 1).astype(np.uint8)
    samples = [{"body_u8": g.randint(0, 256, (S, S, 3)).astype(np.uint8), "target_labels_u8": blocky(), "paths": ("", "")} for _ in range(B)]
    chained = wb.collate(samples)                                   # a 4-map chain per (sample, channel)
    plain = dict(chained, maps=None)
    ref = wb.expand(plain)
    pin = lambda t: t.cpu().contiguous().pin_memory()
    floats = [pin(ref["bodys"]), pin(ref["input_cloths"]), pin(ref["target_cloths"])]
    labels = pin(plain["target_labels_u8"].to(torch.int32))
    pinned = lambda d: {k: (pin(v) if torch.is_tensor(v) else v) for k, v in d.items()}
    plain = pinned(plain)
    plain["input_labels_u8"] = plain["target_labels_u8"]            # image mode: one tensor, uploaded once
    chained = dict(plain, maps=pin(chained["maps"]))
    cubic_maps = chained["maps"].clone()                            # the same draws, the perspective rows resampled BICUBIC
    cubic_maps[..., 0][cubic_maps[..., 0] == GA.KIND_PERSPECTIVE] = GA.KIND_PERSPECTIVE_BICUBIC
    cubic = dict(plain, maps=pin(cubic_maps), perspective_resample="bicubic")

    def float_handover():
        m.set_input(0, floats[0]); m.set_input(1, floats[1]); m.set_input(2, floats[2])

    def label_handover():
        m.set_input(0, floats[0]); m.set_input_labels(1, labels); m.set_input_labels(2, labels)

    def timed(fn):
        torch.cuda.synchronize(); ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ways = [float_handover, label_handover, lambda: m.set_input_warp_batch(plain), lambda: m.set_input_warp_batch(chained),
            lambda: m.set_input_warp_batch(cubic)]
    for _ in range(a.warmup):
        for fn in ways:
            timed(fn)
    times = [[] for _ in ways]
    for _ in range(a.reps):
        for t, fn in zip(times, ways):
            t.append(timed(fn))
    # the compact hand-over left what the float one leaves
    taps = lambda: [m.tap(engine.NET_G, k).clone() for k in ("body", "cloth", "Dx", "slot_body", "slot_cloth", "slot_dx")]
    ways[2](); t1 = taps()
    ways[0](); t2 = taps()
    same = all(torch.equal(x[-B:] if x.shape[0] == 2 * B else x, y[-B:] if y.shape[0] == 2 * B else y) for x, y in zip(t1, t2))
    nbytes = lambda ts: sum(t.numel() * t.element_size() for t in ts)
    moved = [nbytes(floats), nbytes([floats[0], labels, labels]), nbytes([plain["bodys_u8"], plain["target_labels_u8"]]),
             nbytes([chained["bodys_u8"], chained["target_labels_u8"], chained["maps"]]),
             nbytes([cubic["bodys_u8"], cubic["target_labels_u8"], cubic["maps"]])]
    names = ["(a) three float tensors, set_input          ", "(b) float bodys + int32 labels, no augment. ",
             "(c) compact, set_input_warp_batch, no maps  ", "(c') compact, a 4-map chain per channel     ",
             "(c'') the same chains, perspective BICUBIC  "]
    launches = ["9 launches (5 layout, 4 amax)", "9 launches (3 layout, 2 one-hot, 4 amax)", "4 launches (1 + 3 amax)", "4 launches (1 + 3 amax)",
                "4 launches (1 + 3 amax)"]
    lines = ["warp batch hand-over, %s, bs %d, %d x %d, label and body sources %d x %d, load size %d, pinned host memory, interleaved, "
             "%d repetitions each" % (torch.cuda.get_device_name(0), B, S, S, S, S, S, a.reps)]
    for name, t, mb, l in zip(names, times, moved, launches):
        lines.append("%s: median %.3f ms  (min %.3f, max %.3f)   H2D %.2f MB, %s" % (name, statistics.median(t), min(t), max(t), mb / 1e6, l))
    lines.append("input buffers and amax slots equal after (a) and (c): %s" % same)
    n3 = int((cubic_maps[..., 0] == GA.KIND_PERSPECTIVE_BICUBIC).sum())
    ways[4](); ctx.sync()
    cloth = m.tap(engine.NET_G, "cloth")
    lines.append("(c''): %d of %d chains hold a kind-3 row; input cloth after it in [%.3f, %.3f]" % (n3, B * 19, float(cloth.min()), float(cloth.max())))
    if a.pillow:
        lines.append(pillow_chains(plain["target_labels_u8"].numpy(), cubic_maps.numpy()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
