"""Cost of handing one texture batch to the model, both ways, on the device (a record, not a gate).

  (a) float hand-over: input and target textures as normalised float32 NCHW tensors, the ROI table, and the cloths as an int32
      label map through set_input_labels -- the cheapest form the model took before the compact batch existed;
  (b) compact hand-over: uint8 HWC images, uint8 label maps, raw ROIs and five scalars per sample through
      set_input_texture_batch (one launch, csrc/texture_batch.hip).

Both from pinned host memory, each timed from the call to a synchronised device INCLUDING its host-to-device copies, interleaved
in one process (a, b, a, b, ...), median over the repetitions.  Only the hand-over is timed: what the host pays to BUILD the
float tensors (two normalisations, a flip, a resize of the one-hot map and a crop per sample) is not part of (a) here.

    python tools/texture_batch_time.py [--batch 16] [--size 256] [--reps 30] [--out profiles/texture_batch_handover.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swapnet_amd import engine  # noqa: E402
from swapnet_amd.datasets import gpu_texture_batch as TB  # noqa: E402

MEAN = (0.8319639705048438, 0.8105952930426163, 0.8038053056173073)
STD = (0.22878186598352074, 0.245635337367858, 0.2517315913036158)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256, help="crop size = load size (no crop, like the C3 configuration)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, S, R = a.batch, a.size, 12
    ctx = engine.Context(workspace_mb=1024)
    m = engine.NativeModel(ctx, "texture", B, S, S, is_train=True)
    g = np.random.RandomState(0)
    opt = argparse.Namespace(input_transforms=("hflip", "vflip"), load_size=S, crop_size=S, crop_bounds=None, texture_norm_stats=(MEAN, STD),
                             cloth_channels=19)
    tb = TB.GpuTextureBatch(opt, ctx=ctx)
    samples = [{"image_u8": g.randint(0, 256, (S, S, 3)).astype(np.uint8), "labels_u8": g.randint(0, 19, (S, S)).astype(np.uint8),
                "rois_raw": np.sort(g.randint(0, S, (R, 2, 2)), axis=1).reshape(R, 4).astype(np.float32), "original_size": (S, S),
                "paths": ("", "")} for _ in range(B)]
    compact = tb.collate(samples)
    ref = tb.expand(compact)
    pin = lambda t: t.cpu().contiguous().pin_memory()
    floats = [pin(ref["input_textures"]), pin(ref["rois"]), pin(compact["cloth_labels_u8"].to(torch.int32)),
              pin(ref["target_textures"])]
    compact = {k: (pin(v) if torch.is_tensor(v) else v) for k, v in compact.items()}

    def float_handover():
        m.set_input(0, floats[0]); m.set_input(1, floats[1]); m.set_input_labels(2, floats[2]); m.set_input(3, floats[3])

    def compact_handover():
        m.set_input_texture_batch(compact)

    def timed(fn):
        torch.cuda.synchronize(); ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        timed(float_handover); timed(compact_handover)
    ta, tbs = [], []
    for _ in range(a.reps):
        ta.append(timed(float_handover)); tbs.append(timed(compact_handover))
    # the compact hand-over left what the float one leaves
    compact_handover(); u1 = m.tap(engine.NET_G, "unet_in").clone()
    float_handover(); u2 = m.tap(engine.NET_G, "unet_in")
    same = bool(torch.equal(u1[:, 36:], u2[:, 36:]))
    bytes_a = sum(t.numel() * t.element_size() for t in floats)
    bytes_b = sum(v.numel() * v.element_size() for v in compact.values() if torch.is_tensor(v))
    lines = ["texture batch hand-over, %s, bs %d, %d x %d, load size %d, pinned host memory, interleaved, %d repetitions each"
             % (torch.cuda.get_device_name(0), B, S, S, S, a.reps),
             "(a) float tensors + set_input_labels : median %.3f ms  (min %.3f, max %.3f)   H2D %.2f MB, 6 launches"
             % (statistics.median(ta), min(ta), max(ta), bytes_a / 1e6),
             "(b) compact, set_input_texture_batch : median %.3f ms  (min %.3f, max %.3f)   H2D %.2f MB, 1 launch"
             % (statistics.median(tbs), min(tbs), max(tbs), bytes_b / 1e6),
             "cloth channels of the U-Net input equal after either hand-over: %s" % same]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
