"""Cost of handing one texture batch to the model from DECODED images, resize on the host against resize on the device (a record, not
a gate).

  (a) Pillow's `resize` of every image of the batch on the host (one thread, Image.BILINEAR, to torchvision's size for the load
      size), then the compact hand-over: set_input_texture_batch (one launch, csrc/texture_batch.hip).  The two parts are timed
      separately: the resize is host time that dataloader workers spend per sample, the hand-over is on the training process.
  (b) sources hand-over: the decoded images packed back to back through set_input_texture_sources (two launches:
      csrc/image_resize.hip, then csrc/texture_batch.hip).

Both hand-overs from pinned host memory, each timed from the call to a synchronised device INCLUDING its host-to-device copies,
interleaved in one process (a, b, a, b, ...), median over the repetitions.  The Pillow decode, which both forms need, is not timed.

    python tools/texture_sources_time.py [--batch 16] [--size 256] [--reps 30] [--out profiles/texture_sources_handover.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swapnet_amd import engine  # noqa: E402
from swapnet_amd.datasets import gpu_texture_batch as TB  # noqa: E402

MEAN = (0.8319639705048438, 0.8105952930426163, 0.8038053056173073)
STD = (0.22878186598352074, 0.245635337367858, 0.2517315913036158)


def measure(ctx, B, S, source_hw, reps, warmup):
    """One source size: the report lines."""
    h0, w0 = source_hw
    ws, hs = TB.tv_resize_size(w0, h0, S)
    R = 12
    m = engine.NativeModel(ctx, "texture", B, S, S, is_train=True)
    g = np.random.RandomState(h0)
    # the centred S x S window of the resized image, as --crop_bounds would name it (none when the resized image is S x S)
    x_min, y_min = (ws - S) // 2, (hs - S) // 2
    bounds = None if (ws, hs) == (S, S) else ((x_min, y_min), (x_min + S, y_min + S))
    opt = argparse.Namespace(input_transforms=("hflip", "vflip"), load_size=S, crop_size=S, crop_bounds=bounds, texture_norm_stats=(MEAN, STD),
                             cloth_channels=19)
    tb = TB.GpuTextureBatch(opt, ctx=ctx)
    common = [{"labels_u8": g.randint(0, 19, (S, S)).astype(np.uint8),
               "rois_raw": np.sort(g.randint(0, S, (R, 2, 2)), axis=1).reshape(R, 4).astype(np.float32), "paths": ("", "")} for _ in range(B)]
    images = [g.randint(0, 256, (h0, w0, 3)).astype(np.uint8) for _ in range(B)]
    pils = [Image.fromarray(x) for x in images]

    def host_resize():
        return [np.asarray(p.resize((ws, hs), Image.BILINEAR)) for p in pils]

    flips = tb.draw(B)
    sources = tb.collate([dict(c, source_u8=x) for c, x in zip(common, images)], flips=flips)
    compact = tb.collate([dict(c, image_u8=x, original_size=(w0, h0)) for c, x in zip(common, host_resize())], flips=flips)
    pin = lambda t: t.cpu().contiguous().pin_memory()
    sources = {k: (pin(v) if torch.is_tensor(v) and k != "source_geom" else v) for k, v in sources.items()}
    compact = {k: (pin(v) if torch.is_tensor(v) else v) for k, v in compact.items()}

    def timed(fn):
        torch.cuda.synchronize(); ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def host_timed():
        t0 = time.perf_counter()
        host_resize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(warmup):
        timed(lambda: m.set_input_texture_batch(compact)); timed(lambda: m.set_input_texture_sources(sources)); host_timed()
    tr, ta, tbs = [], [], []
    for _ in range(reps):
        tr.append(host_timed())
        ta.append(timed(lambda: m.set_input_texture_batch(compact)))
        tbs.append(timed(lambda: m.set_input_texture_sources(sources)))
    # the device's resize gives Pillow's bytes, and the sources hand-over leaves the cloth channels the compact one leaves
    resized = engine.op_resize_u8_packed(ctx, sources["sources_u8"], sources["source_geom"], hs, ws)
    m.set_input_texture_sources(sources); u1 = m.tap(engine.NET_G, "unet_in").clone()
    m.set_input_texture_batch(compact); u2 = m.tap(engine.NET_G, "unet_in")
    same = bool(torch.equal(resized.cpu(), compact["textures_u8"]) and torch.equal(u1[:, 36:], u2[:, 36:]))
    nbytes = lambda d: sum(v.numel() * v.element_size() for k, v in d.items() if torch.is_tensor(v) and k != "source_geom")
    med = statistics.median
    lines = ["sources %d x %d -> resized %d x %d (H x W), window %d x %d at (%d, %d)" % (h0, w0, hs, ws, S, S, x_min, y_min),
             "  (a) Pillow resize on the host, one thread : median %.3f ms per batch (min %.3f, max %.3f), %.3f ms per image"
             % (med(tr), min(tr), max(tr), med(tr) / B),
             "      + compact, set_input_texture_batch    : median %.3f ms  (min %.3f, max %.3f)   H2D %.2f MB, 1 launch"
             % (med(ta), min(ta), max(ta), nbytes(compact) / 1e6),
             "      = %.3f ms host + device" % (med(tr) + med(ta)),
             "  (b) sources, set_input_texture_sources    : median %.3f ms  (min %.3f, max %.3f)   H2D %.2f MB, 2 launches"
             % (med(tbs), min(tbs), max(tbs), nbytes(sources) / 1e6),
             "  resized bytes equal Pillow's, cloth channels of the U-Net input equal after either hand-over: %s" % same]
    del m
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256, help="load size = crop size")
    ap.add_argument("--sources", default="256x256,768x1024", help="comma-separated H0xW0 source sizes")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = engine.Context(workspace_mb=1024)
    lines = ["texture batch hand-over from decoded images, %s, bs %d, load size %d, pinned host memory, interleaved, %d repetitions each"
             % (torch.cuda.get_device_name(0), a.batch, a.size, a.reps)]
    for s in a.sources.split(","):
        h0, w0 = (int(v) for v in s.split("x"))
        lines += measure(ctx, a.batch, a.size, (h0, w0), a.reps, a.warmup)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
