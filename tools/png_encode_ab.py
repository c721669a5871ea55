"""What writing the six saved images of one sample as PNG costs, batch 1, at 128 x 128 and 256 x 256 (median of --iters after warm-up),
for the synthetic batches tools/infer_images_ab.py uses:

  (a) the host's zlib: Image.fromarray(a).save(BytesIO, "PNG") for the six arrays images() returned (the arrays are staged: neither the
      replay nor the copy of the sheet is in the figure), at Pillow's default settings and at compress_level=1;
  (b) images_png(): armed replay with the PNG launches inside the graph, the two device-to-host copies (sizes, used part of the
      streams) and the container (CRC-32) on the host; next to it the replay + images() it is to be compared with when (a) is added;
  (c) the graph replay alone between HIP events, with the image launches only and with the PNG launches behind them;
  and the bytes each path writes for the six files.

`python tools/png_encode_ab.py [--out FILE]` on the MI355X; the lines it prints are the record (profiles/png_encode.txt)."""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import swapnet_oracle as O          # noqa: E402  (seeded weights and batches only)
from swapnet_amd import engine                  # noqa: E402
from swapnet_amd.util.draw_rois import BODY_COLORS                  # noqa: E402

BODY_STATS = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
TEX_STATS = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))


def build(ctx, size, weights, batch, png):
    warp = engine.NativeModel(ctx, "warp", 1, size, size, is_train=False)
    tex = engine.NativeModel(ctx, "texture", 1, size, size, is_train=False)
    warp.load_state_dict(engine.NET_G, weights[0])
    tex.load_state_dict(engine.NET_G, weights[1])
    bodys, inputs, textures, rois = batch
    warp.set_input(0, bodys); warp.set_input(1, inputs); tex.set_input(0, textures); tex.set_input(1, rois)
    pipe = engine.NativePipeline(warp, tex)
    pipe.enable_images(BODY_STATS, TEX_STATS, BODY_COLORS, max(1, int(round(0.01 * size))))
    if png:
        pipe.enable_png()
    pipe.run(True)
    assert pipe.run(True), "the second call must be a graph replay"
    return warp, tex, pipe


def median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def median_event_ms(ctx, fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ctx.sync()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def pillow_files(arrays, **kw):
    out = []
    for a in arrays:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="PNG", **kw)
        out.append(buf.getvalue())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = engine.Context(workspace_mb=1024)
    lines = ["png_encode_ab: %s (%s), host with %d CPUs, Pillow %s, %s, batch 1, six images, median of %d after %d warm-up calls" %
             (torch.cuda.get_device_name(ctx.device), getattr(torch.cuda.get_device_properties(ctx.device), "gcnArchName", "?"),
              os.cpu_count(), Image.__version__, time.strftime("%Y-%m-%d"), args.iters, args.warmup)]
    for size in args.sizes:
        torch.manual_seed(0)
        weights = (O.warp_module_params(), O.texture_module_params(img_size=size))
        bodys, inputs, _ = O.synth_warp_batch(1, size, size, seed=1)
        textures, rois, _, _ = O.synth_texture_batch(1, size, size, seed=2)
        batch = (bodys, inputs, textures, rois)
        warp, tex, images_only = build(ctx, size, weights, batch, png=False)
        warp_b, tex_b, with_png = build(ctx, size, weights, batch, png=True)
        arrays = [v[0] for v in images_only.images().values()]

        def device_path():
            with_png.run(True)
            return with_png.png()

        def sheet_path():
            images_only.run(True)
            return images_only.images()

        dev = [f[0] for f in device_path().values()]
        for f, a in zip(dev, arrays):                    # the device's files hold the images the host would have saved
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), a)
        a6 = median_ms(lambda: pillow_files(arrays), args.warmup, args.iters)
        a1 = median_ms(lambda: pillow_files(arrays, compress_level=1), args.warmup, args.iters)
        b = median_ms(device_path, args.warmup, args.iters)
        s = median_ms(sheet_path, args.warmup, args.iters)
        c0 = median_event_ms(ctx, lambda: images_only.run(True), args.warmup, args.iters)
        c1 = median_event_ms(ctx, lambda: with_png.run(True), args.warmup, args.iters)
        n6, n1, nd = (sum(len(f) for f in fs) for fs in (pillow_files(arrays), pillow_files(arrays, compress_level=1), dev))
        tag = "%d x %d " % (size, size)
        lines += [tag + " (a) Pillow save x 6, default         %8.3f ms   %8d bytes" % (a6, n6),
                  tag + " (a) Pillow save x 6, compress_level=1 %8.3f ms   %8d bytes" % (a1, n1),
                  tag + " (b) armed replay + images_png()       %8.3f ms   %8d bytes   (replay + images(): %.3f ms)" % (b, nd, s),
                  tag + "     files on the host:  replay + images() + (a) default = %.3f ms,  / (b) = %.2f;  with compress_level=1 = %.3f ms,  / (b) = %.2f"
                  % (s + a6, (s + a6) / b, s + a1, (s + a1) / b),
                  tag + " (c) graph replay, HIP events:         %8.3f ms with the image launches, %8.3f ms with the PNG launches behind them (+%.3f ms)"
                  % (c0, c1, c1 - c0)]
        for obj in (images_only, with_png, warp, tex, warp_b, tex_b):
            obj.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
