"""What the saved images of two-stage inference cost per image, batch 1, at 128 x 128 and 256 x 256 (median of --iters after warm-up):

  (a) today's host path: pipeline replay, then self.fakes of both stages read back as fp32 and the host helpers of
      compute_visuals() -- unnormalize, scale_tensor(scale_each=True), decode_cloth_labels (its own upload, kernel, read-back) --
      and a numpy restatement of util.tensor2im for the six images (no ROI outlines: that path has none);
  (b) the armed pipeline: pipeline replay with the image launches inside the graph, then images(): one copy of the uint8 sheet;
  (c) the graph replay alone, with and without the image launches, between HIP events.

PNG encoding is outside all three.  `python tools/infer_images_ab.py [--out FILE]` on the MI355X; the lines it prints are the record
(profiles/infer_images.txt)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import swapnet_oracle as O          # noqa: E402  (seeded weights and batches only)
from swapnet_amd import engine                  # noqa: E402
from swapnet_amd.util.decode_labels import decode_cloth_labels      # noqa: E402
from swapnet_amd.util.draw_rois import BODY_COLORS                  # noqa: E402
from swapnet_amd.util.util import scale_tensor, unnormalize         # noqa: E402

BODY_STATS = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
TEX_STATS = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))


def numpy_tensor2im(t):
    """util/util.py:23-32 on a float tensor; a decoded uint8 visual as its own bytes."""
    a = t[0].cpu().numpy()
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a.transpose(1, 2, 0))
    if a.shape[0] == 1:
        a = np.tile(a, (3, 1, 1))
    return ((np.transpose(a, (1, 2, 0)) + 1) / 2.0 * 255.0).astype(np.uint8)


def build(ctx, size, weights, batch):
    warp = engine.NativeModel(ctx, "warp", 1, size, size, is_train=False)
    tex = engine.NativeModel(ctx, "texture", 1, size, size, is_train=False)
    warp.load_state_dict(engine.NET_G, weights[0])
    tex.load_state_dict(engine.NET_G, weights[1])
    bodys, inputs, textures, rois = batch
    warp.set_input(0, bodys); warp.set_input(1, inputs); tex.set_input(0, textures); tex.set_input(1, rois)
    return warp, tex, engine.NativePipeline(warp, tex)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = engine.Context(workspace_mb=1024)
    lines = ["infer_images_ab: %s (%s), %s, batch 1, median of %d after %d warm-up calls" %
             (torch.cuda.get_device_name(ctx.device), getattr(torch.cuda.get_device_properties(ctx.device), "gcnArchName", "?"),
              time.strftime("%Y-%m-%d"), args.iters, args.warmup)]
    for size in args.sizes:
        torch.manual_seed(0)
        weights = (O.warp_module_params(), O.texture_module_params(img_size=size))
        bodys, inputs, _ = O.synth_warp_batch(1, size, size, seed=1)
        textures, rois, _, _ = O.synth_texture_batch(1, size, size, seed=2)
        batch = (bodys, inputs, textures, rois)
        warp, tex, plain = build(ctx, size, weights, batch)
        warp_b, tex_b, armed = build(ctx, size, weights, batch)
        armed.enable_images(BODY_STATS, TEX_STATS, BODY_COLORS, max(1, int(round(0.01 * size))))
        for p in (plain, armed):
            p.run(True)
            assert p.run(True), "the second call must be a graph replay"

        def host_path():
            plain.run(True)
            fakes, warped = tex.output().cpu(), warp.output()
            visuals = [decode_cloth_labels(inputs, ctx=ctx), unnormalize(bodys, *BODY_STATS), decode_cloth_labels(warped, ctx=ctx),
                       unnormalize(textures, *TEX_STATS), fakes, scale_tensor(fakes, scale_each=True)]
            return [numpy_tensor2im(v) for v in visuals]

        def device_path():
            armed.run(True)
            return armed.images()

        # the two paths make the same images where both are defined (no outlines on the host path, so not textures_unnormalized)
        host, dev = host_path(), device_path()
        for i, name in enumerate(engine.IMAGE_NAMES):
            if name != "textures_unnormalized":
                assert np.array_equal(host[i], dev[name][0]), name
        a = median_ms(host_path, args.warmup, args.iters)
        b = median_ms(device_path, args.warmup, args.iters)
        c0 = median_event_ms(ctx, lambda: plain.run(True), args.warmup, args.iters)
        c1 = median_event_ms(ctx, lambda: armed.run(True), args.warmup, args.iters)
        lines += ["%d x %d  (a) replay + host visuals      %8.3f ms per image" % (size, size, a),
                  "%d x %d  (b) armed replay + images()     %8.3f ms per image   (a)/(b) = %.2f" % (size, size, b, a / b),
                  "%d x %d  (c) graph replay, HIP events:   %8.3f ms without, %8.3f ms with the image launches (+%.3f ms, %.1f %% of the forward pass)"
                  % (size, size, c0, c1, c1 - c0, 100.0 * (c1 - c0) / c0)]
        for obj in (plain, armed, warp, tex, warp_b, tex_b):
            obj.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
