"""util.draw_rois of the reference (/root/reference/util/draw_rois.py:1-47): the ROI rectangles of a texture batch outlined on the
textures, one pass on the device (engine.op_image_u8) instead of a Pillow loop per image and per box."""
import colorsys

import numpy as np

NUM_BODY_LABELS = 12


def _hls_palette(n, h=0.01, l=0.6, s=0.65):
    return [colorsys.hls_to_rgb((i / n + h) % 1.0, l, s) for i in range(n)]


# The reference takes (numpy.array(seaborn.color_palette("hls", 12)) * 255).astype(uint8).  seaborn is not a dependency here, so the
# table is restated from its published definition (hls_palette: hues i / n + 0.01, lightness 0.6, saturation 0.65, colorsys.
# hls_to_rgb), times 255, truncated.  UNPINNED: nothing here compares it with seaborn's own output (its hues come from numpy.linspace,
# and a last-bit difference can move a truncated byte by one).  It is data and an argument of the drawing, not arithmetic of it.
BODY_COLORS = (np.array(_hls_palette(NUM_BODY_LABELS)) * 255).astype(np.uint8)


def draw_rois_on_texture(rois, texture_tensors, width_factor=0.01, *, colors=None, ctx=None):
    """util/draw_rois.py:16-47: rois (B,R,4) rows x0, y0, x1, y1, texture_tensors (B,3,H,W) float -> (B,H,W,3) uint8 numpy: tensor2im
    of every texture with ROI r outlined in BODY_COLORS[r], width int(round(width_factor * W)), later boxes over earlier ones, by
    Pillow's ImageDraw.rectangle rule.  A width of 0 draws nothing, as Pillow's does; a box with x1 < x0 or y1 < y0 raises Pillow's
    ValueError before anything is launched.  BODY_COLORS is unpinned against seaborn (see above); pass `colors` (R,3) to override."""
    from .. import engine
    ctx = ctx or engine.default_context()
    width = int(round(width_factor * texture_tensors.shape[3]))
    if width == 0:
        return engine.op_image_u8(ctx, texture_tensors).cpu().numpy()
    table = np.asarray(BODY_COLORS if colors is None else colors, dtype=np.uint8)
    r = rois.shape[1]
    if r > len(table):
        raise ValueError("draw_rois_on_texture: %d ROIs per image but %d colours" % (r, len(table)))
    return engine.op_image_u8(ctx, texture_tensors, rois=rois, colours=table[:r], width=width).cpu().numpy()
