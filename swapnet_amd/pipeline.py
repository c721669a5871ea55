"""Two-stage inference on the device.

The reference's inference.py runs the warp stage, writes `fakes[0].argmax(dim=0)` as a sparse
.npz per image (inference.py:140-149, datasets/data_utils.py:311-327), then a second pass
loads those files as the cloth input of the texture stage (inference.py:169-180,
data_utils.py:298-343).  Here the hand-off stays in HBM and the whole sequence is one library
object (`swn_pipeline`): warp forward -> argmax labels on the NHWC output -> one-hot expansion
straight into the texture model's input buffers -> texture forward, captured into a hipGraph on the
first call and replayed afterwards (batch-size-1 inference is launch-latency bound otherwise).  The
label map is exactly what the .npz would contain, so the result equals the reference's two passes.
"""
import torch

from . import engine
from .modules.native import NativeBackend


class TwoStagePipeline:
    def __init__(self, warp_state_dict, texture_state_dict, img_size=128, num_roi=12, ctx=None, lib=None, use_graph=True, images=None):
        """images = dict(body_norm_stats=(mean3, std3), texture_norm_stats=(mean3, std3)[, colours=(num_roi,3) uint8, width_factor=0.01,
        reference_quirk=True, png=False, png_rows_per_chunk=0]) arms the image sheet: every call then also leaves the six images inference.py
        would save, as uint8 on the device inside the same graph; `images()` fetches them.  png=True also encodes them as PNG on the
        device (csrc/png_encode.hip), still inside the graph; `images_png()` fetches the files as bytes."""
        self.ctx = ctx or engine.default_context(lib=lib)
        self.use_graph = use_graph
        self.image_options = dict(images) if images is not None else None
        if self.image_options is not None:
            missing = {"body_norm_stats", "texture_norm_stats"} - set(self.image_options)
            unknown = set(self.image_options) - {"body_norm_stats", "texture_norm_stats", "colours", "width_factor", "reference_quirk", "png",
                                                 "png_rows_per_chunk"}
            if missing or unknown:
                raise ValueError("images: missing %s, unknown %s" % (sorted(missing), sorted(unknown)))
        self._last = None
        self.warp = NativeBackend("warp", is_train=False, ctx=self.ctx)
        self.texture = NativeBackend("texture", is_train=False, num_roi=num_roi, ctx=self.ctx,
                                     default_shape=(1, img_size, img_size))
        self.warp.load_state_dict(engine.NET_G, warp_state_dict)
        self.texture.load_state_dict(engine.NET_G, texture_state_dict)
        self._pipes = {}
        self.last_call_was_graph_replay = False

    def _pipe(self, B, H, W):
        w, t = self.warp.ensure(B, H, W), self.texture.ensure(B, H, W)
        key = (B, H, W)
        if key not in self._pipes:
            self._pipes[key] = engine.NativePipeline(w, t)
            if self.image_options is not None:
                from .util.draw_rois import BODY_COLORS
                o = self.image_options
                colours = o["colours"] if o.get("colours") is not None else BODY_COLORS[:t.num_roi]
                width = max(1, int(round(o.get("width_factor", 0.01) * W)))
                self._pipes[key].enable_images(o["body_norm_stats"], o["texture_norm_stats"], colours, width, o.get("reference_quirk", True))
                if o.get("png"):
                    self._pipes[key].enable_png(o.get("png_rows_per_chunk", 0))
        return w, t, self._pipes[key]

    def images(self):
        """The images of the last call, name -> (B,H,W,3) uint8 numpy array, under the reference's visual names (warp_model.py:60,
        texture_model.py:58-63): inputs_decoded, bodys_unnormalized, fakes_decoded, textures_unnormalized (ROI outlines drawn),
        cloths_decoded (the same array as fakes_decoded: the texture stage's cloth input IS the warped label map), fakes,
        fakes_scaled.  One device-to-host copy."""
        if self.image_options is None:
            raise ValueError("images(): the pipeline was built without images=dict(body_norm_stats=..., texture_norm_stats=...)")
        if self._last is None:
            raise ValueError("images(): call the pipeline first")
        out = self._last.images()
        out["cloths_decoded"] = out["fakes_decoded"]
        return out

    def images_png(self):
        """The images of the last call as PNG files, name -> list of B `bytes` under the names of `images()` (cloths_decoded is
        fakes_decoded's list): what util.save_image would write for each (util/util.py:54-69), filtered and deflated on the device.
        Pillow opens them to exactly the arrays of `images()`."""
        if self.image_options is None or not self.image_options.get("png"):
            raise ValueError("images_png(): the pipeline was built without images=dict(..., png=True)")
        if self._last is None:
            raise ValueError("images_png(): call the pipeline first")
        out = self._last.png()
        out["cloths_decoded"] = out["fakes_decoded"]
        return out

    @torch.no_grad()
    def __call__(self, bodys, input_cloths, textures, rois, return_labels=False):
        """bodys (B,3,H,W), input_cloths (B,19,H,W) one-hot or (B,H,W) int labels, textures
        (B,3,H,W), rois (B,R,4) -> generated textures (B,3,H,W) [, warped cloth labels (B,H,W)].
        The whole device sequence is ONE library call (swn_pipeline_run); from the second call on a shape it is a
        hipGraph replay."""
        B, _, H, W = bodys.shape
        w, t, pipe = self._pipe(B, H, W)
        w.set_input(0, bodys)
        if input_cloths.dim() == 3 and not input_cloths.is_floating_point():
            w.set_input_labels(1, input_cloths)
        else:
            w.set_input(1, input_cloths)
        t.set_input(0, textures)
        if self.image_options is not None:
            engine.check_roi_boxes(rois)                # Pillow's ValueError for a reversed box, before anything is launched
        t.set_input(1, rois)
        self._last = pipe
        self.last_call_was_graph_replay = pipe.run(self.use_graph)
        out = t.output()
        return (out, pipe.labels()) if return_labels else out
