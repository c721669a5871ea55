"""Thin Python handles over the C-ABI objects (swn_ctx / swn_model).

torch is used here only for device memory (tensors whose raw pointers are handed to the
library) and, in swapnet_amd.parallel, for torch.distributed.  No arithmetic of the hot path
happens in torch.
"""
import ctypes as C
import os
from collections import OrderedDict

import torch

from . import _C

NET_G, NET_D, NET_VGG = 0, 1, 2
OPT_ADAMW, OPT_ADABOUND = 0, 1
W_WEIGHT, W_GRAD, W_EXP_AVG, W_EXP_AVG_SQ = 0, 1, 2, 3
NORM_KINDS = {"instance": 0, "batch": 1, "none": 2}       # --norm (swn_ctx_set_patchgan_norm)
NETG_KINDS = {"swapnet": 0, "unet_128": 1}                # --netG of the texture stage (swn_texture_model_create_netG)


class Context:
    """One per process / GPU (models/base_model.py:36-40 picks the device in the reference)."""

    def __init__(self, device=None, lib=None, workspace_mb=512, use_torch_stream=True):
        self.lib = lib or _C.lib()
        if self.lib.is_device:
            if not torch.cuda.is_available():
                raise _C.SwapnetHipError("no HIP device visible; swapnet_amd has no CPU path")
            self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
            torch.cuda.set_device(self.device)
            # enqueue on torch's current stream: H2D copies, allocator reuse of the temporaries whose
            # pointers we borrow, and RCCL collectives are then ordered with our kernels for free
            self.torch_stream = torch.cuda.current_stream(self.device)
            stream = C.c_void_p(self.torch_stream.cuda_stream)
            if os.environ.get("SWAPNET_OWN_STREAM") == "1":     # (experiment: the context's main stream is its own, not torch's current one)
                use_torch_stream = False
            dev_index, create = self.device.index, int(not use_torch_stream)
        else:                       # CI host simulator (tests only)
            self.device = torch.device("cpu")
            stream, dev_index, create = None, 0, 0
        h = C.c_void_p()
        self.lib.call("swn_ctx_create", dev_index, stream, create, C.c_size_t(workspace_mb << 20), C.byref(h))
        self.handle = h
        # the library's main stream is its own non-blocking one: nothing orders it with torch's streams (see NativeModel._torch_done)
        self.owns_stream = bool(create)
        self._copy_stream = None

    def upload(self, tensor, dtype, key=None):
        """Host batch -> device on a dedicated copy stream: `set_input` is called right after
        `optimize_parameters` returned (train.py:62-64) while that step's kernels are still running, so the
        H2D transfer (335 MB/step for one-hot cloths at bs 32) hides under them instead of queueing
        behind them.  With `key` the destination is one of two persistent staging buffers per input slot
        (no allocator traffic -- a fresh hipMalloc per step synchronises the device); the copy stream
        waits for the kernel that last read the buffer it is about to overwrite (`consumed`), the main
        stream for the copy.  Returns (device tensor, token for `consumed`)."""
        t = tensor.detach()
        if self.device.type != "cuda" or t.is_cuda:
            return t.to(device=self.device, dtype=dtype).contiguous(), None
        t = t.to(dtype=dtype).contiguous()
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
            self._staging = {}
        cs, main = self._copy_stream, torch.cuda.current_stream(self.device)
        if key is None:
            with torch.cuda.stream(cs):
                d = t.to(self.device, non_blocking=True)
            main.wait_stream(cs)
            d.record_stream(main)
            return d, None
        st = self._staging.setdefault(key, {"bufs": [None, None], "events": [None, None], "i": 0})
        i = st["i"]
        st["i"] ^= 1
        buf = st["bufs"][i]
        if buf is None or buf.shape != t.shape or buf.dtype != dtype:
            buf = torch.empty(t.shape, dtype=dtype, device=self.device)
            st["bufs"][i], st["events"][i] = buf, None
        if st["events"][i] is not None:
            cs.wait_event(st["events"][i])
        with torch.cuda.stream(cs):
            buf.copy_(t, non_blocking=True)
        main.wait_stream(cs)
        return buf, (key, i)

    def consumed(self, token):
        """The kernel reading an `upload(..., key=)` buffer has been enqueued on the current stream."""
        if token is None:
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._staging[token[0]]["events"][token[1]] = ev

    def set_overlap(self, on):
        """Side stream on/off (results identical; off gives un-overlapped per-kernel timings)."""
        self.lib.call("swn_ctx_set_overlap", self.handle, int(bool(on)))

    def sync(self):
        self.lib.call("swn_ctx_sync", self.handle)

    def attach_comm(self, fn_ptr, comm, world):
        """swn_ctx_attach_comm: hand the library an all-reduce entry point (address of a function with ncclAllReduce's signature)
        and the communicator to call it on; fn_ptr None detaches.  See swapnet_amd.parallel.NativeComm."""
        self.lib.call("swn_ctx_attach_comm", self.handle, C.c_void_p(fn_ptr) if fn_ptr else None,
                      comm if comm is not None else None, int(world))

    def route_trace(self, on):
        """Start (clears the log) / stop recording which kernel every layer launches (swn_route_trace)."""
        self.lib.call("swn_route_trace", int(bool(on)))

    def route_report(self):
        """The distinct "<layer> <phase> <kernel[shape, schedule]>" lines recorded since route_trace(True), in first-use order."""
        need = self.lib.dll.swn_route_report(None, 0)
        buf = C.create_string_buffer(need + 16)
        self.lib.dll.swn_route_report(buf, need + 16)
        return [l for l in buf.value.decode().split("\n") if l]

    def bytes_allocated(self):
        n = C.c_size_t()
        self.lib.call("swn_ctx_bytes_allocated", self.handle, C.byref(n))
        return n.value

    def close(self):
        if getattr(self, "handle", None):
            comm = getattr(self, "native_comm", None)       # the communicator the library's exchange runs on dies with its context,
            if comm is not None:                            # before it: parallel.NativeComm registers itself here
                self.native_comm = None
                comm.close()
            self.lib.call("swn_ctx_destroy", self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=None, lib=None):
    key = (id(lib) if lib is not None else 0, str(device))
    if key not in _default_ctx:
        _default_ctx[key] = Context(device=device, lib=lib)
    return _default_ctx[key]


class NativeModel:
    """swn_model handle: generator (+ discriminator, optimizers) living in library-owned
    NHWC arenas.  Tensors cross the boundary as NCHW fp32, exactly as the reference holds them."""

    def __init__(self, ctx, kind, batch, height, width, is_train=True, dropout=0.5, num_roi=12, body_channels=3,
                 cloth_channels=19, n_layers_D=3, share=None, norm="instance", netG="swapnet"):
        """share = another NativeModel of the same kind: the new model uses ITS parameter arenas (weights, gradients, Adam
        moments, step counters) and owns only activations -- the model of another batch size on the same training state
        (swn_model_create_shared).  netG (texture models): "swapnet", the ROI-pooled TextureModule, or "unet_128", the plain
        BatchNorm pix2pix U-Net on the textures alone; a sharing model inherits its sharer's."""
        if netG not in NETG_KINDS:
            raise ValueError("Cannot find implementation for " + str(netG))
        if netG != "swapnet" and kind != "texture":
            raise ValueError("netG %s belongs to the texture stage" % netG)
        self.netG = netG
        self.ctx, self.lib, self.kind = ctx, ctx.lib, kind
        self.B, self.H, self.W, self.is_train = batch, height, width, is_train
        self.body_channels, self.cloth_channels = body_channels, cloth_channels
        self.n_layers_D = int(n_layers_D)
        if norm not in NORM_KINDS:
            raise NotImplementedError("normalization layer [%s] is not found" % norm)
        self.norm = norm
        self.share = share
        self.num_roi = share.num_roi if share is not None else int(num_roi)
        if share is not None:
            if share.kind != kind:
                raise ValueError("a sharing model must be of its sharer's kind")
            h = C.c_void_p()
            self.lib.call("swn_model_create_shared", share.handle, batch, height, width, C.byref(h))
            self.is_train, self.body_channels, self.cloth_channels = share.is_train, share.body_channels, share.cloth_channels
            self.n_layers_D, self.out_channels, self.norm = share.n_layers_D, share.out_channels, share.norm
            self.netG = share.netG
            self.handle = h
            self._keep = []
            return
        # a context-level option read at model construction (define_D's n_layers_D, base_gan.py:147): set it for this model,
        # whatever an earlier model on the same context asked for
        self.lib.call("swn_ctx_set_patchgan_layers", ctx.handle, self.n_layers_D)
        self.lib.call("swn_ctx_set_patchgan_norm", ctx.handle, NORM_KINDS[norm])
        h = C.c_void_p()
        if kind == "warp":
            self.lib.call("swn_warp_model_create_ex", ctx.handle, batch, height, width, int(is_train),
                          C.c_float(dropout), body_channels, cloth_channels, C.byref(h))
            self.out_channels = cloth_channels
        elif kind == "texture":
            self.lib.call("swn_texture_model_create_netG", ctx.handle, batch, height, width, int(is_train), num_roi,
                          cloth_channels, NETG_KINDS[netG], C.byref(h))
            self.out_channels = 3
        else:
            raise ValueError("unknown model kind " + kind)
        self.handle = h
        self._keep = []

    # ---- parameters ---------------------------------------------------------------------
    def param_infos(self, net):
        n = C.c_int()
        self.lib.call("swn_model_param_count", self.handle, net, C.byref(n))
        out = OrderedDict()
        buf = C.create_string_buffer(256)
        for i in range(n.value):
            shape = (C.c_int * 4)()
            nd = C.c_int()
            self.lib.call("swn_model_param_info", self.handle, net, i, buf, 256, C.byref(shape), C.byref(nd))
            out[buf.value.decode()] = tuple(shape[: nd.value])
        return out

    def buffer_infos(self, net):
        """state_dict() buffers of `net` (BatchNorm running statistics: the discriminator and the TextureModule's U-Net under
        norm="batch", the generator of a texture model with netG="unet_128"): name -> (shape, dtype)."""
        n = C.c_int()
        self.lib.call("swn_model_buffer_count", self.handle, net, C.byref(n))
        out = OrderedDict()
        buf = C.create_string_buffer(256)
        for i in range(n.value):
            numel, is64 = C.c_int(), C.c_int()
            self.lib.call("swn_model_buffer_info", self.handle, net, i, buf, 256, C.byref(numel), C.byref(is64))
            out[buf.value.decode()] = ((), torch.int64) if is64.value else ((numel.value,), torch.float32)
        return out

    def set_buffer(self, net, name, tensor, dtype):
        t = tensor.detach().to(device=self.ctx.device, dtype=dtype).contiguous()
        self._torch_done()
        self.lib.call("swn_model_buffer_set", self.handle, net, name.encode(), _C.ptr(t))
        self._sync_if_needed()

    def get_buffer(self, net, name, shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=self.ctx.device)
        self.lib.call("swn_model_buffer_get", self.handle, net, name.encode(), _C.ptr(t))
        self._sync_if_needed()
        return t

    def _dev(self, t):
        return t.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()

    def set_param(self, net, name, tensor, which=W_WEIGHT):
        t = self._dev(tensor)
        self._torch_done()
        self.lib.call("swn_model_param_set", self.handle, net, which, name.encode(), _C.ptr(t))
        self._sync_if_needed()

    def get_param(self, net, name, shape, which=W_WEIGHT):
        t = torch.empty(shape, dtype=torch.float32, device=self.ctx.device)
        self.lib.call("swn_model_param_get", self.handle, net, which, name.encode(), _C.ptr(t))
        self._sync_if_needed()
        return t

    def _sync_if_needed(self):
        # the library runs on torch's current stream, so torch frees/reuses are ordered; a
        # private stream needs an explicit sync before the temporaries die or torch reads what the library wrote
        if self.ctx.owns_stream:
            self.ctx.sync()

    def _torch_done(self):
        """Before the library reads a tensor torch just produced (an upload, a conversion): on torch's current stream the call is
        ordered behind it for free; a context that owns its stream (hipStreamNonBlocking, not even ordered with the null stream)
        has to wait for torch.  Without this, the pack kernel of one parameter could still be reading the temporary that torch's
        allocator had already handed to the next parameter's upload."""
        if self.ctx.owns_stream:
            torch.cuda.current_stream(self.ctx.device).synchronize()

    def load_state_dict(self, net, sd, which=W_WEIGHT, strict=True):
        infos = self.param_infos(net)
        buffers = self.buffer_infos(net) if which == W_WEIGHT else {}       # (the optimizer's moments have no buffers)
        missing = [k for k in list(infos) + list(buffers) if k not in sd]
        unexpected = [k for k in sd if k not in infos and k not in buffers]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing}, unexpected {unexpected}")
        for k, shape in infos.items():
            if k in sd:
                if tuple(sd[k].shape) != tuple(shape):
                    raise RuntimeError(f"size mismatch for {k}: {tuple(sd[k].shape)} vs {tuple(shape)}")
                self.set_param(net, k, sd[k], which)
        for k, (shape, dtype) in buffers.items():
            if k in sd:
                if tuple(sd[k].shape) != tuple(shape):
                    raise RuntimeError(f"size mismatch for {k}: {tuple(sd[k].shape)} vs {tuple(shape)}")
                self.set_buffer(net, k, sd[k], dtype)
        self.ctx.sync()

    def state_dict(self, net, which=W_WEIGHT, to_cpu=False):
        out = OrderedDict()
        # a BatchNorm site's buffers follow its weight and bias, as in torch's module-tree order
        by_site = OrderedDict()
        if which == W_WEIGHT:
            for k, info in self.buffer_infos(net).items():
                by_site.setdefault(k.rsplit(".", 1)[0], []).append((k, info))
        for k, shape in self.param_infos(net).items():
            t = self.get_param(net, k, shape, which)
            out[k] = t.cpu() if to_cpu else t
            site = k.rsplit(".", 1)[0]
            if k.endswith(".bias") and site in by_site:
                for kb, (bshape, dtype) in by_site.pop(site):
                    t = self.get_buffer(net, kb, bshape, dtype)
                    out[kb] = t.cpu() if to_cpu else t
        for entries in by_site.values():
            for kb, (bshape, dtype) in entries:
                t = self.get_buffer(net, kb, bshape, dtype)
                out[kb] = t.cpu() if to_cpu else t
        self.ctx.sync()
        return out

    def optim_step_count(self, net, value=None):
        if value is None:
            n = C.c_int()
            self.lib.call("swn_model_optim_step_get", self.handle, net, C.byref(n))
            return n.value
        self.lib.call("swn_model_optim_step_set", self.handle, net, int(value))

    def set_hyper(self, **kw):
        h = _C.SwnHyper(lr=1e-4, d_lr=4e-4, weight_decay=0.0, d_weight_decay=0.01, b1=0.9, b2=0.999,
                        lambda_gan=1.0, lambda_ce=100.0, lambda_l1=10.0, lambda_content=20.0,
                        lambda_style=1e-8, gan_mode=0, warp_mode_ce=0, grad_scale=1.0, d_b1=-1.0, d_b2=-1.0,
                        gp_mode=0, lambda_gp=10.0)
        for k, v in kw.items():
            setattr(h, k, v)
        self.lib.call("swn_model_set_hyper", self.handle, C.byref(h))

    def set_optimizer(self, net, kind=OPT_ADAMW, final_lr=0.1, base_lr=0.0, gamma=1e-3):
        """The update optimizer_step / step apply to `net` (swn_model_set_optimizer): OPT_ADAMW or OPT_ADABOUND with its
        final_lr, base_lr (the lr it was constructed with) and gamma; lr, betas and weight decay stay in set_hyper."""
        self.lib.call("swn_model_set_optimizer", self.handle, net, int(kind), C.c_float(final_lr), C.c_float(base_lr), C.c_float(gamma))

    # ---- data / step ----------------------------------------------------------------------
    def set_input(self, slot, tensor):
        t, token = self.ctx.upload(tensor, torch.float32, key=(id(self), "in", slot))
        if t.dim() == 3:                       # rois (B,R,4)
            n, c, h, w = t.shape[0], t.shape[1], t.shape[2], 1
        else:
            n, c, h, w = t.shape
        self._torch_done()
        self.lib.call("swn_model_set_input", self.handle, slot, _C.ptr(t), n, c, h, w)
        self._sync_if_needed()
        self.ctx.consumed(token)
        self._keep = [t]

    def set_input_labels(self, slot, labels):
        """Integer cloth label map (B,H,W) -> one-hot expansion on the device."""
        t, token = self.ctx.upload(labels, torch.int32, key=(id(self), "lab", slot))
        n, h, w = t.shape
        self._torch_done()
        self.lib.call("swn_model_set_input_labels", self.handle, slot, _C.ptr(t), n, h, w)
        self._sync_if_needed()
        self.ctx.consumed(token)
        self._keep_labels = t

    def set_input_texture_batch(self, batch):
        """Texture model: every input slot from the compact batch dict of datasets.gpu_texture_batch.GpuTextureBatch.collate
        (uint8 images and label maps, raw ROIs, five scalars per sample) in one device launch."""
        specs = (("textures_u8", torch.uint8), ("cloth_labels_u8", torch.uint8), ("rois_raw", torch.float32), ("sample_params", torch.float32))
        dev, tokens = [], []
        for name, dtype in specs:
            t, token = self.ctx.upload(torch.as_tensor(batch[name]), dtype, key=(id(self), "tb", name))
            dev.append(t); tokens.append(token)
        img, lab, rois, sample = dev
        if img.dim() != 4 or img.shape[3] != 3 or lab.dim() != 3 or rois.dim() != 3 or rois.shape[2] != 4 or tuple(sample.shape) != (img.shape[0], 5):
            raise ValueError("texture batch: textures_u8 (B,Hs,Ws,3), cloth_labels_u8 (B,Hl,Wl), rois_raw (B,R,4), sample_params (B,5)")
        if lab.shape[0] != img.shape[0] or rois.shape[0] != img.shape[0]:
            raise ValueError("texture batch: the batch sizes of its tensors differ")
        mean, std = batch["norm_stats"]
        x_min, y_min = batch["crop"][:2]
        self._torch_done()
        self.lib.call("swn_model_set_input_texture_batch", self.handle, _C.ptr(img), img.shape[0], img.shape[1], img.shape[2],
                      _C.ptr(lab), lab.shape[1], lab.shape[2], _C.ptr(rois), rois.shape[1], _C.ptr(sample),
                      (C.c_float * 3)(*mean), (C.c_float * 3)(*std), int(x_min), int(y_min))
        self._sync_if_needed()
        for token in tokens:
            self.ctx.consumed(token)
        self._keep = dev

    def set_input_texture_sources(self, batch):
        """Texture model: every input slot from the sources form of GpuTextureBatch.collate -- `sources_u8` (the decoded images,
        packed back to back), `source_geom` (B,3) int64 {offset, H0, W0}, `resized` (Hs, Ws) and the label maps, ROIs and scalars of
        the compact batch -- in two device launches: Pillow's bilinear resize (swn_op_resize_u8), then the compact hand-over."""
        specs = (("sources_u8", torch.uint8), ("cloth_labels_u8", torch.uint8), ("rois_raw", torch.float32), ("sample_params", torch.float32))
        dev, tokens = [], []
        for name, dtype in specs:
            t, token = self.ctx.upload(torch.as_tensor(batch[name]), dtype, key=(id(self), "ts", name))
            dev.append(t); tokens.append(token)
        src, lab, rois, sample = dev
        geom = _source_geom(batch["source_geom"])
        b = geom.shape[0]
        if src.dim() != 1 or lab.dim() != 3 or rois.dim() != 3 or rois.shape[2] != 4 or tuple(sample.shape) != (b, 5):
            raise ValueError("texture sources: sources_u8 (bytes,), source_geom (B,3), cloth_labels_u8 (B,Hl,Wl), rois_raw (B,R,4), sample_params (B,5)")
        if lab.shape[0] != b or rois.shape[0] != b:
            raise ValueError("texture sources: the batch sizes of its tensors differ")
        hs, ws = (int(v) for v in batch["resized"])
        mean, std = batch["norm_stats"]
        x_min, y_min = batch["crop"][:2]
        self._torch_done()
        self.lib.call("swn_model_set_input_texture_sources", self.handle, _C.ptr(src), C.c_size_t(src.numel()), _C.ptr(geom), b, hs, ws,
                      _C.ptr(lab), lab.shape[1], lab.shape[2], _C.ptr(rois), rois.shape[1], _C.ptr(sample),
                      (C.c_float * 3)(*mean), (C.c_float * 3)(*std), int(x_min), int(y_min))
        self._sync_if_needed()
        for token in tokens:
            self.ctx.consumed(token)
        self._keep = dev

    def set_input_warp_batch(self, batch):
        """Warp model: bodys, input_cloths and (training) target_cloths from the compact batch dict of
        datasets.gpu_warp_batch.GpuWarpBatch.collate (uint8 body images and label maps, the per-channel map table) in one device
        launch.  `input_labels_u8` being the very tensor `target_labels_u8` is (--dataset_mode image) is uploaded once.  A batch that
        carries perspective_resample "bicubic" goes through swn_model_set_input_warp_batch_ex with flags bit 0 (its table may hold
        kind 3, at most one row per chain); any other batch makes the call it always made."""
        tgt_src, in_src = batch["target_labels_u8"], batch["input_labels_u8"]
        names = ["bodys_u8", "input_labels_u8"] + (["target_labels_u8"] if self.is_train and tgt_src is not in_src else [])
        dev, tokens = {}, []
        for name in names:
            dev[name], token = self.ctx.upload(torch.as_tensor(batch[name]), torch.uint8, key=(id(self), "wb", name))
            tokens.append(token)
        body, lab = dev["bodys_u8"], dev["input_labels_u8"]
        tgt = dev.get("target_labels_u8", lab) if self.is_train else None
        maps, nmaps = _warp_maps(batch.get("maps"), body.shape[0], self.cloth_channels)
        bicubic = warp_batch_bicubic(batch)
        _check_warp_kinds(maps, bicubic)
        if maps is not None:
            dev["maps"], token = self.ctx.upload(maps, torch.float64, key=(id(self), "wb", "maps"))
            tokens.append(token)
        _check_warp_batch(body, lab, tgt)
        mean, std = batch["norm_stats"]
        x_min, y_min = batch["crop"][:2]
        if tuple(batch["crop"][2:]) not in ((), (self.W, self.H)):
            raise ValueError("warp batch: its crop window is %s (W, H), the model's %s" % (tuple(batch["crop"][2:]), (self.W, self.H)))
        self._torch_done()
        args = (self.handle, _C.ptr(body), body.shape[0], body.shape[1], body.shape[2], _C.ptr(lab),
                _C.ptr(tgt) if tgt is not None else None, lab.shape[1], lab.shape[2],
                _C.ptr(dev["maps"]) if maps is not None else None, nmaps, (C.c_float * 3)(*mean), (C.c_float * 3)(*std),
                int(batch["load_size"]), int(x_min), int(y_min))
        if bicubic:                         # (a "nearest" batch makes the call it always made)
            self.lib.call("swn_model_set_input_warp_batch_ex", *args, 1)
        else:
            self.lib.call("swn_model_set_input_warp_batch", *args)
        self._sync_if_needed()
        for token in tokens:
            self.ctx.consumed(token)
        self._keep = list(dev.values())

    def forward(self, training=False, seed=0):
        self.lib.call("swn_model_forward", self.handle, int(training), C.c_uint64(seed))

    def dropout_masks(self, net=NET_G, seed=0):
        """The keep/scale factors (0 or 1/(1-p)) a training-mode pass with `seed` applies at every dropout
        site of `net`, in forward order, as NCHW tensors (diagnostic export for the parity tests)."""
        n = C.c_int()
        self.lib.call("swn_model_dropout_sites", self.handle, net, C.byref(n))
        out = []
        for i in range(n.value):
            shape, p = (C.c_int * 4)(), C.c_float()
            self.lib.call("swn_model_dropout_mask", self.handle, net, i, C.c_uint64(seed), None, C.byref(shape), C.byref(p))
            t = torch.empty(tuple(shape), dtype=torch.float32, device=self.ctx.device)
            self.lib.call("swn_model_dropout_mask", self.handle, net, i, C.c_uint64(seed), _C.ptr(t), C.byref(shape), C.byref(p))
            out.append((t, p.value))
        self.ctx.sync()
        return out

    def act_patterns(self, net=NET_G):
        """The branch every LeakyReLU / ReLU / MaxPool of `net` took in the last pass, in forward order: a list of
        (kind, uint8 NCHW tensor on the CPU), kind 1 = output > 0, kind 2 = arg-max window position (diagnostic export:
        the parity tests replay the pattern in the float64 oracle).  net: 0 G, 1 D of the D step ([fake | real]),
        2 D inside the G step, 3 VGG16 on the generated image (texture)."""
        n = C.c_int()
        self.lib.call("swn_model_act_sites", self.handle, net, C.byref(n))
        out = []
        for i in range(n.value):
            shape, kind = (C.c_int * 4)(), C.c_int()
            self.lib.call("swn_model_act_pattern", self.handle, net, i, None, C.byref(shape), C.byref(kind))
            t = torch.empty(tuple(shape), dtype=torch.uint8, device=self.ctx.device)
            self.lib.call("swn_model_act_pattern", self.handle, net, i, _C.ptr(t), C.byref(shape), C.byref(kind))
            self.ctx.sync()
            out.append((kind.value, t.cpu()))
        return out

    def set_style_context(self, all_out, all_tgt, n0):
        """Global (all ranks') generated / target images for the style term of the next backward_G (data parallel)."""
        o = all_out.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
        t = all_tgt.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
        self._torch_done()
        self.lib.call("swn_model_set_style_context", self.handle, _C.ptr(o), _C.ptr(t), int(o.shape[0]), int(n0))
        self._style_keep = (o, t)

    def set_gp_random(self, alpha=None, beta=None):
        """alpha (B,) / (B,1,1,1) and beta (B,C_D,H,W): the gradient-penalty draws of the next backward_D (one-shot)."""
        a = None if alpha is None else alpha.detach().reshape(-1).to(device=self.ctx.device, dtype=torch.float32).contiguous()
        b = None if beta is None else beta.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
        self._torch_done()
        self.lib.call("swn_model_set_gp_random", self.handle, _C.ptr(a), _C.ptr(b))
        self._gp_keep = (a, b)

    def discriminate(self, x, training=True):
        """NLayerDiscriminator.forward on a conditioned input in the reference's channel order (B,C_D,H,W),
        C_D = body + cloth channels (warp, 22 by default) / texture + cloth channels (texture).  training: the module's mode
        (only BatchNorm sites care: batch statistics + running update, or the running buffers)."""
        xd = x.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
        cd = self.cloth_channels + (self.body_channels if self.kind == "warp" else 3)
        if tuple(xd.shape) != (self.B, cd, self.H, self.W):
            raise ValueError("discriminator input must be (%d, %d, %d, %d), got %s" % (self.B, cd, self.H, self.W, tuple(xd.shape)))
        k = self.n_layers_D                     # n stride-2 levels, then two 4x4 stride-1 convs with padding 1 (-1 pixel each)
        shape = (self.B, 1, (self.H >> k) - 2, (self.W >> k) - 2) if k > 0 else (self.B, 1, self.H, self.W)     # 0: PixelDiscriminator
        pred = torch.empty(shape, dtype=torch.float32, device=self.ctx.device)
        self._torch_done()
        self.lib.call("swn_model_set_discriminate_mode", self.handle, int(bool(training)))
        self.lib.call("swn_model_discriminate", self.handle, _C.ptr(xd), _C.ptr(pred))
        self.ctx.sync()
        return pred

    def perceptual(self, output, target, use_style=True, content_w=1.0, style_w=1.0, want_grad=False):
        """PerceptualLoss.forward: returns (losses[2] device tensor = content, style ; d_output or None)."""
        o = output.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
        t = target.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
        if tuple(o.shape) != (self.B, 3, self.H, self.W) or o.shape != t.shape:
            raise ValueError("perceptual loss inputs must both be (%d, 3, %d, %d)" % (self.B, self.H, self.W))
        out2 = torch.empty(2, dtype=torch.float32, device=self.ctx.device)
        d = torch.empty_like(o) if want_grad else None
        self._torch_done()
        self.lib.call("swn_model_perceptual", self.handle, _C.ptr(o), _C.ptr(t), int(bool(use_style)), _C.ptr(out2),
                      C.c_float(content_w), C.c_float(style_w), _C.ptr(d))
        self.ctx.sync()
        return out2, d

    def output(self, slot=0):
        t = torch.empty((self.B, self.out_channels, self.H, self.W), dtype=torch.float32, device=self.ctx.device)
        self.lib.call("swn_model_get_output", self.handle, slot, _C.ptr(t))
        self.ctx.sync()
        return t

    def tap(self, net, name):
        shape = (C.c_int * 4)()
        self.lib.call("swn_model_get_tap", self.handle, net, name.encode(), None, C.byref(shape))
        t = torch.empty(tuple(shape), dtype=torch.float32, device=self.ctx.device)
        self.lib.call("swn_model_get_tap", self.handle, net, name.encode(), _C.ptr(t), C.byref(shape))
        self.ctx.sync()
        return t

    def tap_grad(self, net, name):
        """Gradient w.r.t. a named activation after the last backward pass (diagnostics)."""
        shape = (C.c_int * 4)()
        self.lib.call("swn_model_get_tap_grad", self.handle, net, name.encode(), None, C.byref(shape))
        t = torch.empty(tuple(shape), dtype=torch.float32, device=self.ctx.device)
        self.lib.call("swn_model_get_tap_grad", self.handle, net, name.encode(), _C.ptr(t), C.byref(shape))
        self.ctx.sync()
        return t

    def backward_D(self, label_fake, label_real):
        self.lib.call("swn_model_backward_D", self.handle, C.c_float(label_fake), C.c_float(label_real))

    def backward_G(self, label_real):
        self.lib.call("swn_model_backward_G", self.handle, C.c_float(label_real))

    def backward_G_parts(self):
        """Number of buckets backward_G_part splits the generator backward into."""
        n = C.c_int()
        self.lib.call("swn_model_backward_G_parts", self.handle, C.byref(n))
        return n.value

    def backward_G_part(self, label_real, part):
        """Returns (offset, count) of the generator gradient-arena range that is final after this part."""
        off, cnt = C.c_size_t(), C.c_size_t()
        self.lib.call("swn_model_backward_G_part", self.handle, C.c_float(label_real), part, C.byref(off), C.byref(cnt))
        return off.value, cnt.value

    def optimizer_step(self, net):
        self.lib.call("swn_model_optimizer_step", self.handle, net)

    def optimizer_step_range(self, net, off, count, first):
        self.lib.call("swn_model_optimizer_step_range", self.handle, net, C.c_size_t(off), C.c_size_t(count), int(bool(first)))

    def step(self, labels, training=True, seed=0, captured=False):
        """One G+D optimize_parameters step.  captured=True: the hipGraph form (swn_model_step_captured) -- first call eager,
        second records, later ones replay; bit-identical results."""
        arr = (C.c_float * 3)(*[float(x) for x in labels])
        self.lib.call("swn_model_step_captured" if captured else "swn_model_step", self.handle, C.byref(arr), int(training),
                      C.c_uint64(seed))

    def step_dp(self, labels, training=True, seed=0, after_forward=False):
        """One data-parallel G+D step with the exchange owned by the library (swn_model_step_dp; the context needs a communicator:
        Context.attach_comm / parallel.NativeComm)."""
        arr = (C.c_float * 3)(*[float(x) for x in labels])
        self.lib.call("swn_model_step_dp", self.handle, C.byref(arr), int(training), C.c_uint64(seed), int(bool(after_forward)))

    def losses(self):
        buf = (C.c_float * len(_C.LOSS_NAMES))()
        self.lib.call("swn_model_get_losses", self.handle, C.cast(buf, C.POINTER(C.c_float)), len(_C.LOSS_NAMES))
        return OrderedDict(zip(_C.LOSS_NAMES, [float(x) for x in buf]))

    def grad_arena(self, net):
        """Flat fp32 view of the net's gradient arena as a torch tensor (zero-copy on GPU)."""
        p, n = C.c_void_p(), C.c_size_t()
        self.lib.call("swn_model_grad_arena", self.handle, net, C.byref(p), C.byref(n))
        return _wrap_pointer(p.value, n.value, self.ctx.device)

    def weight_arena(self, net):
        p, n = C.c_void_p(), C.c_size_t()
        self.lib.call("swn_model_weight_arena", self.handle, net, C.byref(p), C.byref(n))
        return _wrap_pointer(p.value, n.value, self.ctx.device)

    def arena(self, net, which):
        p, n = C.c_void_p(), C.c_size_t()
        self.lib.call("swn_model_arena", self.handle, net, which, C.byref(p), C.byref(n))
        return _wrap_pointer(p.value, n.value, self.ctx.device)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.call("swn_model_destroy", self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def op_gan_loss(ctx, pred, gan_mode, label, target_is_real, grad_scale=1.0, want_grad=True):
    """GANLoss value (+ gradient w.r.t. the prediction map) through swn_op_gan_loss.  Returns (loss[1], dpred)."""
    p = pred.detach().to(device=ctx.device, dtype=torch.float32).contiguous()
    shape = tuple(p.shape)
    p4 = p.reshape((shape + (1, 1, 1, 1))[:4]) if p.dim() < 4 else p
    n, c, h, w = p4.shape
    loss = torch.empty(1, dtype=torch.float32, device=ctx.device)
    d = torch.empty_like(p4) if want_grad else None
    ctx.lib.call("swn_op_gan_loss", ctx.handle, int(gan_mode), _C.ptr(p4), n, c, h, w, C.c_float(label),
                 int(bool(target_is_real)), C.c_float(grad_scale), _C.ptr(loss), _C.ptr(d))
    return loss, (d.reshape(shape) if d is not None else None)


LOSS_CE, LOSS_L1, LOSS_NORMED_MSE, LOSS_GRAM = 0, 1, 2, 3
PAD_SENTINEL = 0x7F7F7F7F           # what swn_op_loss / swn_op_bias_grad / the view-level swn_op_* put into every pad channel before the call


def op_loss(ctx, kind, a, b, pad_c=0, scale=1.0, accumulate=False, n0=0, nloc=-1, grad=None, want_grad=True, want_pad=True):
    """One loss kernel through swn_op_loss on (N,C,H,W) operands held in C + pad_c channel buffers.  `grad`: the incoming gradient
    (accumulate; nloc samples when nloc >= 0).  Returns (loss[1], da or None, the gradient buffer's pad channels or None)."""
    a = a.detach().to(device=ctx.device, dtype=torch.float32).contiguous()
    b = b.detach().to(device=ctx.device, dtype=torch.float32).contiguous()
    n, c, h, w = a.shape
    ng = n if nloc < 0 else nloc
    loss = torch.empty(1, dtype=torch.float32, device=ctx.device)
    d = pad = None
    if want_grad:
        d = (grad.detach().to(device=ctx.device, dtype=torch.float32).clone().contiguous() if accumulate
             else torch.empty((ng, c, h, w), dtype=torch.float32, device=ctx.device))
        assert tuple(d.shape) == (ng, c, h, w)
        if want_pad and pad_c > 0:
            pad = torch.empty((ng, pad_c, h, w), dtype=torch.float32, device=ctx.device)
    ctx.lib.call("swn_op_loss", ctx.handle, int(kind), _C.ptr(a), _C.ptr(b), n, c, h, w, int(pad_c), C.c_float(scale),
                 int(bool(accumulate)), int(n0), int(nloc), _C.ptr(loss), _C.ptr(d), _C.ptr(pad))
    return loss, d, pad


def op_bias_grad(ctx, dy, pad_c=0):
    """bias_grad (column sums over N*H*W) through swn_op_bias_grad; dy (N,C,H,W) held in a C + pad_c channel buffer."""
    d = dy.detach().to(device=ctx.device, dtype=torch.float32).contiguous()
    n, c, h, w = d.shape
    db = torch.empty(c, dtype=torch.float32, device=ctx.device)
    ctx.lib.call("swn_op_bias_grad", ctx.handle, _C.ptr(d), n, c, h, w, int(pad_c), _C.ptr(db))
    return db


SSIM_MAX_WINDOW = 15                # ssim_math.h: odd windows 1 .. 15 have a kernel


def _torch_stream_done(ctx):
    """A context with a stream of its own: what torch enqueued for the operands (uploads, the producer's kernels) has finished."""
    if ctx.owns_stream:
        torch.cuda.current_stream(ctx.device).synchronize()


def op_ssim(ctx, img1, img2, window, max_val=1.0, want_map=False, grad=None, want_grad=(False, False)):
    """swn_op_ssim: the SSIM loss of modules.losses (reference modules/losses/__init__.py:128-259) on (B,C,H,W) float32 operands.
    Returns (loss_sum[1] = the plain sum over all elements, loss_map or None, d1 or None, d2 or None).  `grad`: the upstream
    gradient, a (B,C,H,W) tensor (reduction 'none') or a Python scalar; want_grad = which of the two image gradients to compute."""
    a, b = _dev(ctx, img1), _dev(ctx, img2)
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError("ssim: two (B,C,H,W) tensors of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    n, c, h, w = a.shape
    total = torch.empty(1, dtype=torch.float32, device=ctx.device)
    lmap = torch.empty_like(a) if want_map else None
    d1 = torch.empty_like(a) if want_grad[0] else None
    d2 = torch.empty_like(a) if want_grad[1] else None
    gmap, gscalar = None, 0.0
    if d1 is not None or d2 is not None:
        if torch.is_tensor(grad) and grad.dim() > 0:
            gmap = _dev(ctx, grad)
            if gmap.shape != a.shape:
                raise ValueError("ssim: the upstream gradient map must have the images' shape")
        else:
            gscalar = float(grad)
    _torch_stream_done(ctx)
    ctx.lib.call("swn_op_ssim", ctx.handle, _C.ptr(a), _C.ptr(b), n, c, h, w, int(window), C.c_float(max_val), _C.ptr(lmap), _C.ptr(total),
                 _C.ptr(gmap), C.c_float(gscalar), _C.ptr(d1), _C.ptr(d2))
    if ctx.owns_stream:                     # (the caller reads the results on torch's stream)
        ctx.sync()
    return total, lmap, d1, d2


def op_charbonnier(ctx, x, y, eps=1e-6, grad=None, want_grad=(False, False)):
    """swn_op_charbonnier: L1_Charbonnier_loss (reference modules/losses/__init__.py:14-27), sum sqrt((x - y)^2 + eps) over tensors of
    equal numel.  Returns (loss_sum[1], dx or None, dy or None); `grad`: the upstream scalar."""
    a, b = _dev(ctx, x), _dev(ctx, y)
    if a.numel() != b.numel() or a.numel() == 0:
        raise ValueError("charbonnier: two non-empty tensors of equal numel, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    total = torch.empty(1, dtype=torch.float32, device=ctx.device)
    dx = torch.empty_like(a) if want_grad[0] else None
    dy = torch.empty_like(b) if want_grad[1] else None
    _torch_stream_done(ctx)
    ctx.lib.call("swn_op_charbonnier", ctx.handle, _C.ptr(a), _C.ptr(b), C.c_size_t(a.numel()), C.c_float(eps),
                 C.c_float(float(grad) if grad is not None else 0.0), _C.ptr(total), _C.ptr(dx), _C.ptr(dy))
    if ctx.owns_stream:
        ctx.sync()
    return total, dx, dy


def op_texture_batch(ctx, textures_u8, labels_u8, rois_raw, sample_params, mean, std, x_min, y_min, height, width, cloth_channels=19):
    """TextureDataset.__getitem__ for a batch through swn_op_texture_batch: (input_textures, target_textures, cloths, rois) on the
    context's device, NCHW float32 / (B,R,4), from uint8 HWC images (B,Hs,Ws,3), uint8 label maps (B,Hl,Wl), raw ROIs (B,R,4) and
    the (B,5) per-sample scalars {vflip, hflip, roi_scale, cy, cx}."""
    img = torch.as_tensor(textures_u8).to(device=ctx.device, dtype=torch.uint8).contiguous()
    lab = torch.as_tensor(labels_u8).to(device=ctx.device, dtype=torch.uint8).contiguous()
    rois = torch.as_tensor(rois_raw).to(device=ctx.device, dtype=torch.float32).contiguous()
    sample = torch.as_tensor(sample_params).to(device=ctx.device, dtype=torch.float32).contiguous()
    if img.dim() != 4 or img.shape[3] != 3 or lab.dim() != 3 or rois.dim() != 3 or rois.shape[2] != 4:
        raise ValueError("texture batch: textures_u8 (B,Hs,Ws,3), labels_u8 (B,Hl,Wl), rois_raw (B,R,4)")
    b = img.shape[0]
    if lab.shape[0] != b or rois.shape[0] != b or tuple(sample.shape) != (b, 5):
        raise ValueError("texture batch: labels, ROIs and sample_params (B,5) must share the images' batch size")
    inp = torch.empty((b, 3, height, width), dtype=torch.float32, device=ctx.device)
    tgt = torch.empty_like(inp)
    cloths = torch.empty((b, cloth_channels, height, width), dtype=torch.float32, device=ctx.device)
    out = torch.empty(tuple(rois.shape), dtype=torch.float32, device=ctx.device)
    if ctx.owns_stream:                     # (the uploads above ran on torch's stream)
        torch.cuda.current_stream(ctx.device).synchronize()
    ctx.lib.call("swn_op_texture_batch", ctx.handle, _C.ptr(img), b, img.shape[1], img.shape[2], _C.ptr(lab), lab.shape[1], lab.shape[2],
                 _C.ptr(rois), rois.shape[1], _C.ptr(sample), (C.c_float * 3)(*mean), (C.c_float * 3)(*std), int(x_min), int(y_min),
                 int(height), int(width), int(cloth_channels), _C.ptr(inp), _C.ptr(tgt), _C.ptr(cloths), _C.ptr(out))
    return inp, tgt, cloths, out


def _source_geom(geom):
    """(B,3) int64 {byte offset, H0, W0} as a contiguous HOST tensor (the library reads it before the call returns)."""
    g = torch.as_tensor(geom).to(device="cpu", dtype=torch.int64).contiguous()
    if g.dim() != 2 or g.shape[1] != 3 or g.shape[0] < 1:
        raise ValueError("resize_u8: the geometry must be (B, 3) rows {offset, H0, W0}, got %s" % (tuple(g.shape),))
    return g


def pack_u8_images(images):
    """HWC uint8 RGB images of any sizes -> (their bytes back to back, 1-D uint8; (B,3) int64 rows {byte offset, H0, W0})."""
    flat, rows, off = [], [], 0
    for a in images:
        t = torch.as_tensor(a)
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
            raise ValueError("resize_u8: images must be (H0, W0, 3) uint8, got %s %s" % (tuple(t.shape), t.dtype))
        flat.append(t.contiguous().reshape(-1))
        rows.append((off, t.shape[0], t.shape[1]))
        off += t.numel()
    if not flat:
        raise ValueError("resize_u8: an empty list of images")
    return torch.cat(flat), torch.tensor(rows, dtype=torch.int64)


def op_resize_u8_packed(ctx, packed_u8, geom, hs, ws):
    """swn_op_resize_u8 on an already packed byte buffer and its (B,3) geometry: (B, hs, ws, 3) uint8 on the context's device."""
    src = torch.as_tensor(packed_u8).to(device=ctx.device, dtype=torch.uint8).contiguous()
    g = _source_geom(geom)
    if src.dim() != 1:
        raise ValueError("resize_u8: the packed source must be one-dimensional")
    dst = torch.empty((g.shape[0], int(hs), int(ws), 3), dtype=torch.uint8, device=ctx.device)
    if ctx.owns_stream:                     # (the upload above ran on torch's stream)
        torch.cuda.current_stream(ctx.device).synchronize()
    ctx.lib.call("swn_op_resize_u8", ctx.handle, _C.ptr(src), C.c_size_t(src.numel()), _C.ptr(g), g.shape[0], int(hs), int(ws), _C.ptr(dst))
    if ctx.owns_stream:                     # (... and the caller reads dst on it)
        ctx.sync()
    return dst


def op_resize_u8(ctx, images, hs, ws):
    """Pillow's Image.resize((ws, hs), Image.BILINEAR) of a list of (H0, W0, 3) uint8 images, each at its own size, in one device
    launch (swn_op_resize_u8), byte for byte: a (B, hs, ws, 3) uint8 tensor on the context's device."""
    return op_resize_u8_packed(ctx, *pack_u8_images(images), hs, ws)


SRC_FLOAT, SRC_ARGMAX, SRC_LABELS = 0, 1, 2          # ops.h ImageSource
RANGE_SIGNED, RANGE_UNIT = 0, 1                      # ops.h ImageRange
IMAGE_NAMES = ("inputs_decoded", "bodys_unnormalized", "fakes_decoded", "textures_unnormalized", "fakes", "fakes_scaled")


def image_rows(batch, channels, mean, std, reference_quirk=True):
    """The (B, 2C + 1) float32 table of swn_op_image_u8 -- scale[C], shift[C], clamp flag per image -- that restates
    util.unnormalize(tensor, mean, std): under `reference_quirk` its zip over dim 0 (datasets/data_utils.py:41-58: image b < len(mean)
    gets (std[b], mean[b]) on all its channels and is clamped, the images behind it stay as they are, unclamped), otherwise the
    per-channel form for every image."""
    rows = torch.zeros((batch, 2 * channels + 1), dtype=torch.float32)
    rows[:, :channels] = 1.0
    if reference_quirk:
        for b, (m, s) in enumerate(zip(mean, std)):
            if b >= batch:
                break
            rows[b, :channels], rows[b, channels:2 * channels], rows[b, 2 * channels] = float(s), float(m), 1.0
    else:
        if len(mean) != channels or len(std) != channels:
            raise ValueError("image_rows: %d channels, but %d means and %d stds" % (channels, len(mean), len(std)))
        rows[:, :channels] = torch.tensor([float(s) for s in std], dtype=torch.float32)
        rows[:, channels:2 * channels] = torch.tensor([float(m) for m in mean], dtype=torch.float32)
        rows[:, 2 * channels] = 1.0
    return rows


def check_roi_boxes(rois):
    """Pillow's own refusal (ImageDraw.rectangle), raised before the library is called: a box is x0, y0, x1, y1 with x1 >= x0, y1 >= y0."""
    r = torch.as_tensor(rois).detach().to(device="cpu", dtype=torch.float32)
    if r.dim() != 3 or r.shape[2] != 4:
        raise ValueError("ROIs must be (B, R, 4) rows x0, y0, x1, y1, got %s" % (tuple(r.shape),))
    if not bool(torch.isfinite(r).all()):
        raise ValueError("ROI coordinates must be finite")
    if bool((r[..., 2] < r[..., 0]).any()):
        raise ValueError("x1 must be greater than or equal to x0")
    if bool((r[..., 3] < r[..., 1]).any()):
        raise ValueError("y1 must be greater than or equal to y0")
    return r


def op_image_u8(ctx, x=None, labels=None, source=None, rows=None, scale_each=False, range=RANGE_SIGNED, rois=None, colours=None, width=1):
    """swn_op_image_u8: util.tensor2im for a whole batch on the device, with unnormalize (`rows`, see image_rows), scale_tensor(
    scale_each=True), decode_cloth_labels (argmax or label source) and draw_rois_on_texture (`rois` (B,R,4), `colours` (R,3) uint8,
    `width`) folded in.  x (B,C,H,W) float, or labels (B,H,W) int -> (B,H,W,3) uint8 on the context's device."""
    if (x is None) == (labels is None):
        raise ValueError("image_u8: exactly one of x (B,C,H,W) and labels (B,H,W)")
    if source is None:
        source = SRC_LABELS if x is None else SRC_FLOAT
    if (source == SRC_LABELS) != (x is None):
        raise ValueError("image_u8: labels go with SRC_LABELS, x with the float and argmax sources")
    xd = lab = rd = roid = cold = None
    if x is not None:
        xd = _dev(ctx, x)
        if xd.dim() != 4:
            raise ValueError("image_u8: x must be (B,C,H,W), got %s" % (tuple(xd.shape),))
        b, c, h, w = xd.shape
    else:
        lab = _dev(ctx, labels, torch.int32)
        if lab.dim() != 3:
            raise ValueError("image_u8: labels must be (B,H,W), got %s" % (tuple(lab.shape),))
        (b, h, w), c = lab.shape, 0
    if rows is not None:
        rd = _dev(ctx, torch.as_tensor(rows))
        if tuple(rd.shape) != (b, 2 * c + 1):
            raise ValueError("image_u8: rows must be (B, 2C + 1) = %s, got %s" % ((b, 2 * c + 1), tuple(rd.shape)))
    r = 0
    if rois is not None:
        roid = check_roi_boxes(rois).to(ctx.device).contiguous()
        r = roid.shape[1]
        if roid.shape[0] != b:
            raise ValueError("image_u8: ROIs for %d images, batch of %d" % (roid.shape[0], b))
        cold = _dev(ctx, torch.as_tensor(colours), torch.uint8)
        if tuple(cold.shape) != (r, 3):
            raise ValueError("image_u8: colours must be (R, 3) = %s, got %s" % ((r, 3), tuple(cold.shape)))
    out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=ctx.device)
    if ctx.owns_stream:                     # (the uploads above ran on torch's stream)
        torch.cuda.current_stream(ctx.device).synchronize()
    ctx.lib.call("swn_op_image_u8", ctx.handle, _C.ptr(xd), b, c, h, w, _C.ptr(lab), int(source), _C.ptr(rd), int(bool(scale_each)),
                 int(range), _C.ptr(roid), r, _C.ptr(cold), int(width), _C.ptr(out))
    return out


def png_stream_bound(h, w, rows_per_chunk=0, lib=None):
    """swn_png_stream_bound: no stream of op_png_encode for this shape is longer.  ValueError for a shape the encoder refuses."""
    out = C.c_size_t()
    (lib or _C.lib()).call("swn_png_stream_bound", int(h), int(w), int(rows_per_chunk), C.byref(out))
    return int(out.value)


def op_png_encode(ctx, images, rows_per_chunk=0, out=None):
    """swn_op_png_encode: the filtering and deflate of util.save_image (util/util.py:54-69) on the device.  images (n,H,W,3) uint8,
    device or host, tensor or numpy array -> (streams (n, stride) uint8, sizes (n,) int32), both on the context's device: stream i is
    streams[i, :sizes[i]], a zlib stream of the PNG-filtered scanlines (util/png.py png_container makes the file).  `out`: a
    contiguous (n, stride >= png_stream_bound) uint8 device tensor to write into; bytes behind a stream are left as they are."""
    img = _dev(ctx, torch.as_tensor(images), torch.uint8)
    if img.dim() != 4 or img.shape[3] != 3:
        raise ValueError("png_encode: images must be (n,H,W,3) uint8, got %s" % (tuple(img.shape),))
    n, h, w, _ = img.shape
    bound = png_stream_bound(h, w, rows_per_chunk, lib=ctx.lib)
    if out is None:
        out = torch.empty((n, (bound + 15) // 16 * 16), dtype=torch.uint8, device=ctx.device)
    if out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != n or out.shape[1] < bound or not out.is_contiguous() \
            or out.device.type != img.device.type:
        raise ValueError("png_encode: out must be a contiguous (n, stride >= %d) uint8 tensor on the context's device" % bound)
    sizes = torch.zeros((n,), dtype=torch.int32, device=ctx.device)
    if ctx.owns_stream:                     # (the uploads above ran on torch's stream)
        torch.cuda.current_stream(ctx.device).synchronize()
    ctx.lib.call("swn_op_png_encode", ctx.handle, _C.ptr(img), n, h, w, int(rows_per_chunk), _C.ptr(out), out.shape[1], _C.ptr(sizes))
    return out, sizes


AMAX_SLOT = 256                     # floats of one amax slot (ops.h)
EW_ACT_FWD, EW_ACT_BWD, EW_AXPY = 0, 1, 2
RS_UPSAMPLE_FWD, RS_UPSAMPLE_BWD, RS_MAXPOOL_FWD, RS_MAXPOOL_BWD, RS_REFLECT_FOLD, RS_ACT_PATTERN = 0, 1, 2, 3, 4, 5


def _dev(ctx, t, dtype=torch.float32):
    return None if t is None else t.detach().to(device=ctx.device, dtype=dtype).contiguous()


def _lead_pad(views, names):
    """{name: (lead_c, pad_c)} -> the flat int array of the swn_op_* view entry points, and the pairs."""
    views = views or {}
    unknown = set(views) - set(names)
    if unknown:
        raise ValueError("unknown operand(s) %s (have %s)" % (sorted(unknown), list(names)))
    pairs = [tuple(int(v) for v in views.get(k, (0, 0))) for k in names]
    return (C.c_int * (2 * len(names)))(*[v for p in pairs for v in p]), dict(zip(names, pairs))


def op_norm_act(ctx, x, dy=None, residual=None, norm=True, act=0, drop_p=0.0, seed=0, seed_on_device=False, salt=0,
                partial_in=None, views=None, want_colsum=1, stats_in=None):
    """norm_act_fwd (+ norm_act_bwd when dy is given) alone through swn_op_norm_act, every operand a channel-slice view of a
    sentinel-filled buffer: views = {"x" | "y" | "dy" | "dx" | "residual": (lead_c, pad_c)}.  partial_in: (N, chunks, C, 2) float64.
    Returns a dict: y, stats (N,C,2), y_slot (256), y_buf (the whole y buffer, N x (lead + C + pad) x H x W) and, with dy: dx, dx_slot,
    dx_buf, colsum_emitted, colsum (N,C float64) and db (C) when emitted.  stats_in (N,C,2): the backward pass ALONE on these statistics."""
    xd, dyd, rd = _dev(ctx, x), _dev(ctx, dy), _dev(ctx, residual)
    n, c, h, w = xd.shape
    lp, pairs = _lead_pad(views, ("x", "y", "dy", "dx", "residual"))
    f32 = dict(dtype=torch.float32, device=ctx.device)
    pin = _dev(ctx, partial_in, torch.float64)
    chunks = 0
    if pin is not None:
        if pin.dim() != 4 or pin.shape[0] != n or pin.shape[2] != c or pin.shape[3] != 2:
            raise ValueError("partial_in must be (N, chunks, C, 2)")
        chunks = pin.shape[1]
    r = {"y": torch.empty((n, c, h, w), **f32), "stats": torch.empty((n, c, 2), **f32) if norm else None,
         "y_slot": torch.empty(AMAX_SLOT, **f32), "y_buf": torch.empty((n, sum(pairs["y"]) + c, h, w), **f32),
         "dx": None, "dx_slot": None, "dx_buf": None, "colsum": None, "db": None, "colsum_emitted": False}
    if dyd is not None:
        r.update(dx=torch.empty((n, c, h, w), **f32), dx_slot=torch.empty(AMAX_SLOT, **f32),
                 dx_buf=torch.empty((n, sum(pairs["dx"]) + c, h, w), **f32),
                 colsum=torch.empty((n, c), dtype=torch.float64, device=ctx.device), db=torch.empty(c, **f32))
    if stats_in is not None:
        r.update(y=None, y_slot=None, y_buf=None, stats=_dev(ctx, stats_in))
    emitted = C.c_int(0)
    ctx.lib.call("swn_op_norm_act", ctx.handle, _C.ptr(xd), _C.ptr(dyd), _C.ptr(rd), n, c, h, w, int(bool(norm)), int(act),
                 C.c_float(drop_p), C.c_uint64(seed), int(bool(seed_on_device)), C.c_uint64(salt), _C.ptr(pin), int(chunks), lp,
                 int(want_colsum) if dyd is not None else 0, _C.ptr(r["y"]), _C.ptr(r["stats"]), _C.ptr(r["y_slot"]), _C.ptr(r["dx"]),
                 _C.ptr(r["dx_slot"]), _C.ptr(r["colsum"]), C.byref(emitted), _C.ptr(r["db"]), _C.ptr(r["y_buf"]), _C.ptr(r["dx_buf"]))
    r["colsum_emitted"] = bool(emitted.value)
    if not r["colsum_emitted"]:
        r["colsum"] = r["db"] = None
    return r


def op_elementwise(ctx, op, a, b=None, act=0, accumulate=False, alpha=1.0, shift=0.0, old=None, views=None):
    """act_fwd / act_bwd (a = dy, b = y) / axpy (a = src) alone through swn_op_elementwise on views = {"a" | "b" | "out": (lead_c,
    pad_c)}; `old`: the incoming contents of the destination (accumulate).  Returns (out, slot[256], the whole destination buffer)."""
    ad, bd = _dev(ctx, a), _dev(ctx, b)
    n, c, h, w = ad.shape
    lp, pairs = _lead_pad(views, ("a", "b", "out"))
    out = _dev(ctx, old).clone() if accumulate else torch.empty_like(ad)
    slot = torch.empty(AMAX_SLOT, dtype=torch.float32, device=ctx.device)
    buf = torch.empty((n, sum(pairs["out"]) + c, h, w), dtype=torch.float32, device=ctx.device)
    ctx.lib.call("swn_op_elementwise", ctx.handle, int(op), _C.ptr(ad), _C.ptr(bd), n, c, h, w, int(act), int(bool(accumulate)),
                 C.c_float(alpha), C.c_float(shift), lp, _C.ptr(out), _C.ptr(slot), _C.ptr(buf))
    return out, slot, buf


def op_resample(ctx, op, a, b=None, factor=2, accumulate=False, old=None, views=None, want_pattern=True):
    """One resampling launcher alone through swn_op_resample (RS_*; include/swapnet_hip.h gives the shapes) on views = {"a" | "b" |
    "out": (lead_c, pad_c)}.  Returns (out, slot[256] or None, pattern (uint8) or None, the whole destination buffer)."""
    ad, bd = _dev(ctx, a), _dev(ctx, b)
    n, c, h, w = ad.shape
    lp, pairs = _lead_pad(views, ("a", "b", "out"))
    f = int(factor)
    ho, wo = {RS_UPSAMPLE_FWD: (h * f, w * f), RS_UPSAMPLE_BWD: (h // max(f, 1), w // max(f, 1)), RS_MAXPOOL_FWD: (h // 2, w // 2),
              RS_MAXPOOL_BWD: (h, w), RS_REFLECT_FOLD: (h - 2, w - 2), RS_ACT_PATTERN: (h, w)}[op]
    f32 = dict(dtype=torch.float32, device=ctx.device)
    out = slot = pat = buf = None
    if op != RS_ACT_PATTERN:
        out = _dev(ctx, old).clone() if accumulate else torch.empty((n, c, max(ho, 0), max(wo, 0)), **f32)
        assert tuple(out.shape) == (n, c, max(ho, 0), max(wo, 0))
        buf = torch.empty((n, sum(pairs["out"]) + c, max(ho, 0), max(wo, 0)), **f32)
    if op in (RS_UPSAMPLE_FWD, RS_MAXPOOL_FWD):
        slot = torch.empty(AMAX_SLOT, **f32)
    if op == RS_ACT_PATTERN or (want_pattern and op in (RS_MAXPOOL_FWD, RS_MAXPOOL_BWD)):
        pat = torch.empty((n, c, h, w) if op == RS_ACT_PATTERN else (n, c, h // 2, w // 2), dtype=torch.uint8, device=ctx.device)
    ctx.lib.call("swn_op_resample", ctx.handle, int(op), _C.ptr(ad), _C.ptr(bd), n, c, h, w, f, int(bool(accumulate)), lp,
                 _C.ptr(out), _C.ptr(slot), _C.ptr(pat), _C.ptr(buf))
    return out, slot, pat, buf


def conv_out_hw(kind, transposed, h, w):
    """Output map of a conv kind (include/swapnet_hip.h swn_op_conv) on an h x w input."""
    if transposed or kind == 4:
        return 2 * h, 2 * w
    return {0: (h // 2, w // 2), 2: (h - 1, w - 1)}.get(kind, (h, w))


def op_conv_views(ctx, kind, transposed, what, x, wgt, dy=None, bias=None, act=0, naive=False, views=None, cimap=None, x_is_input=False,
                  dgrad_C=0, operand_slots=False, dx_old=None, pre_range=None, want_slot=False):
    """One convolution on views through swn_op_conv_views (include/swapnet_hip.h): views = {"x" | "y": (lead_c, pad_c, n_lead, n_pad)}.
    x (N, Ci, H, W) and wgt are the LOGICAL tensors ((Co, Ci, k, k); transposed (Ci, Co, 4, 4)); x is the forward input (what 0 / 1,
    and what 2 behind a fused activation; zeros will do where the call does not read it), dy the gradient of the (activated) output
    for what 1 / 2.  cimap: one entry per view channel of x (-1 = layout pad).  operand_slots: x and dy get external amax slots (the
    routes of a training step).  dx_old: the gradient x.g holds already (what 2; the planner then accumulates).  pre_range = (c0, c):
    a further channel range of x's parent gradient buffer announced to the planner as existing.
    Returns a dict: "out" (y / dW / dX), "y_fwd" (backward calls behind an activation), "y_slot" (want_slot), "dw_rows" (what 1: all
    packed rows), and the four whole parent buffers "x_buf", "xg_buf", "y_buf", "yg_buf"."""
    f32 = dict(dtype=torch.float32, device=ctx.device)
    wd = _dev(ctx, wgt)
    co = wd.shape[1] if transposed else wd.shape[0]
    ci = wd.shape[0] if transposed else wd.shape[1]
    k = wd.shape[2]
    n, h, w = x.shape[0], x.shape[2], x.shape[3]          # (x gives the input shape: zeros will do where the call does not read it)
    if x.shape[1] != ci:
        raise ValueError("op_conv_views: x has %d channels, the weights %d" % (x.shape[1], ci))
    ho, wo = conv_out_hw(kind, transposed, h, w)
    names = ("x", "y")
    views = views or {}
    if set(views) - set(names):
        raise ValueError("unknown operand(s) %s (have %s)" % (sorted(set(views) - set(names)), list(names)))
    geo = {k_: tuple(int(v) for v in views.get(k_, (0, 0, 0, 0))) for k_ in names}
    va = (C.c_int * 8)(*(geo["x"] + geo["y"]))
    cm, cv = None, -(-ci // 4) * 4
    if cimap is not None:
        cv = len(cimap)
        cm = (C.c_int32 * cv)(*[int(v) for v in cimap])
    cov = -(-co // 4) * 4
    xd = _dev(ctx, x).clone()
    bd = _dev(ctx, bias)
    fwd_first = what != 0 and act != 0
    if what == 0:
        yd = torch.empty((n, co, ho, wo), **f32)
    else:
        yd = _dev(ctx, dy).clone()
        if tuple(yd.shape) != (n, co, ho, wo):
            raise ValueError("op_conv_views: dy must be %s, got %s" % ((n, co, ho, wo), tuple(yd.shape)))
    if what == 1:
        wd = wd.clone()
    old = _dev(ctx, dx_old)
    pr = (C.c_int * 2)(*[int(v) for v in pre_range]) if pre_range is not None else None

    def whole(g, c, hh, ww):
        return torch.empty((g[2] + n + g[3], g[0] + c + g[1], hh, ww), **f32)
    r = {"y_fwd": torch.empty((n, co, ho, wo), **f32) if fwd_first else None,
         "y_slot": torch.empty(AMAX_SLOT, **f32) if want_slot else None,
         "dw_rows": torch.empty((cv, co, 4, 4) if transposed else (co, cv, k, k), **f32) if what == 1 else None,
         "x_buf": whole(geo["x"], cv, h, w), "xg_buf": whole(geo["x"], cv, h, w),
         "y_buf": whole(geo["y"], cov, ho, wo), "yg_buf": whole(geo["y"], cov, ho, wo)}
    ctx.lib.call("swn_op_conv_views", ctx.handle, int(kind), int(bool(transposed)), int(what), int(bool(naive)), _C.ptr(xd), n, ci, h, w,
                 _C.ptr(wd), co, _C.ptr(bd), int(act), _C.ptr(yd), va, cm, cv if cm is not None else 0, int(bool(x_is_input)), int(dgrad_C),
                 int(bool(operand_slots)), _C.ptr(old), pr, _C.ptr(r["y_fwd"]), _C.ptr(r["y_slot"]), _C.ptr(r["dw_rows"]), _C.ptr(r["x_buf"]), _C.ptr(r["xg_buf"]),
                 _C.ptr(r["y_buf"]), _C.ptr(r["yg_buf"]))
    r["out"] = {0: yd, 1: wd, 2: xd}[what]
    return r


def _warp_maps(maps, b, cloth_channels):
    """The map table of a warp batch as a (b * cloth_channels, nmaps, 9) float64 tensor and nmaps; (None, 0) without augmentation."""
    if maps is None:
        return None, 0
    maps = torch.as_tensor(maps)
    if maps.numel() == 0:
        return None, 0
    if maps.dim() != 4 or tuple(maps.shape[:2]) != (b, cloth_channels) or maps.shape[3] != 9:
        raise ValueError("warp batch: maps must be (B, cloth_channels, nmaps, 9) = (%d, %d, nmaps, 9), got %s"
                         % (b, cloth_channels, tuple(maps.shape)))
    return maps.to(torch.float64).reshape(b * cloth_channels, maps.shape[2], 9).contiguous(), int(maps.shape[2])


def warp_batch_bicubic(batch):
    """Whether a compact warp batch asks for the bicubic perspective ("perspective_resample", absent: "nearest")."""
    choice = batch.get("perspective_resample", "nearest")
    if choice not in ("nearest", "bicubic"):
        raise ValueError("warp batch: perspective_resample must be 'nearest' or 'bicubic', got %r" % (choice,))
    return choice == "bicubic"


def _check_warp_kinds(maps, bicubic):
    """Before any launch: kind 3 needs the bicubic instantiation, which evaluates one such row per chain."""
    if maps is None:
        return
    n3 = (maps[..., 0] == 3).sum(dim=-1)
    if int(n3.max()) > 1:
        raise ValueError("warp batch: at most one bicubic perspective row (kind 3) per chain, found %d" % int(n3.max()))
    if int(n3.max()) and not bicubic:
        raise ValueError("warp batch: the map table holds kind 3 (bicubic perspective) but the batch is not a bicubic one")


def _check_warp_batch(body, lab, tgt):
    if body.dim() != 4 or lab.dim() != 3 or (tgt is not None and tgt.dim() != 3):
        raise ValueError("warp batch: bodys_u8 (B,Hb,Wb,Cb), input_labels_u8 and target_labels_u8 (B,Hl,Wl)")
    if body.shape[3] != 3:
        raise ValueError("warp batch: the body is an RGB image (B,Hb,Wb,3), got %d channels" % body.shape[3])
    if lab.shape[0] != body.shape[0] or (tgt is not None and tuple(tgt.shape) != tuple(lab.shape)):
        raise ValueError("warp batch: the label maps must share one (B,Hl,Wl) and the bodies' batch size")


def op_warp_batch(ctx, bodys_u8, input_labels_u8, target_labels_u8, maps, mean, std, load_size, x_min, y_min, height, width,
                  cloth_channels=19, bicubic=False):
    """WarpDataset.__getitem__ for a batch through swn_op_warp_batch: (bodys, input_cloths, target_cloths) on the context's device,
    NCHW float32, from uint8 HWC body images (B,Hb,Wb,3), uint8 label maps (B,Hl,Wl) and the (B, cloth_channels, nmaps, 9) map
    table (None: no augmentation).  target_labels_u8 None: no targets (target_cloths is None).  bicubic: the table may hold kind 3
    (swn_op_warp_batch_ex, flags bit 0); off, the call is swn_op_warp_batch as it always was."""
    u8 = lambda t: torch.as_tensor(t).to(device=ctx.device, dtype=torch.uint8).contiguous()
    body, lab = u8(bodys_u8), u8(input_labels_u8)
    tgt = None if target_labels_u8 is None else (lab if target_labels_u8 is input_labels_u8 else u8(target_labels_u8))
    _check_warp_batch(body, lab, tgt)
    b = body.shape[0]
    maps, nmaps = _warp_maps(maps, b, cloth_channels)
    _check_warp_kinds(maps, bicubic)
    md = None if maps is None else maps.to(ctx.device)
    bodys = torch.empty((b, 3, height, width), dtype=torch.float32, device=ctx.device)
    inputs = torch.empty((b, cloth_channels, height, width), dtype=torch.float32, device=ctx.device)
    targets = None if tgt is None else torch.empty_like(inputs)
    if ctx.owns_stream:                     # (the uploads above ran on torch's stream)
        torch.cuda.current_stream(ctx.device).synchronize()
    args = (ctx.handle, _C.ptr(body), b, body.shape[1], body.shape[2], _C.ptr(lab),
            _C.ptr(tgt) if tgt is not None else None, lab.shape[1], lab.shape[2], _C.ptr(md) if md is not None else None, nmaps,
            (C.c_float * 3)(*mean), (C.c_float * 3)(*std), int(load_size), int(x_min), int(y_min), int(height), int(width),
            int(cloth_channels), _C.ptr(bodys), _C.ptr(inputs), _C.ptr(targets) if targets is not None else None)
    if bicubic:
        ctx.lib.call("swn_op_warp_batch_ex", *args, 1)
    else:
        ctx.lib.call("swn_op_warp_batch", *args)
    return bodys, inputs, targets


def op_norm_act_bwd2(ctx, x, gy, u, act=1):
    """(uy, ax) of swn_op_norm_act_bwd2: the second-order step through act(InstanceNorm(x))."""
    d = [t.to(device=ctx.device, dtype=torch.float32).contiguous() for t in (x, gy, u)]
    uy, ax = torch.empty_like(d[0]), torch.empty_like(d[0])
    n, c, h, w = d[0].shape
    ctx.lib.call("swn_op_norm_act_bwd2", ctx.handle, _C.ptr(d[0]), _C.ptr(d[1]), _C.ptr(d[2]), n, c, h, w, int(act),
                 _C.ptr(uy), _C.ptr(ax))
    return uy, ax


def op_batch_norm_act_bwd2(ctx, x, gy, u, weight, bias, act=1):
    """(uy, ax, dweight) of swn_op_batch_norm_act_bwd2: the second-order step through act(BatchNorm2d(x)) in training mode."""
    d = [t.to(device=ctx.device, dtype=torch.float32).contiguous() for t in (x, gy, u, weight, bias)]
    uy, ax = torch.empty_like(d[0]), torch.empty_like(d[0])
    n, c, h, w = d[0].shape
    dw = torch.empty(c, dtype=torch.float32, device=ctx.device)
    ctx.lib.call("swn_op_batch_norm_act_bwd2", ctx.handle, _C.ptr(d[0]), _C.ptr(d[1]), _C.ptr(d[2]), _C.ptr(d[3]), _C.ptr(d[4]),
                 n, c, h, w, int(act), _C.ptr(uy), _C.ptr(ax), _C.ptr(dw))
    return uy, ax, dw


def op_norm_act_dropout(ctx, x, dy=None, norm=True, act=2, p=0.5, seed=0):
    """[InstanceNorm] -> activation -> Dropout(p), training mode, forward (+ backward when dy is given) through
    swn_op_norm_act_dropout.  Returns (y, mask, dx): mask holds the factor (0 or 1/(1-p)) both passes applied."""
    xd = x.to(device=ctx.device, dtype=torch.float32).contiguous()
    dyd = None if dy is None else dy.to(device=ctx.device, dtype=torch.float32).contiguous()
    y, mask = torch.empty_like(xd), torch.empty_like(xd)
    dx = None if dy is None else torch.empty_like(xd)
    n, c, h, w = xd.shape
    ctx.lib.call("swn_op_norm_act_dropout", ctx.handle, _C.ptr(xd), _C.ptr(dyd), n, c, h, w, int(norm), int(act),
                 C.c_float(p), C.c_uint64(seed), _C.ptr(y), _C.ptr(mask), _C.ptr(dx))
    return y, mask, dx


class _ArrayIface:
    def __init__(self, ptr, n, cuda, typestr="<f4"):
        d = dict(shape=(n,), typestr=typestr, data=(ptr, False), version=2 if cuda else 3)
        if cuda:
            self.__cuda_array_interface__ = d
        else:
            self.__array_interface__ = d


def _wrap_pointer(ptr, n, device, typestr="<f4"):
    if device.type == "cuda":
        return torch.as_tensor(_ArrayIface(ptr, n, True, typestr), device=device)
    import numpy as np
    return torch.from_numpy(np.asarray(_ArrayIface(ptr, n, False, typestr)))


class NativePipeline:
    """swn_pipeline handle: warp forward -> argmax labels -> one-hot -> texture forward on the device, optionally
    replayed as a hipGraph (see include/swapnet_hip.h)."""

    def __init__(self, warp_model, texture_model):
        self.warp, self.texture = warp_model, texture_model
        self.lib, self.ctx = warp_model.lib, warp_model.ctx
        h = C.c_void_p()
        self.lib.call("swn_pipeline_create", warp_model.handle, texture_model.handle, C.byref(h))
        self.handle = h

    def run(self, use_graph=True):
        """Returns True when the call was a graph replay (False: eager run, incl. the capturing first call)."""
        replayed = C.c_int()
        self.lib.call("swn_pipeline_run", self.handle, int(bool(use_graph)), C.byref(replayed))
        return bool(replayed.value)

    def labels(self):
        p = C.c_void_p()
        self.lib.call("swn_pipeline_labels", self.handle, C.byref(p))
        n = self.warp.B * self.warp.H * self.warp.W
        self.ctx.sync()
        return _wrap_pointer(p.value, n, self.ctx.device, "<i4").reshape(self.warp.B, self.warp.H, self.warp.W).clone()

    def enable_images(self, body_norm_stats, texture_norm_stats, colours, width, reference_quirk=True):
        """swn_pipeline_enable_images: from the next run on the sequence ends with the image launches (inside the captured graph);
        *_norm_stats = (mean3, std3) as the reference's options hold them, colours (num_roi, 3) uint8, width in pixels."""
        import numpy as np
        col = np.ascontiguousarray(np.asarray(colours, dtype=np.uint8))
        if col.shape != (self.texture.num_roi, 3):
            raise ValueError("enable_images: colours must be (num_roi, 3) = %s, got %s" % ((self.texture.num_roi, 3), col.shape))
        f3 = lambda v: (C.c_float * 3)(*[float(t) for t in v])
        (bm, bs), (tm, ts) = body_norm_stats, texture_norm_stats
        self.lib.call("swn_pipeline_enable_images", self.handle, f3(bm), f3(bs), f3(tm), f3(ts),
                      col.ctypes.data_as(C.POINTER(C.c_uint8)), int(width), int(bool(reference_quirk)))

    def images(self):
        """The image sheet of the last run in ONE device-to-host copy: name -> (B,H,W,3) uint8 numpy array (IMAGE_NAMES order)."""
        p, k = C.c_void_p(), C.c_int()
        self.lib.call("swn_pipeline_images", self.handle, C.byref(p), C.byref(k))
        B, H, W = self.warp.B, self.warp.H, self.warp.W
        self.ctx.sync()
        sheet = _wrap_pointer(p.value, k.value * B * H * W * 3, self.ctx.device, "|u1").cpu().numpy().reshape(k.value, B, H, W, 3)
        if self.ctx.device.type != "cuda":
            sheet = sheet.copy()
        return OrderedDict(zip(IMAGE_NAMES, sheet))

    def enable_png(self, rows_per_chunk=0):
        """swn_pipeline_enable_png: from the next run on the sequence also ends with the two PNG launches over the image sheet
        (inside the captured graph).  Needs enable_images first."""
        self.lib.call("swn_pipeline_enable_png", self.handle, int(rows_per_chunk))

    def png(self):
        """The sheet of the last run as PNG files: name -> list of B `bytes` (IMAGE_NAMES order).  Two device-to-host copies (the
        sizes, then the used part of the streams); the container around each stream is assembled here (util/png.py)."""
        from .util.png import png_container
        ps, pz, stride, k = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_int()
        self.lib.call("swn_pipeline_png", self.handle, C.byref(ps), C.byref(pz), C.byref(stride), C.byref(k))
        B, H, W = self.warp.B, self.warp.H, self.warp.W
        n = k.value * B
        self.ctx.sync()
        sizes = _wrap_pointer(pz.value, n, self.ctx.device, "<i4").cpu().tolist()
        used = _wrap_pointer(ps.value, n * stride.value, self.ctx.device, "|u1").reshape(n, stride.value)[:, :max(sizes)].cpu().numpy()
        files = [png_container(used[i, :sizes[i]].tobytes(), W, H) for i in range(n)]
        return OrderedDict((name, files[j * B:(j + 1) * B]) for j, name in enumerate(IMAGE_NAMES))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.call("swn_pipeline_destroy", self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def op_batch_norm_act_dropout(ctx, x, weight, bias, dy=None, act=0, p=0.5, seed=0):
    """BatchNorm2d -> [act] -> Dropout(p), training mode, forward (+ backward when dy is given) through
    swn_op_batch_norm_act_dropout.  Returns (y, mask, dx, dweight, dbias): mask holds the factor (0 or 1/(1-p)) both passes
    applied (None when p == 0)."""
    xd = _dev(ctx, x)
    dyd, wd, bd = _dev(ctx, dy), _dev(ctx, weight), _dev(ctx, bias)
    n, c, h, w = xd.shape
    y = torch.empty_like(xd)
    mask = torch.empty_like(xd) if p > 0 else None
    dx = None if dy is None else torch.empty_like(xd)
    dw = torch.empty(c, dtype=torch.float32, device=ctx.device) if dy is not None else None
    db = torch.empty_like(dw) if dw is not None else None
    ctx.lib.call("swn_op_batch_norm_act_dropout", ctx.handle, _C.ptr(xd), _C.ptr(dyd), n, c, h, w, int(act), C.c_float(p),
                 C.c_uint64(seed), _C.ptr(wd), _C.ptr(bd), _C.ptr(y), _C.ptr(mask), _C.ptr(dx), _C.ptr(dw), _C.ptr(db))
    return y, mask, dx, dw, db
