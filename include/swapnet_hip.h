/* swapnet_hip.h -- C ABI of libswapnet_hip.so, the MI355X (gfx950) back end of the SwapNet
 * two-stage GAN training hot path.
 *
 * The reference (andrewjong/SwapNet) has no native boundary of its own: it is pure Python
 * on torch.nn.  Each entry point below therefore cites the reference
 * *Python* interface it stands in for; swapnet_amd/_C.py is the ctypes binding and
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; swn_last_error() returns
 *     the message of the last failure on the calling thread (the Python shim re-raises it
 *     as the exception type the reference would raise: ValueError / NotImplementedError /
 *     RuntimeError).
 *   - all tensor arguments are raw DEVICE pointers to fp32 (NCHW, contiguous -- the layout
 *     of the reference's torch tensors) unless the name says host; the library borrows them
 *     for the duration of the call and never frees caller memory.
 *   - one context per process/GPU, driven by one host thread; all work is enqueued on the
 *     context's HIP stream.
 *   - arithmetic: storage and accumulation are fp32 throughout.  The large implicit-GEMM kernels form each fp32 product
 *     on the 16-bit matrix cores from a split of both operands into two fp16 planes, x * 2^k = h + l with k chosen per TENSOR
 *     from its amax: h + l carries 22 of fp32's 24 mantissa bits for every element within 2^-14 of the tensor's largest and
 *     progressively fewer below that (absolute floor amax * 2^-37), and three of the four partial products are formed (the
 *     dropped l*l term is < 2^-22 relative).  This is NOT an exact representation of fp32: it is held to the f32-MFMA
 *     kernels' error on well-conditioned and on heavy-tailed operands by tests/test_ops.py (rel-L2 and element-wise).
 *     Environment: SWN_PC_PLANES=3 / SWN_WGRAD_PLANES=3 (three bf16 planes by truncation -- that split IS exact, 24 bits
 *     in, 24 out -- six MFMAs, dropped terms < 2^-24), SWN_SPLIT=0 (v_mfma_f32_32x32x2_f32); DESIGN.md section 4.
 */
#ifndef SWAPNET_HIP_H
#define SWAPNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct swn_ctx swn_ctx;
typedef struct swn_model swn_model;

int swn_abi_version(void);   /* 2: swn_hyper gained d_b1, d_b2; 3: gp_mode, lambda_gp; 4: swn_route_*, swn_model_step_captured, swn_model_create_shared;
                                5: swn_ctx_attach_comm, swn_model_step_dp; 6: swn_probe_mfma; 7: swn_op_conv_produced, swn_slot_audit; 8: swn_op_loss, swn_op_bias_grad;
                                9: swn_op_norm_act, swn_op_elementwise, swn_op_resample (additions since, version unchanged: swn_op_resize_u8,
                                swn_model_set_input_texture_sources, swn_op_conv_views, swn_op_chain_resample, swn_op_warp_batch_ex,
                                swn_model_set_input_warp_batch_ex, swn_op_image_u8, swn_pipeline_enable_images, swn_pipeline_images; the PNG entry points
                                swn_op_png_encode, swn_png_stream_bound, swn_pipeline_enable_png, swn_pipeline_png were added within ABI 9 as well, and so were
                                the loss entry points swn_op_ssim, swn_op_charbonnier) */
const char* swn_last_error(void);
/* 1 when this library executes on a HIP device (libswapnet_hip.so), 0 for the CI simulator */
int swn_is_device_build(void);

/* ---- context ------------------------------------------------------------------------
 * replaces BaseModel.__init__'s device selection (models/base_model.py:36-40).
 * create_stream == 0: all work is enqueued on `hip_stream` exactly as given -- pass
 * torch.cuda.current_stream().cuda_stream so torch-side copies / allocator reuse stay ordered
 * with the library's kernels (NULL is the legacy default stream, which IS torch's default).
 * create_stream != 0: the library creates and owns a private non-blocking stream. */
int swn_ctx_create(int device, void* hip_stream, int create_stream, size_t workspace_bytes, swn_ctx** out);
int swn_ctx_destroy(swn_ctx* ctx);
/* The context runs weight-gradient work and the derived-weight refresh on an internal second stream
 * (DESIGN.md section 4).  on = 0 keeps everything in order on the caller's stream (used by bench.py's
 * per-kernel roofline pass so that kernel durations are not inflated by co-running kernels); results
 * are identical either way.  Synchronises. */
int swn_ctx_set_overlap(swn_ctx* ctx, int on);
/* discriminators.define_D(input_nc, 64, opt.discriminator, opt.n_layers_D, opt.norm) (modules/discriminators.py:45-88,
 * models/base_gan.py:147-149): the number of stride-2 levels of the NLayerDiscriminator (:91-136) of every model created on
 * this context AFTERWARDS; 3 = "basic", the 70x70 PatchGAN (default).  1..5; the input must keep >= 3 pixels per side after
 * the stride-2 levels.  0 = --discriminator pixel: the 1x1 PixelDiscriminator (:139-170; three 1x1 convs, a prediction per
 * pixel, state_dict keys net.{0,2,5}.{weight,bias}).  The gradient-penalty modes exist for every PatchGAN depth, not for the
 * PixelDiscriminator (swn_model_set_hyper fails). */
int swn_ctx_set_patchgan_layers(swn_ctx* ctx, int n_layers);
/* discriminators.define_D(..., norm) -> get_norm_layer(norm) (modules/discriminators.py:77, modules/__init__.py:53-74;
 * models/base_gan.py:72-77,147-149): --norm for every model created on this context AFTERWARDS -- the norm layer of the warp
 * stage's discriminator, of the texture stage's discriminator, and of the TextureModule's pix2pix U-Net
 * (modules/swapnet_modules.py:176-187; its `encode` branch keeps InstanceNorm, and the warp generator hard-codes it).
 * 0 = instance (default), 1 = batch (nn.BatchNorm2d, affine, running statistics), 2 = none (identity).
 * Under 1 and 2 the convs in front of a norm layer carry no bias (use_bias is true only under InstanceNorm2d,
 * modules/discriminators.py:104-107,151-154): the state dict has no model.{2,5,8}.bias / net.2.bias.  Under 1 every norm site
 * adds model.K.weight / model.K.bias (K = 3, 6, ...; net.3 for the PixelDiscriminator) to the discriminator's parameters -- the
 * optimizer, weight decay and the gradient exchange cover them like any parameter -- and the buffers model.K.running_mean /
 * .running_var / .num_batches_tracked (swn_model_buffer_* below).  A training step updates the running statistics three
 * times, as the reference's three discriminator calls do (models/warp_model.py:115-121,157-158): fake batch, real batch -- the
 * two halves of the one 2B pass, normalised separately -- then the fakes through the updated discriminator.  Under data
 * parallelism the statistics stay local to each rank (torch DDP's default).
 * The TextureModule's U-Net under 1 and 2: no conv carries a bias but the outermost ConvTranspose2d; under 1 every down-norm
 * (<block>.model.2) and up-norm (<block>.model.6, innermost .model.4) is a BatchNorm site of net 0 with weight, bias and running
 * buffers, the upnorm -> Dropout sites fused as in unet_128; an inference model (and swn_pipeline's second stage) normalises with
 * the running buffers.  The unet_128 generator (swn_texture_model_create_netG) ignores the flag -- BatchNorm2d whatever it
 * says -- and its discriminator follows it.
 * A gradient-penalty step (warp stage) under kind 1 updates the running statistics four times: fake, real, the interpolate x_hat
 * (the reference calls the module in train mode, modules/loss.py:157-162), then the generator pass's fakes; the second-order pass
 * walks BatchNorm with swn_op_batch_norm_act_bwd2's kernels and, under kind 2, conv -> LeakyReLU alone.
 * Device library only: on the CI simulator (no BatchNorm kernels) kind 1, texture models under kind != 0 and the gradient-penalty
 * modes under kind != 0 answer with the library's "not implemented" error.  Synchronised statistics across ranks: not implemented. */
int swn_ctx_set_patchgan_norm(swn_ctx* ctx, int kind);
int swn_ctx_sync(swn_ctx* ctx);
int swn_ctx_bytes_allocated(swn_ctx* ctx, size_t* out);

/* per-launch timing of the implicit-GEMM kernels with HIP events on the context's stream
 * (bench.py's roofline leg).  report: one line per kernel variant "<name> <launches> <total_ms>
 * <total_flops>"; returns the number of bytes the full report needs. */
int swn_prof_enable(int on);
int swn_prof_reset(void);
int swn_prof_report(char* buf, int len);
/* What the matrix pipe of THIS chip sustains for the arithmetic of the ring kernels ("Builder must confirm peaks on
 * the box"; bench.py's roofline object quotes it beside the nominal 2.5 PFLOP/s): `iters` rounds of the product loop's twelve
 * v_mfma_f32_32x32x16_f16 per wave (4 accumulators x 3 terms) on operand fragments that stay in registers -- no LDS, no HBM --
 * 1024 workgroups x 4 waves, zeros = 0: pseudo-random fp16 operands (what a training step multiplies), 1: all-zero operands (the
 * clock the same code gets when the multipliers do not toggle).  out[0] = fp16 TFLOP/s, out[1] = the shader clock in GHz measured
 * INSIDE the kernel (s_memtime over s_memrealtime), out[2] = ms per launch, out[3] = matrix-pipe occupancy at that clock (0..1).
 * Replaces nothing in the reference (measurement only); synchronises. */
int swn_probe_mfma(swn_ctx* ctx, int zeros, int iters, float* out4);
/* Routing trace: which kernel family / algorithmic form each layer takes under the CURRENT environment (the SWN_* switches of
 * DESIGN.md section 4 select among kernels; models/base_gan.py:194-203 is the step whose launches are listed).  While on, every
 * implicit-GEMM launch (name, M, N, K, batch, split schedule) and every Winograd transform is recorded against the layer
 * (state_dict prefix) and phase (f forward, b backward, r operand refresh) that issued it; report = the distinct lines in
 * first-use order, returns the bytes the full report needs.  tests/ compare the list of a scrubbed-environment run (what
 * bench.py times) with the list of the run they check against the oracle. */
int swn_route_trace(int on);
int swn_route_report(char* buf, int len);
/* Slot audit (diagnostic, no reference counterpart; off by default).  The GEMMs scale their fp16 operand planes by a power of two
 * that usually comes from an "amax slot" the operand's producer filled, and the Winograd transforms cut their planes with a scale
 * derived from such a slot and a gain bound.  While on, every launch that trusts a slot -- the convolution
 * launches and the pair-form Winograd transforms -- also takes max |v| of exactly what it gathers, reads both back and fails
 * (the call that issued the launch returns non-zero; swn_last_error names the launch, the slot value and the operand's amax) unless
 * amax <= slot <= 4096 * amax; a pair-form transform additionally must leave |plane| * 2^k < 65504.  These are the conditions the CI
 * simulator always checks on its own bookkeeping: there the call does nothing and succeeds.  Every audited launch synchronises, so
 * a launch issued while a stream capture is open fails; swn_model_step_captured and swn_pipeline_run(use_graph) run unaudited. */
int swn_slot_audit(int on);

/* ---- models ---------------------------------------------------------------------------
 * swn_warp_model_create    <-> models.create_model(opt) with --model warp
 *                              (models/__init__.py:33-44, models/warp_model.py:42-76,
 *                               models/base_gan.py:130-176): WarpModule generator and, when
 *                               is_train, the 22-channel conditional PatchGAN + both AdamW states.
 * swn_texture_model_create <-> --model texture (models/texture_model.py:54-111): TextureModule
 *                              generator (RoIAlign -> UNetDown -> pix2pix U-Net), PatchGAN,
 *                              VGG16 perceptual network. */
int swn_warp_model_create(swn_ctx* ctx, int batch, int height, int width, int is_train, float dropout,
                          swn_model** out);
int swn_texture_model_create(swn_ctx* ctx, int batch, int height, int width, int is_train, int num_roi,
                             swn_model** out);
/* The same with the reference's representation options (options/base_options.py:75-105, models/warp_model.py:49-55,
 * models/texture_model.py:94-109): body_channels = 3 for --body_representation rgb, --body_channels (12) for labels;
 * cloth_channels = --cloth_channels (19) for --cloth_representation labels, 3 for rgb.  The plain constructors above
 * are the defaults (3, 19).  swn_model_destroy releases every device buffer the model allocated. */
int swn_warp_model_create_ex(swn_ctx* ctx, int batch, int height, int width, int is_train, float dropout,
                             int body_channels, int cloth_channels, swn_model** out);
int swn_texture_model_create_ex(swn_ctx* ctx, int batch, int height, int width, int is_train, int num_roi,
                                int cloth_channels, swn_model** out);
/* The texture model with the reference's --netG choice (models/texture_model.py define_G).  netG 0 = swapnet, the ROI-pooled
 * TextureModule: identical to swn_texture_model_create_ex.  netG 1 = unet_128, the plain pix2pix U-Net baseline (Isola et al.
 * 2017) UnetGenerator(3, 3, num_downs 7, ngf 64, BatchNorm2d, use_dropout = True) called on the input textures alone: no ROIs and
 * no cloth input reach the generator (slots 1 and 2 are still staged; the cloths condition the discriminator), against the same
 * PatchGAN and losses.  Its state dict (net 0) has the prefix `model`: 15 conv tensors (no conv carries a bias except the outermost
 * ConvTranspose2d, model.model.3.bias), weight / bias of 11 BatchNorm sites as parameters and their running_mean / running_var /
 * num_batches_tracked as buffers (swn_model_buffer_*), 70 keys.  Dropout(0.5) follows the upnorm of the two inner ngf*8 blocks.
 * swn_model_forward(training): batch statistics, one running update per call and dropout -- or, training = 0, the running
 * buffers, nothing updated, no dropout; a backward pass through an eval-mode forward is refused.  Under data parallelism the
 * statistics stay local to each rank, as the discriminator's do.  height = width in {128, 256}.
 * Not implemented: netG 1 on the CI simulator (HIP kernels only), and as the texture stage of swn_pipeline_create. */
int swn_texture_model_create_netG(swn_ctx* ctx, int batch, int height, int width, int is_train, int num_roi,
                                  int cloth_channels, int netG, swn_model** out);
/* A second model on the SAME training state: it uses `sharer`'s parameter arenas (weights, gradients, both Adam moments, step
 * counters -- per network one flat buffer each) and owns only its activations and derived operands.  For the reference's loops
 * that is the model of another batch size: the last, smaller batch of an epoch (train.py:62-64 with drop_last off) or the batch-1
 * pass of inference.py:67 beside a training model -- without a second copy of the state and without copying it back and forth.
 * Same kind, channel options and PatchGAN depth as the sharer; hyper-parameters are copied at creation (set them on both
 * afterwards).  The sharer's buffers live until the last sharing model is destroyed, whatever the order of swn_model_destroy. */
int swn_model_create_shared(swn_model* sharer, int batch, int height, int width, swn_model** out);
int swn_model_destroy(swn_model* m);

/* hyper-parameters = the opt.* fields read by the step (models/base_gan.py:87-120,
 * optimizers/__init__.py:25-59, models/warp_model.py:27-34, models/texture_model.py:31-50) */
typedef struct swn_hyper {
  float lr, d_lr, weight_decay, d_weight_decay, b1, b2;
  float lambda_gan, lambda_ce, lambda_l1, lambda_content, lambda_style;
  int gan_mode;      /* 0 vanilla, 1 lsgan, 2 wgan */
  int warp_mode_ce;  /* 1 = --warp_mode ce (generator only) */
  float grad_scale;  /* multiplies every loss gradient: 1/world_size under data parallelism so the
                        RCCL all-reduce(SUM) of the arenas yields the mean without an extra pass */
  float d_b1, d_b2;  /* AdamW betas of optimizer_D (negative = same as b1 / b2; 0 is a valid beta): the two torch optimizers of the
                        reference are independent objects (models/base_gan.py:87-120) */
  int gp_mode;       /* gradient penalty of --gan_mode (modules/loss.py:133-184): 0 none, 1 wgan-gp (with gan_mode 2),
                        2 dragan-gp, 3 dragan-lp (with gan_mode 0); warp model only */
  float lambda_gp;   /* --lambda_gp (models/base_gan.py:54-58) */
} swn_hyper;
int swn_model_set_hyper(swn_model* m, const swn_hyper* h);

/* parameters: net 0 = generator, 1 = discriminator, 2 = VGG16 features (texture model).
 * Names and shapes are the reference's state_dict() keys (SURVEY.md 8(b) "Checkpoint
 * format").  which: 0 weight, 1 grad, 2 exp_avg, 3 exp_avg_sq (torch.optim.AdamW state). */
int swn_model_param_count(swn_model* m, int net, int* out);
int swn_model_param_info(swn_model* m, int net, int index, char* name, int name_len, int shape[4], int* ndim);
int swn_model_param_set(swn_model* m, int net, int which, const char* name, const float* dev_src);
int swn_model_param_get(swn_model* m, int net, int which, const char* name, float* dev_dst);
int swn_model_optim_step_get(swn_model* m, int net, int* step);   /* AdamW `step` counter */
int swn_model_optim_step_set(swn_model* m, int net, int step);
/* The optimizer of one network, optimizers.define_optimizer's choice (optimizers/__init__.py:37-60): kind 0 = AdamW (the default
 * of every model), 1 = AdaBound (Luo et al., ICLR 2019, as adabound 0.0.5 executes it with amsbound off and eps 1e-8).  AdaBound
 * reads lr, betas and weight decay from swn_hyper like AdamW -- the decay as a COUPLED L2 term, g += wd * p -- and clamps the
 * per-element rate lr * sqrt(1 - b2^t) / (1 - b1^t) / (sqrt(v) + eps) to final * [1 - 1/(gamma t + 1), 1 + 1/(gamma t)],
 * final = final_lr * lr / base_lr; base_lr = the lr the optimizer was constructed with (> 0), gamma > 0 (package default 1e-3).
 * The three values are ignored for kind 0.  Moments and the step counter are kept (which 2 / 3, swn_model_optim_step_*).  Models
 * sharing the arenas share the choice.  Drops the model's recorded step graphs when anything changes.  HIP library only: the
 * CI simulator refuses kind 1. */
int swn_model_set_optimizer(swn_model* m, int net, int kind, float final_lr, float base_lr, float gamma);

/* BaseModel.set_input (models/warp_model.py:99-104, models/texture_model.py:113-119).
 * warp slots: 0 bodys (B,3,H,W), 1 input_cloths (B,19,H,W), 2 target_cloths (B,19,H,W)
 * texture slots: 0 input_textures (B,3,H,W), 1 rois (B,R,4 as N=B,C=R,H=4,W=1), 2 cloths
 * (B,19,H,W), 3 target_textures (B,3,H,W) */
int swn_model_set_input(swn_model* m, int slot, const float* dev_nchw, int n, int c, int h, int w);
/* Same slots, but for the cloth segmentations (warp 1, 2; texture 2) the caller hands over the
 * integer label map (B,H,W) int32 -- the on-disk format, datasets/data_utils.py:298-343 -- and the
 * one-hot expansion (label 0 -> all-zero vector) happens on the device: 1/19 of the H2D bytes of
 * set_input(one_hot).  Bit-identical to to_onehot_tensor + set_input. */
int swn_model_set_input_labels(swn_model* m, int slot, const int32_t* dev_labels, int n, int h, int w);
/* Texture models: all four slots of a step from the COMPACT batch, one device launch (swn_op_texture_batch below has the
 * arithmetic): img (B,hs,ws,3) uint8 = the samples after tf.resize(img, load_size), labels (B,hl,wl) uint8 = the cloth label maps as
 * stored, rois_raw (B,R,4) float32 = the ROI table's rows, sample (B,5) float32 = {vflip, hflip, roi_scale, cy, cx} per sample --
 * all device pointers; mean3 / std3 = the texture statistics, HOST floats.  The crop window is the model's H x W at (x_min, y_min)
 * of the hs x ws source.  Writes slot 0 (input_textures), 1 (rois), 2 (cloths) and, when training, 3 (target_textures),
 * bit-identically to swn_model_set_input on the tensors TextureDataset.__getitem__ builds (datasets/texture_dataset.py:87-160).
 * An inference model has no target: nothing of it is written. */
int swn_model_set_input_texture_batch(swn_model* m, const uint8_t* img, int b, int hs, int ws, const uint8_t* labels, int hl, int wl,
                                      const float* rois_raw, int r, const float* sample, const float* mean3, const float* std3,
                                      int x_min, int y_min);
/* Texture models: the same from the DECODED images, each at its own size -- the tf.resize(img, load_size) of
 * datasets/texture_dataset.py:93-95,132-134 moves into the library.  src = packed device bytes, src_bytes of them; geom_host = HOST
 * (b,3) int64 rows {byte offset, H0, W0}: sample i is the (H0, W0, 3) uint8 image at src + offset.  Two launches: swn_op_resize_u8
 * (below: Pillow's bilinear resize, byte for byte) into a (b, hs, ws, 3) buffer the model owns -- allocated when the model is first
 * used this way, again only if a later call needs a larger one -- then the launch of swn_model_set_input_texture_batch on that
 * buffer with the remaining arguments unchanged, whose bit-exactness this path inherits.  Every argument of both launches is
 * checked before the first goes out; the call allocates nothing in steady state and never synchronises. */
int swn_model_set_input_texture_sources(swn_model* m, const uint8_t* src, size_t src_bytes, const int64_t* geom_host, int b, int hs, int ws,
                                        const uint8_t* labels, int hl, int wl, const float* rois_raw, int r, const float* sample,
                                        const float* mean3, const float* std3, int x_min, int y_min);
/* Warp models: everything swn_model_set_input writes for slots 0 (bodys), 1 (input_cloths) and, when training, 2 (target_cloths) from
 * the COMPACT batch, one device launch (swn_op_warp_batch below has the arithmetic): body (B,hb,wb,3) uint8 = the decoded RGB images,
 * NOT resized; in_labels / tgt_labels (B,hl,wl) uint8 = the cloth label maps as stored (tgt_labels may be the same pointer as
 * in_labels: --dataset_mode image; NULL for an inference model, where nothing of a target is written); maps = doubles
 * [b * cloth_channels][nmaps][9], the table of swn_op_affine_gather (NULL or nmaps 0: no augmentation) -- all device pointers;
 * mean3 / std3 = the body statistics, HOST floats.  The crop window is the model's H x W at (x_min, y_min) of the load_size x load_size
 * resized sample.  Bit-identical to swn_model_set_input on the tensors WarpDataset.__getitem__ builds (datasets/warp_dataset.py:
 * 139-183) with the per-channel augmentation of swn_op_affine_gather, the operand amax slots included.  RGB bodies only. */
int swn_model_set_input_warp_batch(swn_model* m, const uint8_t* body, int b, int hb, int wb, const uint8_t* in_labels,
                                   const uint8_t* tgt_labels, int hl, int wl, const double* maps, int nmaps, const float* mean3,
                                   const float* std3, int load_size, int x_min, int y_min);
/* The same with a trailing `flags`.  Bit 0: the map table may hold kind 3, RandomPerspective resampled BICUBIC as torchvision 0.4.0
 * resamples it (datasets/__init__.py:87-110 get_transforms -> transforms.RandomPerspective, applied per channel by
 * datasets/data_utils.py:346-361; swn_op_chain_resample below has the rule) -- the input cloth is then a float map that need not be
 * 0 or 1, and its amax slot is measured after the launch like any other's.  flags 0 is swn_model_set_input_warp_batch itself: the
 * same launch, the same bytes.  PRECONDITION: at most one kind-3 row per chain; kind 3 only with bit 0 set.  Other bits: refused. */
int swn_model_set_input_warp_batch_ex(swn_model* m, const uint8_t* body, int b, int hb, int wb, const uint8_t* in_labels,
                                      const uint8_t* tgt_labels, int hl, int wl, const double* maps, int nmaps, const float* mean3,
                                      const float* std3, int load_size, int x_min, int y_min, int flags);
/* slot 0: self.fakes (B,19,H,W) warp / (B,3,H,W) texture */
int swn_model_get_output(swn_model* m, int slot, float* dev_nchw);
/* named intermediate activation (debug / per-level parity tests), copied out as NCHW.  Warp models, net 0, also name the buffers
 * filled from outside, pad channels included -- "body", "cloth", "Dx" (the conditional-D input [cloth | body], 2B images when
 * training) -- and their operand amax slots "slot_body", "slot_cloth", "slot_dx" as (1,256,1,1) */
int swn_model_get_tap(swn_model* m, int net, const char* name, float* dev_nchw, int shape[4]);

/* gradient w.r.t. a named activation as left by the last backward pass through `net` (diagnostics) */
int swn_model_get_tap_grad(swn_model* m, int net, const char* name, float* dev_nchw, int shape[4]);

/* nn.Dropout sites of the generator in forward order (WarpModule: body_down4, cloth_down5, cloth_down6 and the
 * four ResidualBlocks, modules/swapnet_modules.py:37,46-47,58 / modules/layers.py:22-23,136; pix2pix U-Net:
 * the three inner ngf*8 blocks, modules/pix2pix_modules.py:251-252; the unet_128 generator: the two inner ngf*8 blocks,
 * where the mask is applied by the BatchNorm apply pass).  swn_model_dropout_mask writes the factor
 * (0 or 1/(1-p)) that a training-mode forward AND backward with `dropout_seed` apply at `site`, as an NCHW
 * tensor of `shape` (channel count = the padded channel count of the layer).  dst may be NULL to query the
 * shape.  Diagnostic: lets a parity test replay the exact masks in the CPU oracle. */
int swn_model_dropout_sites(swn_model* m, int net, int* count);
/* Diagnostic export for parity tests: the branch every piecewise-linear op of the last pass took.  LeakyReLU / ReLU
 * (kind 1): byte 1 where the activation output is > 0, i.e. the side the backward pass differentiates on; MaxPool2d
 * (kind 2): the window position 2*kh + kw that receives the gradient.  NCHW bytes on the device, `shape` = (N,C,H,W)
 * with C the buffer's (possibly padded) channel count; dev_nchw = NULL only queries shape / kind.  Sites are numbered
 * in forward order per network: net 0 = generator, 1 = discriminator of the D step (samples [0,B) generated, [B,2B)
 * real), 2 = discriminator as re-evaluated inside the G step, 3 = VGG16 on the generated image (texture model).
 * Why: an fp32 pass in a different summation order leaves a handful of pre-activations on the other side of zero and
 * each flip moves the gradient by O(1) of that element (rel-L2 ~1e-3 on PatchGAN at 256x256, for torch's own fp32
 * backward as much as for this library); with the pattern replayed in the float64 oracle the comparison is ~1e-5. */
int swn_model_act_sites(swn_model* m, int net, int* count);
int swn_model_act_pattern(swn_model* m, int net, int site, uint8_t* dev_nchw, int shape[4], int* kind);
int swn_model_dropout_mask(swn_model* m, int net, int site, uint64_t dropout_seed, float* dev_nchw, int shape[4],
                           float* p);

/* inference.py's warp -> texture hand-off (inference.py:94-126; .npz round trip of :140-149,169-180 /
 * datasets/data_utils.py:311-343) kept in HBM: warp forward -> argmax label map -> one-hot into the texture model's
 * cloth inputs -> texture forward.  Inputs are staged with swn_model_set_input on the two models beforehand (warp
 * slots 0,1; texture slots 0,1 -- texture slot 2 is produced here); the result is the texture model's output.
 * A texture model created with netG = unet_128 is refused ("not implemented"): that generator has no cloth input to hand over.
 * use_graph != 0: the first call runs eagerly and captures the sequence into a hipGraph, later calls replay it
 * (*graph_replayed = 1).  Both models must be inference models (is_train = 0) of one context and one (B,H,W). */
typedef struct swn_pipeline swn_pipeline;
int swn_pipeline_create(swn_model* warp, swn_model* texture, swn_pipeline** out);
int swn_pipeline_destroy(swn_pipeline* p);
int swn_pipeline_run(swn_pipeline* p, int use_graph, int* graph_replayed);
int swn_pipeline_labels(swn_pipeline* p, int32_t** dev_labels);   /* (B,H,W) int32 of the last run, library-owned */
/* The images inference.py saves per sample (inference.py:94-126: get_current_visuals + save_images, i.e. datasets/data_utils.py:41-90
 * unnormalize / scale_tensor(scale_each), util/decode_labels.py:24-55, util/draw_rois.py:16-47, util/util.py:9-32 tensor2im) produced
 * on the device as the tail of the sequence -- seven launches of swn_op_image_u8's kernels, INSIDE the captured graph -- instead
 * of fp32 read-backs and host loops.  body_* / tex_* = --body_norm_stats / --texture_norm_stats, colours = (num_roi, 3) outline bytes,
 * all HOST arrays; width = outline width in pixels (util/draw_rois.py:41: int(round(0.01 * W))).  reference_quirk != 0 reproduces
 * unnormalize's zip over dim 0 (see swn_op_image_u8), 0 un-normalises every image per channel.  All images use tensor2im's
 * [-1,1] -> [0,255] mapping, as the reference's do.  Allocates the sheet; a graph captured earlier is dropped, so the next
 * swn_pipeline_run(use_graph) runs eagerly and captures again, the one after replays.  May be called again (new tables).  RGB bodies,
 * at most 16 ROIs.  Without this call the pipeline enqueues exactly what it did before the call existed. */
int swn_pipeline_enable_images(swn_pipeline* p, const float* body_mean3, const float* body_std3, const float* tex_mean3,
                               const float* tex_std3, const uint8_t* colours, int width, int reference_quirk);
/* The sheet of the last run: *dev = library-owned device bytes (K,B,H,W,3), *k = K = 6, in the order inputs_decoded (the warp
 * stage's input cloth: argmax of the staged one-hot map, which is the staged label map), bodys_unnormalized, fakes_decoded (from
 * swn_pipeline_labels' map; also the texture stage's cloths_decoded, whose cloth input is that map), textures_unnormalized with the
 * ROI outlines, fakes, fakes_scaled.  Stream-ordered behind the run: synchronise (swn_ctx_sync) before reading. */
int swn_pipeline_images(swn_pipeline* p, uint8_t** dev, int* k);
/* The PNG files of that sheet, encoded on the device -- what util.save_image (util/util.py:54-69: Image.fromarray(a).save(path), six
 * times per sample) makes the host's zlib do.  Requires swn_pipeline_enable_images first (otherwise an error that says so).  An armed
 * pipeline ends its graph with the two launches of swn_op_png_encode over the K * B images of the sheet; arming after a capture drops
 * the graph, as swn_pipeline_enable_images does.  rows_per_chunk as in swn_op_png_encode (0 = default).  May be called again. */
int swn_pipeline_enable_png(swn_pipeline* p, int rows_per_chunk);
/* The streams of the last run, library-owned device memory: *streams = K * B zlib streams, *stride bytes apart, in the sheet's order
 * (image k of sample b at index k * B + b); *sizes = their K * B lengths; *k = K = 6.  Stream-ordered behind the run: synchronise
 * before reading.  The PNG container around a stream is host work: swapnet_amd/util/png.py png_container. */
int swn_pipeline_png(swn_pipeline* p, uint8_t** streams, uint32_t** sizes, size_t* stride, int* k);

/* Data-parallel texture stage: the style term is MSE(Gram(output), Gram(target)) with the Gram over the WHOLE batch viewed
 * as (B*C, H*W) (modules/losses/perceptual.py:6-10,58-63), so it couples the samples of all ranks.  The host all-gathers the
 * generated and target images ((n_total, 3, H, W) each; this rank's samples start at n0) after swn_model_forward; the next
 * backward_G evaluates the Gram over that global batch and back-propagates into the local samples -- the step then equals
 * the one-process big-batch step.  One-shot. */
int swn_model_set_style_context(swn_model* m, const float* all_out_nchw, const float* all_tgt_nchw, int n_total, int n0);
/* The random draws of the next gradient-penalty pass (modules/loss.py:141-147): alpha = torch.rand(B,1,1,1) as B
 * device floats; beta = torch.rand_like(conditioned_real) as (B, 22, H, W) in the reference's channel order (dragan
 * modes only).  Either may be NULL (the library then draws it from its own counter RNG).  One-shot. */
int swn_model_set_gp_random(swn_model* m, const float* alpha_dev, const float* beta_nchw_dev);
/* NLayerDiscriminator.forward(input) (modules/discriminators.py:134-136) as a standalone call on the model's
 * discriminator weights: x = conditioned input in the reference's channel order, (B, 22, H, W); pred receives
 * (B, 1, (H >> n) - 2, (W >> n) - 2), n = the PatchGAN depth (3: H/8-2).  Uses a private activation set: self.fakes and the staged batch stay untouched. */
int swn_model_discriminate(swn_model* m, const float* x_nchw, float* pred_nchw);
/* nn.Module.train(mode) of the discriminator for swn_model_discriminate (torch/nn/modules/module.py train / eval, as
 * models/base_model.py:91-96 switches the reference's networks): training != 0 (the default, as a freshly built torch module) --
 * BatchNorm sites normalise with the batch's statistics and update their running buffers, as torch would; 0 -- they normalise
 * with the running buffers.  No effect under --norm instance / none.  The training step itself always runs in train mode. */
int swn_model_set_discriminate_mode(swn_model* m, int training);
/* state_dict() buffers of a network (torch.nn.BatchNorm2d's running_mean, running_var, num_batches_tracked under the keys of
 * modules/discriminators.py:119,127,160: model.K.* / net.3.*): neither optimised nor exchanged.  The discriminator (net 1) has
 * them under swn_ctx_set_patchgan_norm(ctx, 1); the generator (net 0) of a texture model created with netG = unet_128 has 33
 * (11 sites, keys model.model.1.model.2.* ...); no other network has any.  info: numel elements of fp32, or one int64 when *is_int64.  set / get copy
 * between DEVICE pointers of that type.  Models sharing arenas (swn_model_create_shared) share the buffers. */
int swn_model_buffer_count(swn_model* m, int net, int* out);
int swn_model_buffer_info(swn_model* m, int net, int index, char* name, int name_len, int* numel, int* is_int64);
int swn_model_buffer_set(swn_model* m, int net, const char* name, const void* src);
int swn_model_buffer_get(swn_model* m, int net, const char* name, void* dst);
/* PerceptualLoss(use_style)(output, target) -> (content, style) (modules/losses/perceptual.py:49-66), texture model:
 * output / target (B, 3, H, W); out2 = device float[2] = { sum over the 5 VGG16 slices of MSE(normalised features),
 * 5 x MSE(Gram(output), Gram(target)) }.  d_output (optional, (B,3,H,W)) receives content_w * d(content)/d(output)
 * + style_w * d(style)/d(output) -- what autograd would return for content_w*content + style_w*style. */
int swn_model_perceptual(swn_model* m, const float* output_nchw, const float* target_nchw, int use_style, float* out2,
                         float content_w, float style_w, float* d_output_nchw);

/* BaseModel.forward (models/warp_model.py:106-107, models/texture_model.py:121-125) */
int swn_model_forward(swn_model* m, int training, uint64_t dropout_seed);
/* WarpModel.backward_D / TextureModel.backward_D (warp_model.py:109-139, texture_model.py:
 * 127-155); the two labels are the smooth-label scalars GANLoss draws (modules/loss.py:79-108) */
int swn_model_backward_D(swn_model* m, float label_fake, float label_real);
/* backward_G (warp_model.py:141-167, texture_model.py:157-180) */
int swn_model_backward_G(swn_model* m, float label_real);
/* backward_G in `nparts` buckets (part = 0 .. nparts-1, in this order) so the data-parallel exchange of
 * the generator gradients overlaps the rest of the backward pass: part 0 runs the loss head and the
 * last layers (decoder + late residual blocks), each further part the next group of earlier layers;
 * on return the arena range [ready_off, ready_off+ready_count) holds final gradients and can be handed to
 * the all-reduce while the next part runs.  The ranges tile the arena from its end to its start. */
int swn_model_backward_G_parts(swn_model* m, int* nparts);
int swn_model_backward_G_part(swn_model* m, float label_real, int part, size_t* ready_off, size_t* ready_count);
/* optimizer_{G,D}.step() (models/base_gan.py:199,203): fused AdamW over the net's arena */
int swn_model_optimizer_step(swn_model* m, int net);
/* the same AdamW step restricted to the arena range [off, off+count) (the ranges swn_model_backward_G_part reports):
 * under data parallelism a bucket is stepped as soon as its all-reduce has landed, while the next bucket is still
 * being back-propagated.  first != 0 on the first range of an optimizer step (advances AdamW's step counter). */
int swn_model_optimizer_step_range(swn_model* m, int net, size_t off, size_t count, int first);
/* BaseGAN.optimize_parameters (models/base_gan.py:194-203; warp_model.py:169-183) in one call.  With the context's second
 * stream on, optimizer_G.step() (:203) is applied bucket by bucket behind each bucket's weight gradients, under the
 * back-propagation of the earlier layers -- the same element-wise update from the same gradients: bit-identical to the
 * phased calls above (SWN_STREAM_ADAMW=0: one launch after the pass). */
int swn_model_step(swn_model* m, const float labels[3], int training, uint64_t dropout_seed);
/* Data parallelism with the exchange owned by this library (SURVEY.md 8(b) "allreduce_attach(rccl_comm)", 8(e); the reference has no
 * multi-GPU code: models/base_gan.py:194-203 is the step being sharded).  swn_ctx_attach_comm hands over an all-reduce entry point
 * with ncclAllReduce's signature -- RCCL's own symbol, taken from the librccl the process already holds, so no second copy of RCCL
 * is linked -- and the communicator to call it on (one rank per GPU, ncclCommInitRank done by the caller: swapnet_amd/parallel.py
 * NativeComm).  The library gives the exchange a HIP stream of its own and orders it against its compute streams with events it
 * records itself.  swn_model_step_dp is optimize_parameters under data parallelism in one call: backward_D, all-reduce(SUM) of D's
 * gradient arena, optimizer_D, then the generator's backward pass bucket by bucket, each bucket's all-reduce enqueued on the
 * exchange stream the moment its gradients are final and its AdamW on the same stream behind it; the compute stream joins the
 * exchange stream once, at the end of the step.  swn_hyper.grad_scale = 1 / world makes SUM the mean.  after_forward != 0: the
 * caller ran swn_model_forward itself (texture stage with the style term: swn_model_set_style_context goes in between).
 * fn == NULL detaches.  dtype / op are passed as ncclFloat32 (7) / ncclSum (0). */
typedef int (*swn_allreduce_fn)(const void* sendbuf, void* recvbuf, size_t count, int dtype, int op, void* comm, void* stream);
int swn_ctx_attach_comm(swn_ctx* ctx, swn_allreduce_fn fn, void* comm, int world_size);
int swn_model_step_dp(swn_model* m, const float labels[3], int training, uint64_t dropout_seed, int after_forward);
/* The same step recorded once into a hipGraph and replayed (BASELINE.json C5's "hipGraph-captured step"): the three label
 * draws of GANLoss (modules/loss.py:77-104), the dropout seed and both AdamW bias corrections travel through a 40-byte device
 * block uploaded in stream order, so one recorded launch sequence serves every step; the loss read-back of train.py:74
 * (swn_model_get_losses) stays the only synchronisation.  First call per `training` value runs eagerly, the second records,
 * later ones replay.  Results are bit-identical to swn_model_step.  Falls back to swn_model_step for the gradient-penalty
 * modes; under data parallelism use the phased calls (the exchange runs between them). */
int swn_model_step_captured(swn_model* m, const float labels[3], int training, uint64_t dropout_seed);
/* BaseModel.get_current_losses (models/base_model.py:139-147): host array of 9 floats
 * D, D_real, D_fake, G, G_gan, G_ce, G_l1, G_content, G_style, D_gp  (one small D2H + sync; n <= 10) */
int swn_model_get_losses(swn_model* m, float* host_out, int n);

/* data-parallel hook: flat gradient arena of a net (device pointer, float count) so the host
 * can all-reduce it with RCCL (torch.distributed, backend "nccl") between backward and step */
int swn_model_grad_arena(swn_model* m, int net, float** dev_ptr, size_t* count);
int swn_model_weight_arena(swn_model* m, int net, float** dev_ptr, size_t* count);
/* any of the four arenas (which: 0 weight, 1 grad, 2 exp_avg, 3 exp_avg_sq); the layout does
 * not depend on the batch shape, so a whole training state moves with flat copies */
int swn_model_arena(swn_model* m, int net, int which, float** dev_ptr, size_t* count);

/* ---- operator-level entry points (parity tests, integer work, inference helpers) --------- */
/* torchvision.ops.RoIAlign((128,128),1,1) as used at modules/swapnet_modules.py:166-168,234.
 * tex (B,C,H,W) NCHW, rois (B,R,4) -> out (B,R*C,PH,PW) NCHW */
int swn_op_roi_align(swn_ctx* ctx, const float* tex, int b, int c, int h, int w, const float* rois, int r,
                     int ph, int pw, float* out);
/* integer part only: idx (B*R,PH,PW,4) int32 = yl,yh,xl,xh ; valid (B*R,PH,PW) uint8 */
int swn_op_roi_align_indices(swn_ctx* ctx, const float* rois, int k, int h, int w, int ph, int pw, int32_t* idx,
                             uint8_t* valid);
/* util.decode_labels.decode_cloth_labels (util/decode_labels.py:24-55): (B,C,H,W) f32 -> (B,3,H,W) u8 */
int swn_op_decode_labels(swn_ctx* ctx, const float* x, int b, int c, int h, int w, uint8_t* rgb);
/* util.tensor2im (util/util.py:9-32) for a whole batch, with what the reference runs in front of it folded in: out (B,H,W,3) uint8,
 * interleaved, what Image.fromarray takes.  All pointers but ctx are device pointers.
 *   source 0 (float):  x (B,C,H,W) NCHW, C = 3, or 1 replicated to three (util/util.py:24-25);
 *   source 1 (argmax): x (B,C,H,W), C label channels; the first maximum selects one of the 19 colours of util/decode_labels.py:8-21;
 *   source 2 (labels): x NULL, labels (B,H,W) int32 select the colour.  A label outside [0,19) gives black.  Palette sources write
 *     the palette's bytes (the reference's tensor2im of decode_cloth_labels' uint8 tensor wraps modulo 256: not reproduced).
 *   rows (float source, or NULL): [B][2C+1] = scale[C], shift[C], clamp flag per image: u = v * scale + shift, two rounded fp32
 *     operations, then clamp to [0,1] if the flag is non-zero -- unnormalize (datasets/data_utils.py:41-58), which zips over dim 0:
 *     image b < 3 gets (std[b], mean[b]) on all channels and is clamped, later images are left alone (scale 1, shift 0, flag 0).
 *   scale_each != 0 (float source, excludes rows): scale_tensor(scale_each=True) (datasets/data_utils.py:61-90): lo / hi = min / max of
 *     image b, u = (clamp(v, lo, hi) + (-lo)) / (float)((double)hi - (double)lo + 1e-5), reduced on the device.
 *   range 0: byte = (u + 1) / 2 * 255 (tensor2im; the reference applies it to its [0,1] visuals as well); 1: byte = u * 255.  Both
 *     saturate to [0,255] and truncate: numpy's cast wherever that is defined.  NaN in a float source: unspecified bytes.
 *   rois (B,R,4) = x0,y0,x1,y1, R <= 16 (0: none), colours (R,3) uint8, width >= 1: draw_rois_on_texture (util/draw_rois.py:16-47):
 *     a pixel takes the colour of the last ROI whose outline covers it, by Pillow's ImageDraw.rectangle(outline, width) rule
 *     (coordinates truncated toward zero, clipped to the image).  x1 < x0 or y1 < y0 is Pillow's ValueError: check before calling. */
int swn_op_image_u8(swn_ctx* ctx, const float* x, int b, int c, int h, int w, const int32_t* labels, int source, const float* rows,
                    int scale_each, int range, const float* rois, int r, const uint8_t* colours, int width, uint8_t* out);
/* The encoding half of util.save_image (util/util.py:54-69: Image.fromarray(image_numpy).save(image_path) writes a PNG): n images
 * (h,w,3) uint8, interleaved and contiguous -- what swn_op_image_u8 writes -- to n zlib streams (RFC 1950) of the PNG-filtered
 * scanlines, streams[i * stream_stride ...], sizes[i] bytes long.  img, streams and sizes are DEVICE pointers.  Rows are filtered by the
 * type with the smallest sum of min(b, 256 - b) (ties to the lower type); each chunk of rows_per_chunk rows (0 = default:
 * min(16, 32768 / (1 + 3w)), at least 1) becomes one dynamic-Huffman block with run-length matches, or a stored block where that is
 * not larger.  w <= 2048 and rows_per_chunk * (1 + 3w) <= 32768, otherwise an error (code 1).  stream_stride >=
 * swn_png_stream_bound(h, w, rows_per_chunk); bytes of a slot behind its stream are not written.  Signature, IHDR, IDAT and IEND are
 * assembled on the host (swapnet_amd/util/png.py).  Synchronises.  Device library only. */
int swn_op_png_encode(swn_ctx* ctx, const uint8_t* img, int n, int h, int w, int rows_per_chunk, uint8_t* streams, size_t stream_stride,
                      uint32_t* sizes);
/* No stream of swn_op_png_encode for this shape is longer than *out bytes (plain arithmetic: answered by every build). */
int swn_png_stream_bound(int h, int w, int rows_per_chunk, size_t* out);
/* datasets/data_utils.py:322 (argmax for compress_and_save_cloth) and :330-343 (to_onehot_tensor) */
int swn_op_argmax_labels(swn_ctx* ctx, const float* x, int b, int c, int h, int w, int32_t* labels);
int swn_op_labels_to_onehot(swn_ctx* ctx, const int32_t* labels, int b, int c, int h, int w, float* out);
/* a single convolution through the MFMA implicit-GEMM kernel (or the naive checker):
 * kind 0 k4s2p1, 1 k3s1 reflect, 2 k4s1p1, 3 k3s1 zero-pad, 4 upsample-pad-conv tail, 5 k1s1 (PixelDiscriminator);
 * transposed!=0 -> ConvTranspose2d k4s2p1 (weight (Ci,Co,4,4)).  x (N,Ci,H,W), y NCHW.
 * what: 0 forward, 1 weight gradient (y = dY in, w = dW out), 2 input gradient (y = dY in, x = dX out) */
int swn_op_conv(swn_ctx* ctx, int kind, int transposed, int what, int naive, float* x, int n, int ci, int h, int w,
                float* wgt, int co, const float* bias, int act, float* y);
/* The same convolution with its operands PRODUCED on the tape, as inside a network: x0 -> [pre] -> x -> [conv] -> y -> [post] -> z.
 * swn_op_conv fills x and dY from outside, so its launches take the amax of their operands themselves; here x and dY = y.g are
 * written by kernels of the library, which leave the amax in the buffers' slots, and the conv launches take the producer-scaled
 * routes a training step takes (pair-form Winograd planes, slot-scaled ring launches).
 * pre:  0 identity, 1 InstanceNorm + LeakyReLU(0.2), 2 ReLU, 3 nearest upsample x2 (h, w even), 4 MaxPool2d(2, 2);
 * post: 0 identity, 1 InstanceNorm + LeakyReLU(0.2).
 * n, ci, h, w describe the CONV input x; x0 is (n, ci, h0, w0) with h0 = h / 2 (pre 3), 2 h (pre 4), else h.
 * what 0: x = x0 in, y = z out.  what 1: x = x0 in, y = dZ in, wgt = weights in (the forward pass in front of
 * the backward one runs on them; zeros will do behind identity stages) and dW out.  what 2: y = dZ in, wgt in, x = dX out, the gradient
 * with respect to the conv input x, (n, ci, h, w); x0 is zero.  With pre = post = 0 every result equals swn_op_conv's.
 * Optional outputs (device pointers, NULL to skip): x_out = the produced x, NCHW (n, ci, h, w); dy_out = y.g, NCHW (backward
 * calls); x_slot, y_slot, z_slot, dy_slot = the 256 floats of the amax slot of x, y, z, y.g (an error when that buffer has no
 * complete slot on the layer's route: y has one only behind a fused LeakyReLU / ReLU); kscale_out = the layer's published
 * pair-form scale exponents, at most 8 ints in the order the layer reserved them (entries past its count are left untouched). */
int swn_op_conv_produced(swn_ctx* ctx, int kind, int transposed, int what, int naive, float* x, int n, int ci, int h, int w,
                         float* wgt, int co, const float* bias, int act, float* y, int pre, int post, float* x_out, float* x_slot,
                         float* y_slot, float* z_slot, float* dy_out, float* dy_slot, int* kscale_out);
/* InstanceNorm(+act) forward / backward on NCHW tensors (modules/__init__.py:66-69) */
int swn_op_instance_norm_act(swn_ctx* ctx, const float* x, int n, int c, int h, int w, int act, float* y);
int swn_op_instance_norm_act_bwd(swn_ctx* ctx, const float* x, const float* dy, int n, int c, int h, int w, int act,
                                 float* dx);
/* BatchNorm2d(+act) forward / backward on NCHW tensors (modules/__init__.py:62-65: nn.BatchNorm2d(affine=True,
 * track_running_stats=True), eps 1e-5, momentum 0.1; as used by modules/discriminators.py:118-120,126-128,159-161).
 * groups (1 or 2): the batch is `groups` consecutive runs of n / groups images, and the call equals `groups` calls of the torch
 * module on the runs in order -- each run normalised with its own biased statistics, the running buffers updated once per run with
 * the unbiased variance, num_batches_tracked (device int64, optional) += groups.  This is how the discriminator's fake and real
 * passes (models/warp_model.py:115-121) run as ONE 2B batch.  One value per channel and run (n / groups * h * w == 1) is refused
 * as torch refuses it.  training = 0: normalise with the running buffers, which stay untouched (groups is ignored).
 * weight, bias, running_mean, running_var: (c) device floats; the running buffers are updated IN PLACE (training; NULL = no
 * update).  save_stats (optional, training): (groups, c, 2) = (mean, 1 / sqrt(var + eps)) of every run.
 * _bwd: dy -> dx, dweight, dbias (both NULL: the parameter gradients are skipped, dx is the same) through the training-mode
 * forward; with two groups the parameter gradients are the sum over the runs.
 * HIP kernels only: the CI simulator returns the library's "not implemented" error. */
int swn_op_batch_norm_act(swn_ctx* ctx, const float* x, int n, int c, int h, int w, int groups, int act, int training,
                          const float* weight, const float* bias, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float* y, float* save_stats);
int swn_op_batch_norm_act_bwd(swn_ctx* ctx, const float* x, const float* dy, int n, int c, int h, int w, int groups, int act,
                              const float* weight, const float* bias, float* dx, float* dweight, float* dbias);
/* BatchNorm2d -> [act] -> nn.Dropout(p) in TRAINING mode as ONE op (the upnorm -> Dropout sites of the pix2pix U-Net), one group,
 * no running buffers: y, the keep/scale mask it used (0 or 1/(1-p); optional, p > 0 only) and, when dy and dx are given (they go
 * together), dx and optionally dweight / dbias computed with the same mask: a dropped element adds nothing to any of them.
 * p = 0 launches the kernels of swn_op_batch_norm_act / _bwd and gives their results bit for bit.  NCHW fp32, C % 4 == 0.
 * HIP kernels only: the CI simulator returns the library's "not implemented" error. */
int swn_op_batch_norm_act_dropout(swn_ctx* ctx, const float* x, const float* dy, int n, int c, int h, int w, int act, float p,
                                  uint64_t seed, const float* weight, const float* bias, float* y, float* mask, float* dx,
                                  float* dweight, float* dbias);
/* The forward (what 0) or backward (what 1) pass of the layer behind swn_op_instance_norm_act (kind 0; modules/__init__.py:66-69) or
 * swn_op_batch_norm_act (kind 1, training mode, weight 1, bias 0; modules/__init__.py:62-65) timed with HIP events on the
 * context's stream: `warmup` untimed runs, then `iters` timed ones back to back on the same buffers, ms_out[i] (HOST floats) = the
 * i-th.  Only the pass is timed -- no layout conversion, allocation or synchronisation inside the window (tools/bn_shapes.py).
 * x, dy: (n, c, h, w) device tensors (dy only for what 1); groups: kind 1 only.  Device library only. */
int swn_op_norm_act_time(swn_ctx* ctx, int kind, int what, const float* x, const float* dy, int n, int c, int h, int w, int groups,
                         int act, int warmup, int iters, float* ms_out);
/* WarpDataset's per-channel augmentation (datasets/warp_dataset.py:131-137, datasets/data_utils.py:346-361
 * per_channel_transform: an independent random flip / affine / perspective chain for each of the 19 cloth channels
 * of each sample) as ONE device gather over the batch instead of B*19*ntransforms PIL calls.  src, dst (B,C,H,W)
 * fp32; maps = device doubles [B*C][nmaps][9] = {kind, c0..c7} applied in index order: kind 0 identity, 1 affine in
 * Pillow's 16.16 fixed point (bit-identical to Image.transform(AFFINE, NEAREST) and to the flips), 2 perspective with
 * NEAREST sampling.  swapnet_amd/datasets/gpu_augment.py draws the parameters like torchvision's transforms do. */
int swn_op_affine_gather(swn_ctx* ctx, const float* src, float* dst, int b, int c, int h, int w, const double* maps,
                         int nmaps);
/* swn_op_affine_gather with one more kind in the table: kind 3 = perspective resampled BICUBIC, c0..c7 as for kind 2 -- what
 * torchvision 0.4.0's RandomPerspective (datasets/__init__.py:87-110 get_transforms; per channel through
 * datasets/data_utils.py:346-361 per_channel_transform, whose Image.fromarray of a float32 array is a mode-"F" image) computes:
 * img.transform(size, PERSPECTIVE, coeffs, Image.BICUBIC).  Bit-identical to Pillow given the same coefficients.  In IEEE double, one
 * rounded operation per step, no fused multiply-add, for output pixel (x, y) of the h x w image:
 *   xc = x + .5, yc = y + .5;  den = c6 xc + c7 yc + 1;  fx = (c0 xc + c1 yc + c2) / den;  fy = (c3 xc + c4 yc + c5) / den
 *   FLOOR(v) = (int)floor(v) for v < 0, else (int)v;  FLOOR(fx) outside [0, w) or FLOOR(fy) outside [0, h): the output is 0 (the fill)
 *   fx -= .5, fy -= .5;  x0 = FLOOR(fx), y0 = FLOOR(fy);  dx = fx - x0, dy = fy - y0;  the 4 x 4 window starts at (x0 - 1, y0 - 1), its
 *   column indices each clipped to [0, w - 1]
 *   cub(v1, v2, v3, v4, d) = p1 + d (p2 + d (p3 + d p4)),  p1 = v2,  p2 = -v1 + v3,  p3 = 2 (v1 - v2) + v3 - v4,  p4 = -v1 + v2 - v3 + v4
 *   window row 0 uses its row index clipped to [0, h - 1]; rows 1 to 3 are evaluated only where their index is inside the image, an
 *   outside row takes the previous row's value;  row value = cub(four texels, dx) with p2, p3, p4 evaluated in FP32 on the fp32 texels
 *   (Pillow's macro receives the FLOAT32 lvalues) and p1 and the Horner form in double;  pixel = (float)cub(r0, r1, r2, r3, dy) in double
 * Kinds 0 to 2 keep their NEAREST meaning.  The rows behind the kind-3 row are walked first from the output pixel; the rows in front of
 * it define the image the sixteen taps read: each tap walks them backwards like swn_op_affine_gather, and a tap that leaves the image
 * on the way reads 0.  PRECONDITION: at most one kind-3 row per chain (one RandomOrder draw cannot produce more; a further one is
 * resampled NEAREST, nothing is accessed out of bounds); coefficients finite with |fx|, |fy| < 2^31; h * w < 2^31.  A table without
 * kind 3 gives swn_op_affine_gather's bytes.  What stays unpinned is torchvision's float32 least-squares fit of the coefficients. */
int swn_op_chain_resample(swn_ctx* ctx, const float* src, float* dst, int b, int c, int h, int w, const double* maps,
                          int nmaps);
/* TextureDataset.__getitem__ (datasets/texture_dataset.py:87-160, datasets/data_utils.py:169-295) for a whole batch as ONE device
 * launch, from the compact form (arguments as swn_model_set_input_texture_batch; h x w = the crop window at (x_min, y_min)).
 * With (y, x) a pixel of the window, everything in fp32, one correctly rounded operation per step:
 *   tgt_nchw (B,3,h,w)  = (float(img[y_min + y, x_min + x]) / 255 - mean) / std                       to_tensor, Normalize, crop
 *   in_nchw  (B,3,h,w)  = the same of the flipped image: rows mirrored if vflip, then columns if hflip   random_image_roi_flip
 *   cloths_nchw (B,cloth_channels,h,w) = one-hot (label 0: all zero) of labels[min(int(floorf((y_min + y) * (float(hl) / hs))),
 *                         hl - 1)], likewise in x                       to_onehot_tensor, F.interpolate(size = (hs, ws)), crop
 *   rois_out (B,R,4)    = rint(rois_raw * roi_scale); vflip: (y1, y2) <- (-(y2 - cy) + cy, -(y1 - cy) + cy); hflip: the same in x
 *                         with cx; crop: clamp(x, x_min, x_min + w - 1) - x_min, likewise y.  A window that is the whole source
 *                         is the reference's "no crop_bounds": the ROIs are then NOT clamped (crop_rois(rois, None)).
 * cy, cx = int(H0 / 2), int(W0 / 2) of the image BEFORE the resize -- the reference flips the ROIs about the original centre.
 * The resized image is flipped here where the reference flips and resizes a second time; Pillow's resize commutes with both flips
 * bit for bit (tests/test_texture_batch.py).  rois_out must be 16-byte aligned. */
int swn_op_texture_batch(swn_ctx* ctx, const uint8_t* img, int b, int hs, int ws, const uint8_t* labels, int hl, int wl,
                         const float* rois_raw, int r, const float* sample, const float* mean3, const float* std3, int x_min,
                         int y_min, int h, int w, int cloth_channels, float* in_nchw, float* tgt_nchw, float* cloths_nchw,
                         float* rois_out);
/* tf.resize(img, load_size) of TextureDataset.__getitem__ (datasets/texture_dataset.py:93-95,132-134) = Pillow's
 * Image.resize((ws, hs), Image.BILINEAR) on RGB uint8, for a batch of images of DIFFERENT sizes as ONE device launch, byte for byte
 * (Pillow's 8-bit resample; no box, no reducing_gap).  src = packed device bytes; geom_host = HOST (b,3) int64 rows {byte offset, H0,
 * W0}; dst = device (b,hs,ws,3) uint8, dense.  Per axis, source length `in`, output length `out`, in IEEE double, one rounded
 * operation per step, no fused multiply-add:
 *   scale = (double)in / out;  fs = max(scale, 1.0);  support = 1.0 * fs;  ss = 1.0 / fs
 *   for each output index xx:
 *     center = (xx + 0.5) * scale
 *     xmin = (int)(center - support + 0.5), at least 0;  xmax = (int)(center + support + 0.5), at most in;  n = xmax - xmin
 *     w[x] = tri((x + xmin - center + 0.5) * ss) for x = 0 .. n-1,  tri(a) = |a| < 1 ? 1 - |a| : 0
 *     ww = w[0] + w[1] + ... in index order;  w[x] /= ww if ww != 0;  k[x] = (int)(0.5 + w[x] * 4194304.0)      22 fractional bits
 *   one pass, per output element and colour byte:  dst = clamp((2097152 + sum_x src[xmin + x] * k[x]) >> 22, 0, 255)     in int32
 * If ws != W0 the horizontal pass runs first and leaves ROUNDED bytes (H0, ws); if hs != H0 the vertical pass runs on those.  An
 * axis whose length does not change is not resampled; both equal: a copy.  Every sample is validated before anything is
 * launched: H0, W0 >= 1, offset + 3 * H0 * W0 <= src_bytes (samples may overlap), and BOUND: H0 <= 31 * hs and W0 <= 31 * ws (windows
 * of at most 63 taps; a larger reduction is refused by name).  The kernel cannot read outside [src, src + src_bytes).  Enqueued on
 * the context's stream: no device allocation, no synchronisation; geom_host is consumed before the call returns.  On the simulator
 * src and dst are host pointers. */
int swn_op_resize_u8(swn_ctx* ctx, const uint8_t* src, size_t src_bytes, const int64_t* geom_host, int b, int hs, int ws, uint8_t* dst);
/* WarpDataset.__getitem__ (datasets/warp_dataset.py:139-183) for a whole batch as ONE device launch, from the compact form
 * (arguments as swn_model_set_input_warp_batch; h x w = the crop window at (x_min, y_min) of the load_size x load_size resized sample).
 * With (y, x) a pixel of the window, sy = y_min + y, sx = x_min + x, Ls = load_size and
 * near(d, in) = min(int(floorf(d * (float(in) / Ls))), in - 1)           (F.interpolate(size = Ls), torch's nearest rule):
 *   target_cloths_nchw (B,cloth_channels,h,w) = one-hot (label 0 and labels >= cloth_channels: all zero) of
 *                         tgt_labels[near(sy, hl), near(sx, wl)]                    to_onehot_tensor, F.interpolate, crop
 *   input_cloths_nchw (B,cloth_channels,h,w): channel c is 1 where channel c's chain of maps, walked backwards from
 *                         (near(sy, hl), near(sx, wl)) exactly as swn_op_affine_gather walks it on the hl x wl map (16.16 fixed
 *                         point for kind 1, the double-precision perspective for kind 2), stays inside the map and ends on a pixel
 *                         with in_labels == c, c != 0; else 0      per_channel_transform of the one-hot map, F.interpolate, crop
 *   bodys_nchw (B,3,h,w) = bilinear sample (align_corners False) of the texels t = (float(byte) / 255 - mean) / std of the hb x wb
 *                         image, in fp32, one correctly rounded operation per step, no fused multiply-add:
 *                           src = max(scale * (d + 0.5f) - 0.5f, 0), scale = float(in) / Ls, for d = sy (in = hb) and d = sx (in = wb)
 *                           i0 = min(int(src), in - 1), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1
 *                           v = h0 * (w0 * t[y0,x0] + w1 * t[y0,x1]) + h1 * (w0 * t[y1,x0] + w1 * t[y1,x1])
 *                                                       ToTensor, Normalize, F.interpolate(size = Ls, mode = "bilinear"), crop
 * The float one-hot map of the host chain is never built.  target_cloths_nchw may be NULL (then tgt_labels may be too).  As with
 * swn_op_affine_gather, a kind-2 RandomPerspective is resampled NEAREST (the reference: BICUBIC, which swn_op_warp_batch_ex offers);
 * everything else is bit-identical. */
int swn_op_warp_batch(swn_ctx* ctx, const uint8_t* body, int b, int hb, int wb, const uint8_t* in_labels, const uint8_t* tgt_labels, int hl,
                      int wl, const double* maps, int nmaps, const float* mean3, const float* std3, int load_size, int x_min, int y_min,
                      int h, int w, int cloth_channels, float* bodys_nchw, float* input_cloths_nchw, float* target_cloths_nchw);
/* The same with a trailing `flags`.  Bit 0: the table may hold kind 3 (swn_op_chain_resample: RandomPerspective resampled BICUBIC,
 * datasets/__init__.py:87-110, datasets/data_utils.py:346-361).  Channel c of input_cloths_nchw is then c's chain evaluated by that
 * rule at (near(sy, hl), near(sx, wl)) of the hl x wl map whose texels are the indicators in_labels == c (0 for c = 0): the reference's
 * one-hot map -> per-channel PIL chain -> F.interpolate nearest -> crop, bit for bit given the same coefficients.  bodys_nchw and
 * target_cloths_nchw do not depend on the flag.  flags 0 is swn_op_warp_batch itself: the same launch, the same bytes.
 * PRECONDITION: at most one kind-3 row per chain; kind 3 only with bit 0 set.  Other bits: refused. */
int swn_op_warp_batch_ex(swn_ctx* ctx, const uint8_t* body, int b, int hb, int wb, const uint8_t* in_labels, const uint8_t* tgt_labels, int hl,
                         int wl, const double* maps, int nmaps, const float* mean3, const float* std3, int load_size, int x_min, int y_min,
                         int h, int w, int cloth_channels, float* bodys_nchw, float* input_cloths_nchw, float* target_cloths_nchw,
                         int flags);
/* GANLoss(gan_mode)(prediction, target_is_real) (modules/loss.py:110-130) with the target scalar already drawn
 * (`label`; the smooth-label draw stays host-side like in the reference, loss.py:65-108): mean BCE-with-logits /
 * MSE / +-mean over ALL elements of pred (N,C,H,W).  loss_out = device float; dpred (optional, same shape) receives
 * grad_scale * d(loss)/d(pred). */
int swn_op_gan_loss(swn_ctx* ctx, int gan_mode, const float* pred, int n, int c, int h, int w, float label,
                    int target_is_real, float grad_scale, float* loss_out, float* dpred);
/* One loss kernel of ops.h on NCHW tensors (tests).  kind 0: ce_argmax_loss (a = logits, b = target, c <= 32), 1: l1_loss,
 * 2: normed_mse_loss (c % 4 == 0, c <= 512), 3: gram_style_loss (n * c <= 1024; the only kind that reads n0 / nloc: nloc < 0 =
 * the whole batch, otherwise the gradient is formed for samples [n0, n0 + nloc) and da holds nloc samples).
 * The operands and the gradient live in buffers of c + pad_c channels ((c + pad_c) % 4 == 0) and the kernels get channel-slice
 * views of them (pixel stride > C).  The pad channels of all three buffers hold the bit pattern 0x7f7f7f7f before the call;
 * pad_out (optional, (n or nloc, pad_c, h, w)) receives the gradient buffer's pad channels after it.  accumulate != 0: the
 * incoming contents of da are loaded first and the kernel adds to them.  loss_out = the plain mean (device float); da may be
 * NULL (value only). */
int swn_op_loss(swn_ctx* ctx, int kind, const float* a_nchw, const float* b_nchw, int n, int c, int h, int w, int pad_c,
                float scale, int accumulate, int n0, int nloc, float* loss_out, float* da_nchw, float* pad_out);
/* bias_grad (the column sums of dy over N*H*W) on a (c + pad_c)-channel buffer whose pads hold 0x7f7f7f7f; c, pad_c % 4 == 0;
 * db = c device floats. */
int swn_op_bias_grad(swn_ctx* ctx, const float* dy_nchw, int n, int c, int h, int w, int pad_c, float* db);
/* SSIM(window, reduction, max_val)(img1, img2) of modules/losses/__init__.py:128-259 (Gaussian of :30-35, sigma 1.5), value and both
 * gradients in one call.  img1, img2: (b,c,h,w) fp32, contiguous NCHW, device.  Zero padding (window - 1) / 2, no renormalisation at
 * the border; the window is applied separably (rows, then columns), which differs from the reference's 2-D product by rounding only.
 *   S = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),  C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2
 *   loss = clamp(1 - S, 0, 1) / 2
 * loss_map (NULL ok): the per-element loss (reduction 'none').  loss_sum: one device float, the PLAIN sum over all elements ('sum';
 * 'mean' = loss_sum / (b c h w)), fp64 partials combined in a fixed order: two calls give the same bits.
 * d1 / d2 (each NULL ok): d loss / d img1, d img2 under the upstream gradient gmap (per element, (b,c,h,w)) or, gmap NULL, the scalar
 * gscalar (for 'mean' pass g / (b c h w)); torch's convention at the clamp: the gradient passes where 0 <= 1 - S <= 1.  With a
 * gradient the call runs two tile launches and keeps four coefficient maps (16 bytes per element) in the context's workspace; a
 * problem beyond the workspace is refused by name.  window: odd, 1 .. 15 (an even one is refused with the reference's message, a
 * larger one by naming the cap).  Enqueued on the context's stream: no allocation, no synchronisation.  On the simulator all pointers
 * are host pointers. */
int swn_op_ssim(swn_ctx* ctx, const float* img1, const float* img2, int b, int c, int h, int w, int window, float max_val,
                float* loss_map, float* loss_sum, const float* gmap, float gscalar, float* d1, float* d2);
/* L1_Charbonnier_loss (modules/losses/__init__.py:14-27): loss_sum = sum over n elements of sqrt((x - y)^2 + eps) (device float, fp64
 * partials, fixed order); dx = gscalar (x - y) / sqrt((x - y)^2 + eps), dy = -dx (each NULL ok).  Any shape of equal numel, contiguous.
 * One launch plus the finalize, enqueued on the context's stream: no allocation, no synchronisation. */
int swn_op_charbonnier(swn_ctx* ctx, const float* x, const float* y, size_t n, float eps, float gscalar, float* loss_sum, float* dx,
                       float* dy);
/* [InstanceNorm] -> act -> nn.Dropout(p) in TRAINING mode as ONE op (UNetDown / ResidualBlock, modules/layers.py:
 * 18-23,133-136): y, the keep/scale mask it used (0 or 1/(1-p); may be NULL) and, when dy and dx are given, the
 * input gradient computed with the same mask.  NCHW fp32, C % 4 == 0. */
int swn_op_norm_act_dropout(swn_ctx* ctx, const float* x, const float* dy, int n, int c, int h, int w, int norm, int act,
                            float p, uint64_t seed, float* y, float* mask, float* dx);
/* second-order step through y = act(InstanceNorm(x)) (gradient-penalty pass, csrc/gp.cpp): with gx = d<y,gy>/dx the first
 * backward, returns uy = d<gx,u>/d gy and ax = d<gx,u>/d x.  NCHW fp32, C % 4 == 0. */
int swn_op_norm_act_bwd2(swn_ctx* ctx, const float* x, const float* gy, const float* u, int n, int c, int h, int w, int act,
                         float* uy, float* ax);
/* the same step through y = act(BatchNorm2d(x)) in training mode (biased statistics over N*H*W, eps 1e-5, affine gamma / beta of c
 * device floats): uy = d<gx,u>/d gy, ax = d<gx,u>/d x and dgamma = d<gx,u>/d gamma (c device floats; d<gx,u>/d beta is 0 for the
 * piecewise-linear activations).  NCHW fp32, C % 4 == 0.  Device library only: the CI simulator answers "not implemented". */
int swn_op_batch_norm_act_bwd2(swn_ctx* ctx, const float* x, const float* gy, const float* u, const float* gamma, const float* beta,
                               int n, int c, int h, int w, int act, float* uy, float* ax, float* dgamma);
/* The kernels between the convolutions, each launcher of ops.h called alone on channel-slice views (tests).  Convention of the three
 * entry points below: tensors are NCHW device floats; every operand lives in an NHWC buffer of lead + c + pad channels (lead, pad
 * multiples of 4, given per operand in `lead_pad` = {lead, pad} pairs), every byte of which holds 0x7f before the logical channels
 * are loaded, and the launcher gets buffer.slice(lead, c).  The optional *_buf outputs receive the WHOLE buffer afterwards as
 * (n, lead + c + pad, h, w): its non-logical channels must still hold 0x7f7f7f7f.  Amax slots are 256 floats, zeroed before the call.
 *
 * swn_op_norm_act: norm_act_fwd, then (dy and dx given) norm_act_bwd on the same x and stats.  lead_pad[10] = x, y, dy, dx, residual.
 * seed_on_device != 0: the kernels read `seed` from device memory and use seed * 0x9E3779B1 + salt (NormActArgs::seed_base), else
 * `seed` itself.  partial_in (optional, device doubles [n][partial_chunks][c][2]): the statistics' partial sums (finalize + apply,
 * no statistics pass).  want_colsum 0: no column sums; 1: request them where norm_act_bwd_emits_colsum(h * w, c) holds; 2: request
 * them regardless (the launcher refuses where it cannot emit them).  *colsum_emitted (host int) = whether they were requested and
 * written: then colsum = (n, c) device doubles and db = c device floats = bias_grad_from_colsums(colsum).  stats = (n, c, 2).
 * y == NULL: the backward pass alone, with the (mean, rstd) pairs the caller put into `stats`. */
int swn_op_norm_act(swn_ctx* ctx, const float* x, const float* dy, const float* residual, int n, int c, int h, int w, int norm,
                    int act, float drop_p, uint64_t seed, int seed_on_device, uint64_t salt, const double* partial_in,
                    int partial_chunks, const int* lead_pad, int want_colsum, float* y, float* stats, float* y_slot, float* dx,
                    float* dx_slot, double* colsum, int* colsum_emitted, float* db, float* y_buf, float* dx_buf);
/* op 0: act_fwd(a) ; 1: act_bwd(dy = a, y = b) ; 2: axpy(src = a, alpha, shift).  lead_pad[6] = a, b, out.  accumulate != 0 (ops 1, 2):
 * the incoming contents of `out` are loaded first and the kernel adds to them.  slot (optional): the amax slot of what was written. */
int swn_op_elementwise(swn_ctx* ctx, int op, const float* a, const float* b, int n, int c, int h, int w, int act, int accumulate,
                       float alpha, float shift, const int* lead_pad, float* out, float* slot, float* out_buf);
/* (n, c, h, w) is the shape of a.  op 0: upsample_nearest_fwd, out (h * factor, w * factor) ; 1: upsample_nearest_bwd, a = dy, out
 * (h / factor, w / factor) ; 2: maxpool2_fwd, out (h / 2, w / 2), pattern = pool_pattern ; 3: maxpool2_bwd, a = x, b = dy (h / 2,
 * w / 2), out = dx (h, w), pattern = pool_pattern ; 4: reflect_fold, a = the (h, w) gradient of the padded tensor, out (h - 2, w - 2) ;
 * 5: act_pattern of a (no out).  pattern (optional): device bytes, NCHW of the pooled map (ops 2, 3) or of a (op 5).
 * lead_pad[6] = a, b, out; accumulate (ops 1, 3, 4) and slot (ops 0, 2) as in swn_op_elementwise. */
int swn_op_resample(swn_ctx* ctx, int op, const float* a, const float* b, int n, int c, int h, int w, int factor, int accumulate,
                    const int* lead_pad, float* out, float* slot, uint8_t* pattern, float* out_buf);
/* swn_op_conv on views, as the networks call their convolutions (tests): the same kind 0..5, transposed, what 0 / 1 / 2, naive and
 * NCHW tensors of the LOGICAL channels, with the conventions of the three entry points above.  x and y are each a slice of a parent
 * Var (value and gradient buffers of one geometry): the parent has lead_c + C + pad_c channels and n_lead + n + n_pad images, C =
 * round_up(ci, 4) (x; cimap_len with a channel map) or round_up(co, 4) (y), and the conv gets parent.batch(n_lead, n).slice(lead_c, C).
 * views = host int[8]: {lead_c, pad_c, n_lead, n_pad} of x, then of y; lead_c, pad_c multiples of 4.  Every byte of the four parent
 * buffers (x, x.g, y, y.g) holds 0x7f before the logical channels are loaded; the channels INSIDE a view that are not logical -- at
 * and above ci / co, or with map entry -1 -- are loaded with zeros in all four, as the allocator and the producers leave them in a
 * network.  What is not loaded keeps the sentinel (y and y.g of a forward call, x.g of an overwriting input-gradient call, ...).
 * what 0: x, wgt, bias in, y out.  what 1: x in, y = dY in, wgt = weights in (a forward pass in front runs on them) and dW out.
 * what 2: y = dY in, wgt in, x = dX out, all ci logical channels of the view x.g (those a narrow gradient leaves alone come back as
 * they were loaded).  act may be LeakyReLU or ReLU in the backward calls too (tanh in the forward call only): the forward pass then
 * runs first on x (an input of what 2 as well) and the weights, dY is the gradient of the ACTIVATED output, and y_fwd (optional)
 * receives that forward output (n, co, Ho, Wo), from which a reference takes the branch pattern.
 * cimap (optional, host, cimap_len entries, one per view channel of x): view channel -> logical channel or -1 = layout pad; ci must
 * be the number of non-negative entries.  cimap, x_is_input and dgrad_C are handed to the layer unchanged (not with transposed).
 * operand_slots != 0: the value buffer of x and the gradient buffer of y get external amax slots, taken over the loaded VIEWS, as a model
 * gives the buffers it fills from outside the tape; the launches then take the slot-scaled and pair-form routes of a training step
 * (swn_op_conv_produced).  0: every launch takes the amax of its operand itself, with a pass over the view.
 * dx_old (optional, what 2, (n, ci, h, w)): x.g is loaded with it and x is announced to the accumulate planner as a gradient that
 * exists already, so that the planner sets the layer's accumulate flag: the flag reaches the kernels in no other way.  pre_range
 * (optional, host int[2] = {c0, c}): channels [c0, c0 + c) of x's PARENT gradient buffer are announced as existing too; a range that
 * covers part of the view makes planning fail ("partially initialised gradient range").
 * y_slot (optional): the 256 floats of the amax slot of y's buffer after the forward pass; an error where the layer's route leaves
 * no complete slot (it does for a direct conv with fused LeakyReLU / ReLU) and in a backward call that runs no forward pass.
 * dw_rows (optional, what 1): the packed weight gradient with EVERY row of the view, (co, C, KH, KW) (transposed: (C, co, 4, 4)):
 * rows of non-logical channels included.  x_buf, xg_buf, y_buf, yg_buf (optional): each whole parent buffer afterwards,
 * (n_lead + n + n_pad, lead_c + C + pad_c, H, W).
 * What tests/test_conv_views.py holds every route to: nothing outside a view is written (lead / pad channels and images keep
 * 0x7f7f7f7f; the channels of x.g at and above a narrow gradient's dgrad_C keep what they held); the non-logical channels inside
 * the views of y and x.g are exactly 0 afterwards; dw_rows is exactly 0 in the rows of non-logical channels; two runs are bit-equal. */
int swn_op_conv_views(swn_ctx* ctx, int kind, int transposed, int what, int naive, float* x, int n, int ci, int h, int w, float* wgt,
                      int co, const float* bias, int act, float* y, const int* views, const int32_t* cimap, int cimap_len,
                      int x_is_input, int dgrad_C, int operand_slots, const float* dx_old, const int* pre_range, float* y_fwd,
                      float* y_slot, float* dw_rows, float* x_buf, float* xg_buf, float* y_buf, float* yg_buf);
/* torch.optim.AdamW single step on flat arrays (optimizers/__init__.py:52-59) */
int swn_op_adamw(swn_ctx* ctx, float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2,
                 float eps, float wd, int step);
/* adabound.AdaBound single step on flat arrays (optimizers/__init__.py:37-60; the update swn_model_set_optimizer describes),
 * n % 4 == 0, step = 1-based.  HIP library only. */
int swn_op_adabound(swn_ctx* ctx, float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2,
                    float eps, float wd, float final_lr, float base_lr, float gamma, int step);

#ifdef __cplusplus
}
#endif
#endif /* SWAPNET_HIP_H */
