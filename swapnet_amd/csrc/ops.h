// swapnet_amd -- device op launchers.  The engine (engine.cpp) is written against this
// header only.  The product implementation is the set of HIP translation units in this
// directory (conv_gemm.hip and the kernel-family units behind it, wino.hip, norm_act.hip, batch_norm.hip, losses.hip, optim.hip, gather.hip,
// texture_batch.hip, warp_batch.hip, image_resize.hip, image_out.hip, ssim.hip).
// tests/hostsim/hostsim_ops.cpp implements the same signatures with plain loops so that
// the engine's graph / backward / packing logic can be checked in CI without a GPU; it is
// never part of the shipped library.
#pragma once
#include "common.h"
#include "ssim_math.h"
#include <cmath>
#include <cstdlib>
#include <functional>

namespace swn {

struct WShape;

// SWN_* switches, from the value getenv() returned: on unless set to 0 / an integer with a default.  The getenv("SWN_...")
// itself stays at the call site: when it runs is part of each switch's contract (tests/test_route_switches.py)
inline bool env_on(const char* v) { return !(v && atoi(v) == 0); }
inline int env_int(const char* v, int dflt) { return v ? atoi(v) : dflt; }

struct Stream {
  void* handle = nullptr;   // hipStream_t
  char* ws = nullptr;       // scratch for split-K slabs / reduction partials (device)
  size_t ws_bytes = 0;
};

// ---- stream ordering (the weight-gradient side stream of engine.cpp) ------------------------------
void* event_create();
void event_destroy(void* ev);
void event_record(void* ev, Stream& s);
void stream_wait_event(Stream& s, void* ev);      // work enqueued on s afterwards starts after the recorded point

// ---- hipGraph capture of a launch sequence (two-stage inference, pipeline.cpp) ---------------------------------
// graph_begin puts the stream into capture mode: everything enqueued until graph_end is recorded instead of executed
// (no allocation, synchronisation or host read-back in between).  graph_end returns an executable graph handle (NULL on
// the host simulator, which has no graphs: callers then simply run the sequence eagerly).
void* stream_create_current();        // a new non-blocking stream on the calling thread's current device (NULL on the simulator)
void graph_begin(Stream& s);
void* graph_end(Stream& s);
void graph_abort(Stream& s);          // ends a capture that failed half way: status ignored, any partial graph destroyed
void graph_launch(void* exec, Stream& s);
void graph_destroy(void* exec);

// ---- memory -------------------------------------------------------------------------
void* dev_alloc(size_t bytes);            // zero-filled
void dev_free(void* p);
void dev_memset(Stream& s, void* p, int v, size_t bytes);     // a kernel launch (a recordable KERNEL node, not a memset node: device.hip)
void dev_copy(Stream& s, void* dst, const void* src, size_t bytes);        // device->device
void dev_upload(Stream& s, void* dst, const void* src, size_t bytes);      // host->device
// <= 64 bytes (a multiple of 4) of host data into device memory, stream-ordered and WITHOUT a host synchronisation: the bytes travel
// as the arguments of a one-thread kernel (device.hip) -- per-step parameter blocks of a recorded step
void dev_store_small(Stream& s, void* dst, const void* src, size_t bytes);
void dev_download(Stream& s, void* dst, const void* src, size_t bytes);    // device->host (syncs)
void stream_sync(Stream& s);
void* stream_create(int device);          // selects the device, returns a new stream handle
void stream_destroy(void* handle);
void device_check(int device);            // throws unless `device` is a usable HIP device; makes it current
int is_device_build();                    // 1: HIP library, 0: CI host simulator
// `warmup` untimed calls of `enqueue`, then `iters` timed ones back to back on s: ms_host[i] = HIP-event time of the i-th (tools/
// bn_shapes.py through swn_op_norm_act_time).  Synchronises.  Device library only (the simulator has no device clock).
void time_launches(Stream& s, int warmup, int iters, const std::function<void()>& enqueue, float* ms_host);
void conv_force_naive(int on);            // route conv_fwd/conv_wgrad to the naive checkers (tests)
// optional per-launch timing of the implicit-GEMM kernels (bench.py's roofline leg): when on,
// every conv_fwd / conv_wgrad launch is bracketed by HIP events recorded on the launch stream.
void prof_enable(int on);
void prof_reset();
// one line per kernel variant: "<name> <launches> <total_ms> <total_flops>\n"; returns bytes written
int prof_report(char* buf, int len);
// swapnet_hip.h swn_probe_mfma: register-only fp16 MFMA loop, in-kernel clock (prof.hip); synchronises the stream
void probe_mfma(Stream& s, int zeros, int iters, float* out4);
// Routing trace (swn_route_trace / swn_route_report, engine.cpp): which kernel family / algorithmic form every layer of a model
// takes under the current environment.  While on, the engine labels each tape op as it runs it (phase f = forward, b = backward,
// r = derived-operand refresh) and the launchers note the kernel they picked (implicit-GEMM launches with their M, N, K, batch
// and split schedule; the Winograd transforms by form).  The report lists the distinct (label, phase, kernel) triples in first-
// use order: tests compare the list of the configuration bench.py times with the one their own run takes.
void route_enable(int on);
bool route_on();
void route_label(const char* label, char phase);
void route_note(const char* kernel);
int route_report(char* buf, int len);      // returns the bytes the full report needs
// Slot audit (swn_slot_audit, engine.cpp): the host simulator's sim_slot_check and pair-plane check, applied by the HIP launchers to
// what the producers really left behind.  Off by default: one flag test per launch, like route_on().  While on, every launch that
// takes an operand's scale from an amax slot (conv_fwd, conv_wgrad, the pair-form Winograd transforms) also takes the amax of exactly
// what it gathers with a pass, reads both back and throws unless amax <= slot <= 4096 * amax; a pair-form transform additionally
// requires amax(plane) * 2^k < 65504.  The read-back synchronises: an open stream capture is an error, step_captured is not audited.
// The simulator always checks, so there the flag does nothing.
void slot_audit(int on);
bool slot_audit_on();

// ---- implicit-GEMM convolution (MFMA) -----------------------------------------------
// y[map(m)][co] (=|+=) act( sum_k A[m][k] * w[k][co] + bias[co] ),  A = gather(x)
// Views and pad channels (tests/test_conv_views.py asserts every line of this, per kernel route, through swn_op_conv_views): x, y and
// dy are channel-slice views (cs >= C, any base offset, a run of the parent's images) and every route -- the launches below, the
// Winograd transforms and adjoints, the amax passes in front of and behind them -- reads and writes channels [0, C) of the view's
// pixels and nothing else of the buffer.  The channels of a view at and above the layer's logical count (x.C > Ci, y.C = round_up(Cout,
// 4) > Cout) and the layout pads of a channel map hold zeros on entry; a launch leaves them alone or writes zeros into them (adds zero
// when it accumulates), so they are exactly 0 afterwards, and the weight-gradient rows of such input channels are exactly 0.  With
// accumulate the launch adds to what the view holds; an input gradient formed for the first dgrad_C channels only leaves the others
// as they were.  The order of every sum is fixed by the shape: two runs give bit-equal results.
struct ConvFwdArgs {
  TView x;
  Gather g;
  const float* w = nullptr;   // [K = KH*KW*x.C][Npad]
  int Npad = 0;
  const float* bias = nullptr;
  int act = ACT_NONE;
  int accumulate = 0;         // 1: y += result (act must be NONE)
  TView y;                    // y.C = Cout (logical), may be a slice
  OutMap om;
  int Cout = 0;               // valid output channels (<= Npad)
  // batched mode (Winograd: the 16 / 36 plane GEMMs in one launch): element strides between batches
  int batch = 1;
  size_t x_bs = 0, w_bs = 0, y_bs = 0;
  // sub-pixel phase mode (k4s2 transposed convs and the dgrad of k4s2 convs): with phases = 4 one
  // launch covers the four phases ph = 2a + b of a stride-2 scatter: phase ph gathers with
  // pad_t = g.pad_t - a, pad_l = g.pad_l - b, writes outputs (2oy + a, 2ox + b) (om.ymul = om.xmul = 2)
  // and uses the weight panel w + ph * w_bs.  Excludes batch > 1.
  int phases = 0;
  // folded tail conv (tail_fold_weights below), four phases fused: w = the folded block, g = the 3x3
  // union gather (KH = KW = 3, stride 1, pad 1 on the un-upsampled input), om.ymul = om.xmul = 2; phase
  // (a,b) uses taps u < 2+a, v < 2+b and writes outputs (2oy + a, 2ox + b).
  int tail4 = 0;
  // optional: the weight operand pre-cut into bf16 planes (conv_precut below) for the column tile `wpc_bn`; `w` stays valid
  // (the launch falls back to it when it does not take the pre-cut kernel).  wpc_bs = elements between batch / phase panels.
  const uint16_t* wpc = nullptr;
  int wpc_bn = 0;
  size_t wpc_bs = 0;
  // optional: an amax slot of the A operand (AMAX_SLOT floats, device; their maximum >= max |x| over everything the launch
  // gathers).  The two-plane kernels scale the operand by a power of two from it; without a slot the launch takes the amax itself
  // with a pass over x.  Producers that write the operand fill the slot for free (amax_out of the transforms below).
  const float* x_amax = nullptr;
  // optional: the A operand is stored in PAIR form (see wino_input_transform): *x_pair_k = the exponent its producer scaled it by
  const int* x_pair_k = nullptr;
  // optional: an amax slot the launch folds max |y| of everything it stores into -- in the epilogue of the pre-cut ring kernel
  // (and the reduce kernel of its split tiles), by a pass over the output view behind every other kernel family
  float* y_amax = nullptr;
  // optional (north_star's Conv + InstanceNorm fusion, modules/layers.py:12-24): the launch leaves the InstanceNorm statistics'
  // partial sums of its OUTPUT behind -- stat_partial[(m / chunk) * y.C + c][2] = (sum, sum of squares) in fp64 over the `chunk`
  // consecutive output rows m of one image, chunk = conv_fwd_stat_chunk(...) -- from the accumulators in the epilogue, so that
  // norm_act_fwd needs no statistics pass over the tensor (NormActArgs::partial_in).  Requires act = NONE, accumulate = 0, one launch
  // (no batch / phases) and Ho * Wo a multiple of the chunk.
  double* stat_partial = nullptr;
};
// rows per statistics partial if a forward conv (K = taps x xC) over xC input channels into Npad columns, nimg images of HoWo output
// pixels each, can emit them -- the 128 x 128 pre-cut ring kernel, HoWo a multiple of its 128 rows, and a launch the planner runs in
// whole tiles anyway (no K split to give up) -- else 0 (always 0 on the host simulator)
int conv_fwd_stat_chunk(int xC, int Npad, int HoWo, int nimg, int K);
constexpr int AMAX_SLOT = 256;
// 256 partial maxima of |x| over a view into `slot` (overwrites all AMAX_SLOT entries): the amax of a tensor no kernel of ours
// produced (network inputs)
void tensor_amax(Stream& s, const TView& x, float* slot, float floor = 0.f);
void conv_fwd(Stream& s, const ConvFwdArgs& a);
// Pre-cut weight operand of the LDS-DMA ring kernel (conv_ring.hip conv_fwd_pc_kernel): x = hi + mid + lo, three bf16 planes by
// truncation (exact), laid out in MFMA operand order per 16-k stage and column tile.  conv_precut_tile: the column tile (64 /
// 128) a forward-type launch over xC input channels into Npad columns takes, 0 = it would not use a pre-cut operand (host
// simulator, narrow / first-layer launches, SWN_PRECUT=0): callers then need not produce one.
int conv_precut_tile(int xC, int Npad);
size_t conv_precut_elems(int K, int Npad, int bn);       // uint16 elements of one [K][Npad] panel
// amax_io (two-plane form, optional): a layer's forward and input-gradient operands are permutations (transposes, flips, leading
// channels) of ONE parameter tensor, so the 256 partial maxima taken for the first bound the second.  *amax_io == NULL on entry: the
// launch takes its own and leaves the pointer; != NULL: it uses them -- valid only back to back on one stream (the partials live in the
// stream scratch until the next pass) and for sources whose values are a subset of what the partials were taken over.
void conv_precut(Stream& s, const float* w, int K, int Npad, int bn, int batch, size_t w_bs, uint16_t* out, const float** amax_io = nullptr);
// Plane format of the pre-cut operands: 3 = three bf16 planes (six MFMAs per product), 2 = two fp16 planes of the operand times a
// power of two chosen from its amax (three MFMAs; conv_gemm.h "two fp16 planes").  In the two-plane form a panel carries a
// 16-byte trailer with the scale exponent (counted by conv_precut_elems) and a producer first takes the 256 partial maxima of its
// SOURCE tensor ([batch][rows][C] floats, dense rows, batch stride bs) with conv_precut_amax (NULL in the three-plane form).
int conv_precut_planes();
const float* conv_precut_amax(Stream& s, const float* src, size_t rows, int C, int batch, size_t bs);

// dw[k][co] = sum_m A[m][k] * dy[map(m)][co]      (dw: [K][Npad], overwritten)
struct ConvWgradArgs {
  TView x;
  Gather g;
  TView dy;
  OutMap om;
  float* dw = nullptr;
  int Npad = 0;
  int Cout = 0;
  int batch = 1;
  size_t x_bs = 0, dy_bs = 0, dw_bs = 0;
  int phases = 0;             // as in ConvFwdArgs; phase ph reads dy at (2oy + a, 2ox + b), writes dw + ph * dw_bs
  int tail4 = 0;              // as in ConvFwdArgs; dw = the folded-gradient block (layout of tail_fold_weights)
  const float* x_amax = nullptr;      // amax slots of the two operands (as ConvFwdArgs::x_amax)
  const float* dy_amax = nullptr;
  const int* x_pair_k = nullptr;      // operands stored in pair form (as ConvFwdArgs::x_pair_k): scale exponents of their producers
  const int* dy_pair_k = nullptr;
};
// true when the library's transforms / GEMMs implement the pair form (the device build with two-plane operands; SWN_PAIR=0 disables)
bool wino_pair_planes();
// would a batched plane GEMM of these dimensions read pair-form operands? (forward-type: A = planes with xC channels into Npad
// columns; weight-gradient: T rows reduced, K x Npad outputs).  False on the host simulator.
bool conv_fwd_takes_pairs(int xC, int Npad);
bool conv_wgrad_takes_pairs(size_t T, int K, int Npad);
void conv_wgrad(Stream& s, const ConvWgradArgs& a);

// reference implementations of the two launches above (one thread per output element,
// no MFMA): used by tests to cross-check the tiled kernels at sizes the CPU cannot reach.
void conv_fwd_naive(Stream& s, const ConvFwdArgs& a);
void conv_wgrad_naive(Stream& s, const ConvWgradArgs& a);

// db[c] = sum over pixels of dy[.,c]   (db overwritten)
void bias_grad(Stream& s, const TView& dy, float* db);

// dx[i] (+)= sum_{u: reflect(u-1)==i} dxpad[u]   -- folds the (H+2)x(W+2) gradient of a
// ReflectionPad2d(1) back onto the HxW tensor.
void reflect_fold(Stream& s, const TView& dxpad, const TView& dx, int accumulate);

// ---- Winograd F(m x m, r x r) transforms (stride-1 convolutions; see wino.hip) -------------------
// supported (m, r): (2,3), (4,3) for the 3x3 convs, (3,4) for PatchGAN's k4 s1 conv.
// tile (n,ty,tx) covers outputs (m*ty..m*ty+m-1, m*tx..) and input rows m*ty-pad .. m*ty-pad+m+r-2;
// P = (m+r-1)^2 transform planes (16 for F(2,3): 2.25x fewer multiplies; 36 for F(4,3) / F(3,4): 4x fewer)
// amax_out (optional, here and below): an amax slot (AMAX_SLOT floats, zeroed by the caller before the first producer of a
// tensor runs) into which the kernel folds max |v| over everything it writes: entry blockIdx % AMAX_SLOT, an atomic max on
// the bit pattern (non-negative floats order like unsigned integers, so the slot's maximum is exact and order-independent)
// in_amax / kscale_out (optional, the 6-point and strided forms): write the planes in PAIR form for the two-plane GEMMs -- each
// element the 32-bit word {h | l << 16} of fp16 planes of (x 2^k), k derived from the amax slot `in_amax` of the transform's INPUT
// through the transform's gain bound (wino.hip) and published in *kscale_out (device int) for the GEMM (ConvFwdArgs::x_pair_k)
void wino_input_transform(Stream& s, int m, int r, const TView& x, int pad, int pad_mode, int Th, int Tw, float* V,
                          float* amax_out = nullptr, const float* in_amax = nullptr, int* kscale_out = nullptr);        // V[P][T][x.C]
// mode 0: U[P][Cip][Npad] for the forward conv; mode 1: U[P][Npad][Cip] (flipped, transposed) for the transposed-conv form of
// dgrad; mode 2: U[P][Npad][Cip] = mode 0 with the channel axes swapped, the operand of the adjoint form (wino_input_adjoint)
void wino_filter_transform(Stream& s, int m, int r, const WShape& w, int mode, const float* packed, float* U);
// the same transform (modes 0 and 2, 6-point forms) written straight into the pre-cut operand layout of the ring kernel
// (conv_precut's, one panel of `panel_elems` = conv_precut_elems(K, N, bn) uint16 per Winograd plane): no fp32 U at all
void wino_filter_transform_pc(Stream& s, int m, int r, const WShape& w, int mode, const float* packed, int bn, uint16_t* out,
                              size_t panel_elems, const float** amax_io = nullptr);       // amax_io: as conv_precut's
// Input gradient in the forward tiling: dV[P][T][C] = dM U^T (dM = wino_dy_transform of dY, T = dx.N * Th * Tw forward tiles).
// dx (+)= sum over tiles of the patches BT^T dV_t BT placed where wino_input_transform(pad, pad_mode, Th, Tw) gathered them
// (reflected / dropped exactly like the forward gather).  dV is overwritten (scratch).
void wino_input_adjoint(Stream& s, int m, int r, float* dV, int C, int pad, int pad_mode, int Th, int Tw, const TView& dx,
                        int accumulate);
void wino_output_transform(Stream& s, int m, int r, const float* M, int Cm, int Th, int Tw, const float* bias, int act,
                           const TView& y, int Cout, int accumulate, float* amax_out = nullptr);    // amax_out: 6-point forms only                                      // M[P][T][Cm]
void wino_dy_transform(Stream& s, int m, int r, const TView& dy, int Th, int Tw, float* dM, float* amax_out = nullptr,
                       const float* in_amax = nullptr, int* kscale_out = nullptr);                                     // dM[P][T][dy.C]
// ---- the folded tail conv (tail_fold_weights below) in Winograd form: its four sub-pixel phases are (2+a)x(2+b)-tap stride-1
// convolutions over the same input, i.e. four F(4x4,3x3) convolutions sharing ONE wino_input_transform(4, 3, x, pad 1, zero);
// their filters sit side by side on the N axis (N = 4 * Npad) of one batched GEMM.  Th, Tw = tiles of 4x4 INPUT positions.
void tailw_filter_transform(Stream& s, const WShape& w, const float* folded, float* U);        // U[36][Cip][4 * Npad]
void tailw_filter_grad(Stream& s, const WShape& w, const float* dU, float* dfolded);          // dU[36][Cip][4 * Npad] -> folded layout
// y (2H x 2W, Npad channels): y[2 i + a][2 j + b] = act(A^T M_ab A + bias),  M[36][T][4 * Npad]
void tailw_output_transform(Stream& s, const float* M, int Th, int Tw, int Npad, const float* bias, int act, const TView& y, int Cout);
void tailw_dy_transform(Stream& s, const TView& dy, int Th, int Tw, int Npad, float* dM, float* amax_out = nullptr,
                        const float* in_amax = nullptr, int* kscale_out = nullptr);                        // dM[36][T][4 * Npad]
// ---- strided Winograd F(4x4, 2x2): the k4 s2 p1 convolutions and their transposes as four polyphase 2x2 stride-1 convolutions
// sharing one batched GEMM (wino.hip).  "fine" = the 2H x 2W side, "coarse" = the H x W side; tiles = 4x4 coarse pixels.
// (m, r) = (4, 2) is accepted by wino_output_transform (coarse = A^T M A) and wino_dy_transform (dM = A coarse A^T).
void wino_s2_input_transform(Stream& s, const TView& fine, int Th, int Tw, float* V, float* amax_out = nullptr,
                             const float* in_amax = nullptr, int* kscale_out = nullptr);   // V[25][T][4 * fine.C], channel (2s+t)*C + c
// fine (+)= [bias +] adjoint of the transform above applied to dV[25][T][4 * Cf] (overwritten: scratch)
void wino_s2_input_adjoint(Stream& s, float* dV, int Cf, int Th, int Tw, const TView& fine, const float* bias, int accumulate);
// w: the layer's WShape (WK_CONV: fine = input, coarse = output; WK_CONVT: fine = output, coarse = input).
// mode 0: U[25][4 * Cf][Cc] (fine -> coarse GEMM); mode 1: U[25][Cc][4 * Cf] (coarse -> fine GEMM); Cf, Cc = padded counts
void wino_s2_filter_transform(Stream& s, const WShape& w, int mode, const float* packed, float* U);
void wino_s2_filter_grad(Stream& s, const WShape& w, const float* dU, float* dpacked);       // dU[25][4 * Cf][Cc]
void wino_filter_grad(Stream& s, int m, int r, const WShape& w, const float* dU, float* dpacked);          // dU[P][Cip][Npad]

// ---- InstanceNorm / activation / dropout -------------------------------------------
struct NormActArgs {
  TView x;                    // raw conv output (dense)
  TView y;                    // destination (may be a channel slice)
  float* stats = nullptr;     // [N][C][2] (mean, rstd); written when norm
  int norm = 1;
  int act = ACT_NONE;
  float drop_p = 0.f;         // 0 => no dropout
  uint64_t seed = 0;          // dropout stream for this call (ignored if drop_p==0)
  const TView* residual = nullptr;   // y = ... + residual
  float* amax_out = nullptr;  // optional amax slot of y (see wino_input_transform)
  // captured training step (engine.h Model::step_captured): the step seed is read from device memory, so that one recorded
  // launch sequence serves every step -- the kernels use *seed_base * 0x9E3779B1 + salt (= Net::drop_seed) instead of `seed`
  const uint64_t* seed_base = nullptr;
  uint64_t salt = 0;
  // optional: the statistics' partial sums as the producing conv's epilogue left them (ConvFwdArgs::stat_partial):
  // [N][partial_chunks][x.C][2] fp64.  The statistics pass over x is skipped: finalize + apply only.
  const double* partial_in = nullptr;
  int partial_chunks = 0;
};
void norm_act_fwd(Stream& s, const NormActArgs& a);

struct NormActBwdArgs {
  TView dy;                   // grad wrt y (view, same geometry as y)
  TView x;                    // the forward's INPUT x (raw conv output), with and without norm: act' is taken from (x - mean) * rstd,
                              // or from x itself when !norm (tanh: 1 - tanh(x)^2) -- never the output y (tests/test_norm_act_ops.py)
  const float* stats = nullptr;
  TView dx;                   // grad wrt raw conv output (dense), overwritten
  int norm = 1;
  int act = ACT_NONE;
  float drop_p = 0.f;
  uint64_t seed = 0;
  // optional [N][C] (fp64): per-image column sums of dx -- the bias gradient of the conv that produced x, for free while the
  // slab is in registers.  Written only by launches for which norm_act_bwd_emits_colsum(H * W, C) holds.
  double* colsum = nullptr;
  float* amax_out = nullptr;  // optional amax slot of dx
  const uint64_t* seed_base = nullptr;   // as NormActArgs
  uint64_t salt = 0;
};
void norm_act_bwd(Stream& s, const NormActBwdArgs& a);
bool norm_act_bwd_emits_colsum(int HW, int C);
// db[c] = sum_n partial[n][c]   (fixed order)
void bias_grad_from_colsums(Stream& s, const double* partial, int N, int C, float* db);

// ---- BatchNorm2d + activation (batch_norm.hip; modules/__init__.py:62-65: affine, running statistics, eps 1e-5, momentum 0.1) ----
// The batch is `groups` (1 or 2) consecutive runs of N / groups images.  Training mode normalises every run with its own biased
// statistics and updates the running buffers once per run, in run order, with the unbiased variance -- exactly what `groups`
// separate calls on the runs would do (the discriminator's fake and real passes as one 2B batch).  Eval mode normalises with the
// running buffers and changes nothing.  HIP kernels only: on the host simulator both launchers throw "not implemented".
struct BatchNormArgs {
  TView x;                    // raw conv output (dense)
  TView y;                    // destination
  const float* gamma = nullptr;      // [C]
  const float* beta = nullptr;       // [C]
  float* running_mean = nullptr;     // [C]; training: updated when given; eval: read
  float* running_var = nullptr;
  long long* num_batches_tracked = nullptr;   // optional device counter: += groups per training call
  float* stats = nullptr;     // [groups][C][2] (mean, rstd); written in training mode
  float* fold = nullptr;      // [groups][2][C] (scale = gamma * rstd, shift = beta - mean * scale); written, 16-byte aligned
  int groups = 1;
  int act = ACT_NONE;
  int training = 1;
  float* amax_out = nullptr;  // optional amax slot of y (see wino_input_transform)
  // optional (training): the statistics' partial sums as the producing conv's epilogue left them (ConvFwdArgs::stat_partial)
  const double* partial_in = nullptr;
  int partial_chunks = 0;
  // BatchNorm2d -> [act] -> Dropout(p) in the same apply pass (training mode only; eval applies no mask), NormActArgs' conventions:
  // the factor is drop_scale(seed, element index, p), with seed = *seed_base * 0x9E3779B1 + salt when seed_base is given (captured
  // step) -- what dropout_mask exports.  The amax slot of y is taken after the mask.  0 => today's kernels, untouched.
  float drop_p = 0.f;
  uint64_t seed = 0;
  const uint64_t* seed_base = nullptr;
  uint64_t salt = 0;
};
void batch_norm_fwd(Stream& s, const BatchNormArgs& a);
struct BatchNormBwdArgs {
  TView dy;                   // grad wrt y
  TView x;                    // raw conv output saved by forward
  const float* stats = nullptr;      // as the training-mode forward left them
  const float* fold = nullptr;
  TView dx;                   // grad wrt x, overwritten
  float* dgamma = nullptr;    // [C], overwritten; both NULL: the parameter gradients are skipped (dx is the same)
  float* dbeta = nullptr;
  int groups = 1;
  int act = ACT_NONE;
  float* amax_out = nullptr;  // optional amax slot of dx
  // the forward's dropout (BatchNormArgs): dy is multiplied by the same factor before anything else, so a dropped element adds 0
  // to sum(dy'), sum(dy' xh), d gamma, d beta and dx
  float drop_p = 0.f;
  uint64_t seed = 0;
  const uint64_t* seed_base = nullptr;
  uint64_t salt = 0;
};
void batch_norm_bwd(Stream& s, const BatchNormBwdArgs& a);
// Second-order step through y = act(gamma xh + beta), xh = (x - mean) rstd with the biased statistics of ONE group over N H W
// (reverse over reverse; the BatchNorm counterpart of norm_act_bwd2 below: the gradient penalties' pass is one B batch).  With
// z = gamma xh + beta, gm = act'(z) gy, q = gamma gm and <.> the mean over the N H W elements of a channel, the first backward was
// gx = rstd (q - <q> - xh <q xh>).  Given u, the adjoint of gx:
//   v  = rstd (u - <u> - xh <u xh>)
//   uy = act'(z) gamma v                                  (adjoint of gy, and J u for the up pass)
//   ax = -rstd^2 [ xh (<u q> - <u><q> - <u xh><q xh>) + <q xh> (u - <u> - xh <u xh>) + <u xh> (q - <q> - xh <q xh>) ]
//   d gamma = sum v gm = rstd M (<u gm> - <u><gm> - <u xh><gm xh>),  M = N H W;   d beta = 0 (piecewise-linear activations)
// exact with eps inside rstd.  The activation branch is taken from z (with a negative gamma it differs from the sign of xh).  All
// reductions in fp64 and in a fixed order: two runs are bit-identical.  No dropout variant (the discriminator has none).
struct BatchNormBwd2Args {
  TView u, gy, x;             // adjoint of gx; gradient w.r.t. y from the first backward; raw activation
  const float* stats = nullptr;      // as the training-mode forward left them (groups 1)
  const float* fold = nullptr;
  const float* gamma = nullptr;      // [C], 16-byte aligned
  TView uy, ax;               // outputs (overwritten)
  float* dgamma = nullptr;    // [C], overwritten; NULL: skipped
  int act = ACT_NONE;
};
void batch_norm_bwd2(Stream& s, const BatchNormBwd2Args& a);

// The keep/scale factor norm_act_fwd / norm_act_bwd apply at a dropout site, written out as an NCHW tensor
// (N,C,H,W): element (n,c,h,w) = drop_scale(seed, ((n*H*W + h*W + w)*C + c), p) -- 0 or 1/(1-p).
// Diagnostic export (swn_model_dropout_mask): parity tests hand it to the oracle so that a train-mode
// step is compared value for value.
void dropout_mask(Stream& s, int N, int H, int W, int C, float p, uint64_t seed, float* out_nchw);

// The branch every piecewise-linear op took, written out as NCHW bytes (diagnostic export, swn_model_act_pattern).
// LeakyReLU / ReLU: 1 where the activation OUTPUT y is > 0 -- the side act_bwd / norm_act_bwd differentiate on.
// MaxPool2d(2,2): the window position (2*kh + kw) the backward pass routes the gradient to (first maximum in scan
// order).  An fp32 evaluation in another summation order puts pre-activations within round-off of zero on the other
// side; each such flip changes the gradient by O(1) of that element, which is what bounds any fp32-vs-fp64 gradient
// comparison at ~1e-3.  Parity tests replay these patterns in the float64 oracle and compare at ~1e-5 instead.
void act_pattern(Stream& s, const TView& y, uint8_t* out_nchw);
void pool_pattern(Stream& s, const TView& x, const TView& y, uint8_t* out_nchw);

// y = act(x) elementwise on views; bwd: dx (+)= dy * act'  (derivative expressed through the
// activation OUTPUT y: lrelu y>0?1:.2, relu y>0, tanh 1-y^2)
void act_fwd(Stream& s, const TView& x, const TView& y, int act, float* amax_out = nullptr);     // amax_out: fold max|y| into the slot
void act_bwd(Stream& s, const TView& dy, const TView& y, const TView& dx, int act, int accumulate, float* amax_out = nullptr);
// dst (+)= alpha * src + shift   (views)
void axpy(Stream& s, const TView& src, const TView& dst, float alpha, int accumulate, float shift = 0.f, float* amax_out = nullptr);

// ---- resampling / gather ---------------------------------------------------------------
void upsample_nearest_fwd(Stream& s, const TView& x, const TView& y, int factor, float* amax_out = nullptr);
void upsample_nearest_bwd(Stream& s, const TView& dy, const TView& dx, int factor, int accumulate);
void maxpool2_fwd(Stream& s, const TView& x, const TView& y, float* amax_out = nullptr);
void maxpool2_bwd(Stream& s, const TView& dy, const TView& x, const TView& y, const TView& dx, int accumulate);
// legacy RoIAlign (torchvision 0.4.0), sampling_ratio 1, spatial_scale 1.  tex: (B,H,W,C);
// rois: device float [B*R][4] = x1,y1,x2,y2 (batch index = k / R); out: (B,PH,PW,R*C) with
// channel index r*C + c (the reference's view(B,-1,PH,PW), swapnet_modules.py:237-240).
void roi_align_fwd(Stream& s, const TView& tex, int C, const float* rois, int R, const TView& out);
// bit-exact debug dump of the integer part: idx[k][ph][pw][4] = yl,yh,xl,xh ; valid[k][ph][pw]
void roi_align_indices(Stream& s, const float* rois, int K, int H, int W, int PH, int PW,
                       int32_t* idx, uint8_t* valid);

// Per-channel geometric augmentation of the warp dataloader (datasets/warp_dataset.py:131-137 ->
// datasets/data_utils.py:346-361: every one of the 19 cloth channels of every sample goes through its own random
// PIL transform chain) as one device gather.  src / dst: (B, C, H, W) fp32 NCHW.  maps: device doubles
// [B*C][nmaps][9] = { kind, c0..c7 }, applied to a channel in index order (map 0 first), each with PIL's NEAREST rule:
//   kind 0 -- identity;
//   kind 1 -- affine in Pillow's 16.16 fixed point (Geometry.c affine_fixed): c0..c5 = the six FIXed integers
//             a0,a1,a2',a3,a4,a5' (a2', a5' already include the half-pixel terms): xin = (a2' + a1 y + a0 x) >> 16,
//             yin = (a5' + a4 y + a3 x) >> 16 -- flips and RandomAffine, bit-identical to Image.transform(AFFINE, NEAREST);
//   kind 2 -- perspective (Geometry.c perspective_transform): xin = floor((c0 xc + c1 yc + c2) / (c6 xc + c7 yc + 1)),
//             xc = x + .5 (same for y with c3..c5); -1 when negative.
// A source coordinate outside the image at ANY step yields 0 (PIL's fill), like the sequential PIL calls.
void affine_gather(Stream& s, const float* src, float* dst, int B, int C, int H, int W, const double* maps, int nmaps);

// affine_gather with one more kind in the table (gather.hip; the host loop of engine.cpp): kinds 0 to 2 as above, and
//   kind 3 -- perspective resampled BICUBIC, bit-identical to Pillow's Image.transform(size, PERSPECTIVE, c0..c7, BICUBIC) on a mode-"F"
//             image, which is what torchvision 0.4.0's RandomPerspective does to a channel of per_channel_transform
//             (datasets/data_utils.py:346-361).  c0..c7 as for kind 2.  In IEEE double unless said otherwise, one rounded operation per
//             step, no FMA contraction.  For output pixel (x, y):
//               xc = x + .5, yc = y + .5;  den = c6 xc + c7 yc + 1;  fx = (c0 xc + c1 yc + c2) / den;  fy = (c3 xc + c4 yc + c5) / den
//               FLOOR(v) = (int)floor(v) for v < 0, else (int)v.  FLOOR(fx) outside [0, W) or FLOOR(fy) outside [0, H): the output is 0.
//               fx -= .5, fy -= .5;  x0 = FLOOR(fx), y0 = FLOOR(fy);  dx = fx - x0, dy = fy - y0;  the window starts at (x0 - 1, y0 - 1);
//               its four column indices are each clipped to [0, W - 1].
//               cub(v1, v2, v3, v4, d) = p1 + d (p2 + d (p3 + d p4)),  p1 = v2, p2 = -v1 + v3, p3 = 2 (v1 - v2) + v3 - v4,
//               p4 = -v1 + v2 - v3 + v4, every sum left to right.
//               Row 0 of the window uses its row index clipped to [0, H - 1]; rows 1 to 3 are evaluated only where their index lies inside
//               the image, an outside row takes the previous row's value.  A row's value is cub(its four texels, dx), where p2, p3 and p4
//               are FP32 expressions of the fp32 texels (Pillow's macro is handed the FLOAT32 lvalues: each operation rounds to
//               fp32; on 0/1 maps this is exact either way) and p1 and the Horner form in d are double.  The pixel is
//               (float)cub(r0, r1, r2, r3, dy), all in double.
// A chain is evaluated as for affine_gather: the rows behind the kind-3 row are walked first from the output pixel, and the rows in
// front of it define the image the sixteen taps read -- each tap walks them backwards with the NEAREST rule, and a tap that leaves the
// image anywhere on the way reads 0.  PRECONDITION: at most one kind-3 row per chain (what one RandomOrder draw can produce; the
// Python layer refuses more); a further one would be resampled NEAREST like kind 2, and nothing is read or written out of bounds.
// Coefficients are those of the transform's own draw: finite, |fx|, |fy| < 2^31.  A table without kind 3 gives affine_gather's bytes.
void chain_resample(Stream& s, const float* src, float* dst, int B, int C, int H, int W, const double* maps, int nmaps);
inline void chain_resample_check(int B, int C, int H, int W, int nmaps) {
  if (nmaps < 1) throw Error(1, "chain_resample: need at least one map per channel");
  if (B < 1 || C < 1 || H < 1 || W < 1 || (size_t)H * (size_t)W > 0x7fffffffu) throw Error(1, "chain_resample: empty or oversized image");
}

// layout conversion at the Python boundary (NCHW fp32 <-> NHWC view)
void nchw_to_nhwc(Stream& s, const float* src, int N, int C, int H, int W, const TView& dst);
void nhwc_to_nchw(Stream& s, const TView& src, float* dst, int C);
// integer work
void decode_labels(Stream& s, const TView& x, int C, uint8_t* rgb_nchw);            // util/decode_labels.py
void argmax_labels(Stream& s, const TView& x, int C, int32_t* labels);              // data_utils.py:322
void labels_to_onehot(Stream& s, const int32_t* labels, const TView& y, int C);     // data_utils.py:330-343

// ---- texture batch hand-over (texture_batch.hip) ------------------------------------------------------------------------------
// What TextureDataset.__getitem__ (datasets/texture_dataset.py:87-160, datasets/data_utils.py:169-295) computes per sample on the
// host, for a whole batch in ONE launch, from the compact form: the resized uint8 HWC image, the uint8 label map, the raw ROI table
// and five scalars per sample.  With (y, x) a pixel of the H x W crop window at (y_min, x_min) of the Hs x Ws source:
//   tgt_tex[b,y,x,c] = (float(img[b, y_min + y, x_min + x, c]) / 255 - mean[c]) / std[c]                       (to_tensor, Normalize)
//   in_tex          = the same of the flipped image: row Hs-1-. if vflip, then column Ws-1-. if hflip      (random_image_roi_flip)
//   cloth[k][b,y,x,:] = one-hot of labels[b, min(int(floorf((y_min + y) * (float(Hl) / Hs))), Hl - 1), likewise for x]; label 0 and
//                     labels >= C give the all-zero vector                      (to_onehot_tensor, F.interpolate nearest, then the crop)
//   rois_out[b,r]   = v = rintf(rois_raw * roi_scale); vflip: (y1, y2) <- (-(y2 - cy) + cy, -(y1 - cy) + cy); hflip: the same on x
//                     with cx; then clamp(x, x_min, x_min + W - 1) - x_min and likewise for y                (flip_rois_, crop_rois)
// all in fp32, one correctly rounded operation per step, pad channels of every view written as zero.  The ROI clamp belongs to the
// crop: a window that is the whole source (x_min = y_min = 0, H = Hs, W = Ws) is the reference's "no crop_bounds" and leaves the
// ROIs unclamped, as its crop_rois(rois, None) does.  Every view must be 16-byte tileable (C % 4, cs % 4, aligned base).
struct TextureBatchArgs {
  const uint8_t* img = nullptr; int Hs = 0, Ws = 0;          // (B,Hs,Ws,3)
  const uint8_t* labels = nullptr; int Hl = 0, Wl = 0;       // (B,Hl,Wl)
  const float* rois_raw = nullptr; int R = 0;                // (B,R,4)
  const float* sample = nullptr;                             // (B,5): vflip, hflip, roi_scale, cy, cx
  float mean[3] = {0.f, 0.f, 0.f}, std[3] = {1.f, 1.f, 1.f}; int x_min = 0, y_min = 0; int C = 0;   // C = cloth channels
  TView in_tex, tgt_tex;                                     // 4-channel NHWC views; tgt_tex may be empty (inference)
  TView cloth[3]; int ncloth = 0;                            // up to three one-hot destinations, C padded to a multiple of 4
  float* rois_out = nullptr;                                 // (B,R,4)
};
void texture_batch(Stream& s, const TextureBatchArgs& a);
// the argument checks of every texture_batch implementation (the HIP launcher and the host loop of engine.cpp)
inline void texture_batch_check(const TextureBatchArgs& a) {
  auto tileable = [](const TView& v) { return v.p && v.C % 4 == 0 && v.cs % 4 == 0 && v.cs >= v.C && !((uintptr_t)v.p & 15); };
  const TView& t = a.in_tex;
  if (!a.img || !a.labels || !a.rois_raw || !a.sample || !a.rois_out) throw Error(1, "texture_batch: NULL argument");
  if ((uintptr_t)a.rois_out & 15) throw Error(1, "texture_batch: rois_out not 16-byte aligned");
  if (t.N < 1 || t.H < 1 || t.W < 1 || a.Hs < 1 || a.Ws < 1 || a.Hl < 1 || a.Wl < 1 || a.R < 1) throw Error(1, "texture_batch: empty sizes");
  if (a.x_min < 0 || a.y_min < 0 || a.x_min > a.Ws - t.W || a.y_min > a.Hs - t.H)
    throw Error(1, "texture_batch: crop window (" + std::to_string(a.x_min) + ", " + std::to_string(a.y_min) + ") + " + std::to_string(t.W) +
                       " x " + std::to_string(t.H) + " lies outside the " + std::to_string(a.Ws) + " x " + std::to_string(a.Hs) + " source");
  if (a.C < 1 || a.C > 64) throw Error(1, "texture_batch: cloth channels in [1,64]");
  if (a.ncloth < 1 || a.ncloth > 3) throw Error(1, "texture_batch: one to three cloth destinations");
  if (!tileable(t) || t.C != 4) throw Error(1, "texture_batch in_tex: view not a 16-byte tileable 4-channel view");
  auto same = [&](const TView& v) { return v.N == t.N && v.H == t.H && v.W == t.W; };
  if (a.tgt_tex.p && (!tileable(a.tgt_tex) || a.tgt_tex.C != 4 || !same(a.tgt_tex))) throw Error(1, "texture_batch tgt_tex: view mismatch");
  for (int k = 0; k < a.ncloth; ++k)
    if (!tileable(a.cloth[k]) || a.cloth[k].C != round_up(a.C, 4) || !same(a.cloth[k])) throw Error(1, "texture_batch cloth: view mismatch");
}

// ---- Pillow's bilinear resize of uint8 RGB images (image_resize.hip) -----------------------------------------------------------
// Image.resize((Ws, Hs), Image.BILINEAR) of the reference's tf.resize(img, load_size) (datasets/texture_dataset.py:93-95,132-134)
// for a batch of decoded images of DIFFERENT sizes in one launch, byte for byte: Pillow's 8-bit resample (Resample.c), no box, no
// reducing_gap.  Per axis with source length `in` and output length `out`, in IEEE double, one rounded operation per step:
//   scale = (double)in / out;  fs = max(scale, 1.0);  support = 1.0 * fs;  ss = 1.0 / fs
//   center = (xx + 0.5) * scale
//   xmin = (int)(center - support + 0.5), at least 0;  xmax = (int)(center + support + 0.5), at most in;  n = xmax - xmin
//   w[x] = tri((x + xmin - center + 0.5) * ss), tri(a) = |a| < 1 ? 1 - |a| : 0;  ww = w[0] + w[1] + ... in index order;
//   w[x] /= ww where ww != 0;  k[x] = (int)(0.5 + w[x] * 4194304.0)                                    (22 fractional bits)
//   dst = clamp((2097152 + sum_x src[xmin + x] * k[x]) >> 22, 0, 255)                                   (int32)
// The horizontal pass runs first where Ws != W0 and leaves ROUNDED bytes (H0, Ws); the vertical pass runs on those where Hs != H0.  An
// axis whose length does not change is not resampled (here: the identity coefficients xmin = xx, n = 1, k = 1 << 22, which give
// the source byte back exactly).
// src: packed bytes; sample b is the (H0, W0, 3) image at byte `offset`, geom[b] = {offset, H0, W0} -- a HOST array, validated before
// anything is launched.  dst: (B, Hs, Ws, 3) dense.  BOUND: in <= 31 * out on both axes (windows of at most 63 taps: the
// coefficient and intermediate-row stages of a workgroup are static LDS); a larger reduction is refused by name.
constexpr int RESIZE_MAX_FACTOR = 31;
struct ResizeU8Args {
  const uint8_t* src = nullptr; size_t src_bytes = 0;
  const int64_t* geom = nullptr;                             // HOST (B,3): byte offset, H0, W0
  int B = 0, Hs = 0, Ws = 0;
  uint8_t* dst = nullptr;                                    // (B,Hs,Ws,3)
};
void resize_u8(Stream& s, const ResizeU8Args& a);
// the argument checks of every resize_u8 implementation (the HIP launcher and the host loop of engine.cpp): after it, no sample
// reaches outside [src, src + src_bytes) and every window fits the kernel's stages
inline void resize_u8_check(const ResizeU8Args& a) {
  if (!a.src || !a.geom || !a.dst) throw Error(1, "resize_u8: NULL argument");
  if (a.B < 1 || a.Hs < 1 || a.Ws < 1) throw Error(1, "resize_u8: empty sizes");
  for (int b = 0; b < a.B; ++b) {
    const int64_t off = a.geom[3 * b], h0 = a.geom[3 * b + 1], w0 = a.geom[3 * b + 2];
    const std::string who = "resize_u8: sample " + std::to_string(b);
    if (h0 < 1 || w0 < 1 || h0 > 0x7fffffff || w0 > 0x7fffffff)
      throw Error(1, who + " has an empty or oversized source (H0 " + std::to_string(h0) + ", W0 " + std::to_string(w0) + ")");
    const uint64_t bytes = 3ull * (uint64_t)h0 * (uint64_t)w0;           // < 3 * 2^62: no wrap
    if (off < 0 || (uint64_t)off > a.src_bytes || bytes > a.src_bytes - (uint64_t)off)
      throw Error(1, who + " runs past src_bytes (offset " + std::to_string(off) + " + " + std::to_string(bytes) + " > " + std::to_string(a.src_bytes) + ")");
    if (h0 > (int64_t)RESIZE_MAX_FACTOR * a.Hs || w0 > (int64_t)RESIZE_MAX_FACTOR * a.Ws)
      throw Error(1, who + " exceeds the reduction bound: " + std::to_string(h0) + " x " + std::to_string(w0) + " -> " + std::to_string(a.Hs) +
                         " x " + std::to_string(a.Ws) + " is more than " + std::to_string(RESIZE_MAX_FACTOR) + " to 1 on an axis");
  }
}

// ---- warp batch hand-over (warp_batch.hip) ------------------------------------------------------------------------------------
// What WarpDataset.__getitem__ (datasets/warp_dataset.py:139-183) computes per sample on the host, for a whole batch in ONE launch,
// from the compact form: the decoded uint8 HWC body image (not resized), the uint8 input and target label maps and the per-channel
// map table of affine_gather (B * C chains of nmaps rows {kind, c0..c7}).  With (y, x) a pixel of the H x W crop window at
// (y_min, x_min) of the Ls x Ls resized sample, sy = y_min + y, sx = x_min + x, and nearest(d) = min(int(floorf(d * (float(in) / Ls))),
// in - 1) (torch's nearest rule):
//   tgt_cloth[b,y,x,:] = one-hot of tgt_labels[b, nearest(sy), nearest(sx)]; label 0 and labels >= C give the all-zero vector
//   in_cloth[b,y,x,c]  = 1 if channel c's chain, walked backwards from (nearest(sy), nearest(sx)) exactly as affine_gather walks it
//                        (bounds Wl, Hl), stays inside and ends on a pixel whose in_labels value is c, c != 0; else 0
//                        (per_channel_transform of the one-hot map, F.interpolate nearest, crop -- the one-hot map never exists)
//   body[k][b,y,x,c]   = bilinear sample (align_corners False, torch's formula, below) of the texels
//                        (float(byte) / 255 - mean[c]) / std[c] of the Hb x Wb image at (sy, sx) of its Ls x Ls resize
//                        (ToTensor, Normalize, F.interpolate(size = Ls, mode = "bilinear"), crop)
//     src = max(scale * (d + 0.5f) - 0.5f, 0), scale = float(in) / Ls;  i0 = min(int(src), in - 1), i1 = i0 + (i0 < in - 1);
//     l1 = src - i0, l0 = 1 - l1;  v = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)
// all in fp32, one correctly rounded operation per step (no FMA contraction), pad channels of every view written as zero.
// tgt_labels may be in_labels (--dataset_mode image); tgt_cloth may be empty (inference: nothing of a target is read or written).
// Every view must be 16-byte tileable (C % 4, cs % 4, aligned base).
// `bicubic` says that the table may hold kind 3 (chain_resample above): in_cloth[b,y,x,c] is then channel c's chain evaluated by
// chain_resample's rule at (nearest(sy), nearest(sx)) of the Hl x Wl map, the texels being the indicators in_labels == c (0 for c = 0) --
// a float that need not be 0 or 1.  It selects another instantiation of the kernel; without it the launch is the one it always was and
// kind 3 must not occur.  The body and target outputs do not depend on it.
struct WarpBatchArgs {
  const uint8_t* body = nullptr; int Hb = 0, Wb = 0;                          // (B,Hb,Wb,3)
  const uint8_t* in_labels = nullptr; const uint8_t* tgt_labels = nullptr; int Hl = 0, Wl = 0;       // (B,Hl,Wl) each
  const double* maps = nullptr; int nmaps = 0;                                // [B*C][nmaps][9]; nmaps 0: no augmentation
  bool bicubic = false;                                                       // the table may hold kind 3
  float mean[3] = {0.f, 0.f, 0.f}, std[3] = {1.f, 1.f, 1.f}; int Ls = 0, x_min = 0, y_min = 0; int C = 0;   // C = cloth channels
  TView in_cloth, tgt_cloth;                                                  // C padded to a multiple of 4; tgt_cloth may be empty
  TView body_out[3]; int nbody = 0;                                           // one to three 4-channel destinations of the body
};
void warp_batch(Stream& s, const WarpBatchArgs& a);
// the argument checks of every warp_batch implementation (the HIP launcher and the host loop of engine.cpp)
inline void warp_batch_check(const WarpBatchArgs& a) {
  auto tileable = [](const TView& v) { return v.p && v.C % 4 == 0 && v.cs % 4 == 0 && v.cs >= v.C && !((uintptr_t)v.p & 15); };
  const TView& t = a.in_cloth;
  if (!a.body || !a.in_labels) throw Error(1, "warp_batch: NULL argument");
  if (a.tgt_cloth.p && !a.tgt_labels) throw Error(1, "warp_batch: a target destination but no target label map");
  if (a.nmaps < 0 || (a.nmaps > 0 && !a.maps)) throw Error(1, "warp_batch: " + std::to_string(a.nmaps) + " maps per channel but a NULL map table");
  if (t.N < 1 || t.H < 1 || t.W < 1 || a.Hb < 1 || a.Wb < 1 || a.Hl < 1 || a.Wl < 1 || a.Ls < 1) throw Error(1, "warp_batch: empty sizes");
  if (a.x_min < 0 || a.y_min < 0 || a.x_min > a.Ls - t.W || a.y_min > a.Ls - t.H)
    throw Error(1, "warp_batch: crop window (" + std::to_string(a.x_min) + ", " + std::to_string(a.y_min) + ") + " + std::to_string(t.W) +
                       " x " + std::to_string(t.H) + " lies outside the " + std::to_string(a.Ls) + " x " + std::to_string(a.Ls) + " source");
  if (a.C < 2 || a.C > 64) throw Error(1, "warp_batch: cloth channels in [2,64]");
  if (a.nbody < 1 || a.nbody > 3) throw Error(1, "warp_batch: one to three body destinations");
  if (!tileable(t) || t.C != round_up(a.C, 4)) throw Error(1, "warp_batch in_cloth: view not 16-byte tileable with the padded cloth channels");
  auto same = [&](const TView& v) { return v.N == t.N && v.H == t.H && v.W == t.W; };
  if (a.tgt_cloth.p && (!tileable(a.tgt_cloth) || a.tgt_cloth.C != t.C || !same(a.tgt_cloth))) throw Error(1, "warp_batch tgt_cloth: view mismatch");
  for (int k = 0; k < a.nbody; ++k)
    if (!tileable(a.body_out[k]) || a.body_out[k].C != 4 || !same(a.body_out[k])) throw Error(1, "warp_batch body: view mismatch");
}

// ---- saved-image visuals (image_out.hip) ------------------------------------------------------------------------------------------
// What inference.py does per image between a model's tensors and Image.fromarray -- unnormalize / scale_tensor(scale_each)
// (datasets/data_utils.py:41-90), decode_cloth_labels (util/decode_labels.py:24-55), draw_rois_on_texture (util/draw_rois.py:16-47)
// and util.tensor2im (util/util.py:9-32) -- for a whole batch: one NHWC view (or one label map) in, (B,H,W,3) interleaved bytes out.
//
// The 19 colours of util/decode_labels.py:8-21, one definition for every unit that holds them (gather.hip's decode_labels, image_out.hip
// and the host form in engine.cpp)
#define SWN_LABEL_PALETTE                                                                                                             \
  {0, 0, 0}, {128, 0, 0}, {255, 0, 0}, {0, 85, 0}, {255, 85, 0}, {0, 0, 85}, {0, 119, 221}, {85, 85, 0}, {0, 85, 85}, {85, 51, 0},    \
  {52, 86, 128}, {0, 128, 0}, {0, 0, 255}, {51, 170, 221}, {0, 255, 255}, {85, 255, 170}, {170, 255, 85}, {255, 255, 0}, {255, 170, 0}
constexpr int LABEL_PALETTE_SIZE = 19;
// Sources (one per call):
//   SRC_FLOAT   x has C = 3 logical channels, or C = 1 replicated to three (tensor2im's grayscale branch);
//   SRC_ARGMAX  x has C = number of labels; the first maximum over the channels selects a colour (argmax, then the palette);
//   SRC_LABELS  an int32 (B,H,W) map selects the colour.
// Palette sources write the palette's bytes; a label outside [0, 19) gives black.  (The reference passes decode_cloth_labels' uint8
// tensor through tensor2im's float formula, (x + 1) / 2 * 255 cast to uint8, which wraps modulo 256 -- numpy leaves that cast
// undefined, it is not reproducible and not reproduced.)
// Float sources, per element v of image b and channel c, every step ONE correctly rounded fp32 operation:
//   rows != NULL:  u = v * rows[b][c] + rows[b][C + c] (a product, then a sum: never fused); rows[b][2C] != 0: u = min(max(u, 0), 1)
//   scale_each:    lo / hi = min / max over the C LOGICAL channels of image b (pad channels of the view take no part);
//                  den = (float)((double)hi - (double)lo + 1e-5);  u = (min(max(v, lo), hi) + (-lo)) / den       (scale_tensor)
//   neither:       u = v                                                      (rows and scale_each together are refused)
//   RANGE_SIGNED:  byte = (u + 1) / 2 * 255       (tensor2im: also what the reference applies to its [0,1] visuals, whose saved
//   RANGE_UNIT:    byte = u * 255                  images therefore span 127..255)
// both saturated to [0, 255] and truncated: equal to numpy's astype(uint8) wherever that is defined ([0, 256)), the saturating value
// elsewhere.  A NaN anywhere in a float source leaves that pixel's bytes -- under scale_each the whole image's -- unspecified.
// The min / max reduction stays on the device: chunks = image_u8_chunks(H, W) <= 64 blocks per image leave wave-reduced partials in
// minmax[b][chunk][2] (caller's scratch, nothing of it needs initialising), the conversion kernel's waves finish it.  No atomics,
// no host read: capturable, and exact because min and max do not depend on the order.
// ROI outlines (R > 0), drawn over the converted bytes in the same pass: rois (B,R,4) = x0, y0, x1, y1, colours (R,3) bytes, both
// device arrays, width >= 1.  A pixel takes the colour of the LAST ROI whose outline covers it, as Pillow's sequential
// ImageDraw.rectangle(box, outline = colour, width = width) calls leave it (Draw.c ImagingDrawRectangle): coordinates truncate toward
// zero; rows y0 .. y0 + width - 1 and y1 - width + 1 .. y1 over columns x0 .. x1; columns x0 .. x0 + width - 1 and x1 - width + 1 .. x1
// over the rows from a = y0 + width towards e = y1 - width + 1, e itself excluded (a .. e - 1, or e + 1 .. a where a > e: a box flatter
// than twice the width paints below itself, the all-zero box with width 1 paints (0,0) and (0,1)); everything clipped to the image.
// x1 < x0 or y1 < y0 is Pillow's ValueError: the callers refuse such boxes before anything is launched.
enum ImageSource : int { SRC_FLOAT = 0, SRC_ARGMAX = 1, SRC_LABELS = 2 };
enum ImageRange : int { RANGE_SIGNED = 0, RANGE_UNIT = 1 };
constexpr int IMAGE_MAX_ROIS = 16, IMAGE_MAX_CHUNKS = 64;
struct ImageU8Args {
  int source = SRC_FLOAT;
  TView x; int C = 0;                                        // SRC_FLOAT / SRC_ARGMAX: the view and its logical channels
  const int32_t* labels = nullptr; int B = 0, H = 0, W = 0;  // SRC_LABELS: (B,H,W); the other sources take B, H, W from x
  const float* rows = nullptr;                               // device [B][2C + 1]: scale[C], shift[C], clamp flag
  int scale_each = 0; float* minmax = nullptr;               // device scratch [B][image_u8_chunks(H, W)][2]
  int range = RANGE_SIGNED;
  const float* rois = nullptr; int R = 0; const uint8_t* colours = nullptr; int width = 1;
  uint8_t* out = nullptr;                                    // (B,H,W,3)
};
inline int image_u8_chunks(int H, int W) {                   // 1024 pixels per block, at most one wave's worth of partials
  const size_t c = ((size_t)H * W + 1023) / 1024;
  return (int)(c < 1 ? 1 : (c > (size_t)IMAGE_MAX_CHUNKS ? IMAGE_MAX_CHUNKS : c));
}
void image_u8(Stream& s, const ImageU8Args& a);
// the argument checks of every image_u8 implementation (the HIP launcher and the host loop of engine.cpp); fills B, H, W from the view
inline ImageU8Args image_u8_check(ImageU8Args a) {
  if (!a.out) throw Error(1, "image_u8: NULL output");
  if (a.source == SRC_LABELS) {
    if (!a.labels) throw Error(1, "image_u8: SRC_LABELS without a label map");
  } else if (a.source == SRC_FLOAT || a.source == SRC_ARGMAX) {
    if (!a.x.p || a.x.cs < a.C) throw Error(1, "image_u8: empty view, or logical channels beyond the pixel stride");
    a.B = a.x.N; a.H = a.x.H; a.W = a.x.W;
    if (a.source == SRC_FLOAT && a.C != 3 && a.C != 1) throw Error(1, "image_u8: a float source has 3 channels, or 1 (grayscale), got " + std::to_string(a.C));
    if (a.source == SRC_ARGMAX && (a.C < 1 || a.C > 256)) throw Error(1, "image_u8: SRC_ARGMAX takes 1 to 256 label channels");
  } else {
    throw Error(1, "image_u8: source [" + std::to_string(a.source) + "] is not recognized (0 float, 1 argmax, 2 labels)");
  }
  if (a.B < 1 || a.H < 1 || a.W < 1) throw Error(1, "image_u8: empty sizes");
  if ((size_t)a.H * a.W > (size_t)1 << 28) throw Error(1, "image_u8: images of more than 2^28 pixels are not implemented");
  if (a.range != RANGE_SIGNED && a.range != RANGE_UNIT) throw Error(1, "image_u8: range [" + std::to_string(a.range) + "] is not recognized (0 signed, 1 unit)");
  if (a.source != SRC_FLOAT && (a.rows || a.scale_each)) throw Error(1, "image_u8: the affine table and scale_each apply to float sources only");
  if (a.rows && a.scale_each) throw Error(1, "image_u8: the affine table and scale_each exclude each other");
  if (a.scale_each && !a.minmax) throw Error(1, "image_u8: scale_each needs the min/max scratch");
  if (a.R < 0 || a.R > IMAGE_MAX_ROIS) throw Error(1, "image_u8: 0 to " + std::to_string(IMAGE_MAX_ROIS) + " ROIs per image, got " + std::to_string(a.R));
  if (a.R > 0 && (!a.rois || !a.colours)) throw Error(1, "image_u8: ROI outlines need the ROI table and the colour table");
  if (a.R > 0 && (a.width < 1 || a.width > (1 << 20))) throw Error(1, "image_u8: outline width in [1, 2^20]");
  return a;
}

// ---- PNG encoding of saved images (png_encode.hip, png_chunk.h) --------------------------------------------------------------------
// What util.save_image (util/util.py:54-69: Image.fromarray(a).save(path)) spends its time on -- PNG row filtering and deflate -- for n
// interleaved (H,W,3) uint8 images, the layout image_u8 writes: one zlib stream per image (RFC 1950) holding the filtered scanlines;
// the container around it (signature, IHDR, IDAT, IEND, CRC-32) is a few bytes of host work (util/png.py).  Two launches with fixed
// grids, nothing the host reads, no allocation: capturable.
//   chunk kernel, one workgroup per (image, R consecutive rows): adaptive filter per row (all five types, the smallest sum of
//     min(b, 256 - b) wins, ties to the lower type), run-length matches (distance 1 only, from a parallel scan of the run starts), one
//     dynamic-Huffman block per chunk, byte-aligned behind it by an empty stored block, or a stored block where that is not larger;
//   gather kernel, one workgroup per image: 78 01, the chunks back to back, the Adler-32 combined from the chunks' partials.
// R = rows_per_chunk, 0: min(16, 32768 / (1 + 3W)), at least 1.  W <= 2048 and R * (1 + 3W) <= 32768 (the chunk lives in LDS, its
// positions in two 64-bit masks per thread, and it fits one stored block); R is cut to H.  HIP kernels only: on the host simulator
// the launcher throws "not implemented".
struct PngGeom {
  int R = 0, chunks = 0, chunk_bytes = 0, last_bytes = 0;    // filtered bytes of a full chunk and of the image's last one
  size_t slot = 0;                                           // bytes between the chunk slots of the scratch (a multiple of 4)
  size_t bound = 0;                                          // no stream is longer: 2 + the chunk slots' capacities + 4
};
PngGeom png_geometry(int h, int w, int rows_per_chunk);      // throws Error(1, ...) on a shape the encoder refuses
inline size_t png_scratch_bytes(int n, const PngGeom& g) { return (size_t)n * g.chunks * (g.slot + 3 * sizeof(uint32_t)); }
struct PngEncodeArgs {
  const uint8_t* img = nullptr; int n = 0, h = 0, w = 0, rows_per_chunk = 0;
  void* scratch = nullptr;                                   // device, png_scratch_bytes, 4-byte aligned; nothing of it needs initialising
  uint8_t* streams = nullptr; size_t stream_stride = 0;      // device [n][stream_stride], stream_stride >= bound
  uint32_t* sizes = nullptr;                                 // device [n]: bytes of each stream
};
void png_encode(Stream& s, const PngEncodeArgs& a);

// ---- losses: each writes the plain MEAN loss into *loss_out (device float) and, if a grad
// view is given, scale * d(mean loss)/dx into it (scale carries lambda and the 0.5 of loss_D).
// Views and pad channels (tests/test_loss_ops.py asserts every line of this): the kernels take channel-slice views (cs >= C) and
// honour `accumulate` (dx += ..., else dx = ...).  They never read or write a channel at or above round_up(C, 4).  Channels in
// [C, round_up(C, 4)): ce_argmax_loss moves whole float4 groups -- it reads them (and ignores what it read) and WRITES ZEROS
// into those channels of dlogits (adds zero to them when it accumulates); l1_loss, gram_style_loss and the GAN losses (channel
// 0 of the map only) touch the C logical channels alone; normed_mse_loss and bias_grad require C % 4 == 0.
// All sums are fp64 partials of fp32 terms combined in a fixed order: two runs give bit-equal results.
// BCEWithLogits(pred, label) mean over N*H*W of channel 0;  dpred = scale*(sigmoid-t)/numel
// label_dev (optional): the label is read from device memory instead (captured training step)
void bce_logits_loss(Stream& s, const TView& pred, float label, float scale, float* loss_out,
                     const TView* dpred, const float* label_dev = nullptr);
void lsgan_loss(Stream& s, const TView& pred, float label, float scale, float* loss_out, const TView* dpred,
                const float* label_dev = nullptr);
void wgan_loss(Stream& s, const TView& pred, float sign, float scale, float* loss_out, const TView* dpred);
// CrossEntropy(logits, argmax_c(target)) mean over pixels; dlogits (+)= scale*(softmax-onehot)/P
void ce_argmax_loss(Stream& s, const TView& logits, const TView& target, int C, float scale,
                    float* loss_out, const TView* dlogits, int accumulate);
void l1_loss(Stream& s, const TView& a, const TView& b, int C, float scale, float* loss_out,
             const TView* da, int accumulate);
// content term of PerceptualLoss for one VGG slice: MSE of channel-L2-normalised features, y = x / (|x| + 1e-8) per pixel;
// C % 4 == 0, C <= 512.  df = g / (s + eps) - f (f.g) / (s (s + eps)^2), s = |f|, g = 2 scale (y_f - y_t) / numel.
// CONVENTION at a pixel with s == 0 (all-zero features, normal behind a ReLU): the second term is dropped, df = g / eps =
// -2 scale y_t / (numel * 1e-8), finite.  The reference program's autograd gives NaN there (sqrt'(0) * 0); the loss value agrees.
void normed_mse_loss(Stream& s, const TView& f, const TView& t, float scale, float* loss_out,
                     const TView* df, int accumulate);
// style term: scale * MSE(Gram(a), Gram(b)), Gram over (N*C) x (H*W) of the raw images; N*C <= 1024.  Gram entries are fp32 fmaf
// chains (64 pixels long when N*C <= 128 and the whole batch is differentiated, up to 1024 otherwise) added in fp64.
// Under data parallelism a, b are the GLOBAL batches (all ranks' images, gathered by the host) and the gradient is
// produced for the nloc samples starting at n0 only (da: a view of those samples); n0 = 0, nloc < 0: whole batch.
void gram_style_loss(Stream& s, const TView& a, const TView& b, int C, float scale, float* loss_out,
                     const TView* da, int accumulate, int n0 = 0, int nloc = -1);
// ---- gradient penalty (modules/loss.py:133-184; wgan-gp / dragan-gp / dragan-lp), see gp.cpp ---------------------
// x_hat = a + alpha[n] * (b - a) per sample n.  b = the second view (wgan: the conditioned fakes) or, when b is NULL
// (dragan), a + half_std[0] * beta with beta ~ U[0,1) the same shape as a (NHWC view; pad channels 0).
void gp_interpolate(Stream& s, const TView& a, const TView* b, const float* alpha, const TView* beta, const float* half_std,
                    const TView& out);
// out[0] = 0.5 * unbiased std of the `numel` logical elements of view a (pad channels hold zeros and add nothing)
void gp_half_std(Stream& s, const TView& a, size_t numel, float* out);
// per-sample L2 norm of g over all its elements; penalty = mean_n (norm_n - 1)^2 (lp != 0: max(0, norm_n - 1)^2);
// loss_out[0] = penalty, u = scale * d(penalty)/dg   (same geometry as g)
void gp_penalty(Stream& s, const TView& g, int lp, float scale, float* loss_out, const TView& u);
// fills a view with U[0,1) from the library's counter RNG: beta of dragan.  Channels c >= Clog and, when a device channel map
// is given (WShape::cimap of the layer that reads the buffer), channels with cimap[c] < 0 are layout pads and stay 0 -- a
// non-zero pad would reach the pad rows of the first conv's weight gradient.
void gp_uniform(Stream& s, const TView& v, int Clog, uint64_t seed, const int32_t* cimap = nullptr);
// Second-order step through y = act(InstanceNorm(x)) (reverse over reverse).  The first backward computed
// gx = IN'(x)^T (act'(xh) * gy).  Given u = adjoint of gx:  uy = act'(xh) * IN'(x) u   (adjoint of gy; IN' is symmetric)
// and ax = (d gx / d x)^T u (adjoint of the raw activation x):
//   ax = -rstd^2 [ xh (<u gm> - <u><gm> - <u xh><gm xh>) + <gm xh> (u - <u> - xh <u xh>) + <u xh> (gm - <gm> - xh <gm xh>) ],
//   gm = act'(xh) * gy, <.> = mean over the pixels of one (n, c) plane.  All reductions in fp64.
struct NormActBwd2Args {
  TView u, gy, x;             // adjoint of gx; gradient w.r.t. y from the first backward; raw activation
  const float* stats = nullptr;
  TView uy, ax;               // outputs (overwritten)
  int act = ACT_NONE;
};
void norm_act_bwd2(Stream& s, const NormActBwd2Args& a);

// out[0] = a[0]*ca + b[0]*cb (device scalars; used to combine loss terms without a sync)
void scalar_axpby(Stream& s, const float* a, float ca, const float* b, float cb, float* out);

// ---- SSIM and Charbonnier losses of modules.losses (ssim.hip, ssim_math.h) -------------------------------------------------------
// SSIM(window, reduction, max_val)(img1, img2) of modules/losses/__init__.py:128-259 on contiguous NCHW fp32 planes (the op is
// depthwise: each of the B*C planes on its own, no NHWC conversion): zero padding (window - 1) / 2, the float32 Gaussian of sigma
// 1.5 applied separably (rows, then columns: the reference's 2-D window up to rounding), loss = clamp(1 - S, 0, 1) / 2 (ssim_math.h
// has the arithmetic).  One fused launch plus the fixed-order finalize: a workgroup owns a 32 x 32 tile of one plane, stages the
// tile and its halo of both images in LDS with zeros outside the image, and no filtered map touches HBM.
//   loss_map (optional): the per-element loss, (B,C,H,W);  loss_sum: device float, the PLAIN sum over B*C*H*W (fp64 block partials of
//   fp32 terms combined in a fixed order: two runs give bit-equal results).
// Backward, when d1 or d2 is given: the upstream gradient is gmap (per element, reduction 'none') or, gmap NULL, the scalar gscalar
// (for 'mean' the caller passes g / numel).  The forward launch also leaves the four coefficient maps a1, a2, b, c of ssim_math.h in
// the stream's workspace, and a second launch filters them: d1 = f(a1) + 2 x f(b) + y f(c), d2 = f(a2) + 2 y f(b) + x f(c).
// The workspace must hold 4 * B*C*H*W floats plus one double per tile; a larger problem is refused by name.  window: odd, 1 ..
// SSIM_MAX_WINDOW.  Enqueued on s: no allocation, no synchronisation.
struct SsimArgs {
  const float* img1 = nullptr; const float* img2 = nullptr;
  int B = 0, C = 0, H = 0, W = 0, window = 0; float max_val = 1.f;
  float* loss_map = nullptr; float* loss_sum = nullptr;
  const float* gmap = nullptr; float gscalar = 0.f;
  float* d1 = nullptr; float* d2 = nullptr;
};
constexpr int SSIM_TILE = 32;
void ssim_loss(Stream& s, const SsimArgs& a);
// the argument checks of every ssim_loss implementation (the HIP launcher and the host loop of engine.cpp)
inline void ssim_check(const SsimArgs& a) {
  if (!a.img1 || !a.img2 || !a.loss_sum) throw Error(1, "ssim: NULL argument");
  if (a.B < 1 || a.C < 1 || a.H < 1 || a.W < 1) throw Error(1, "ssim: empty sizes");
  if (a.window < 1 || a.window % 2 == 0)
    throw Error(1, "ssim: kernel_size must be an odd positive integer. Got " + std::to_string(a.window));
  if (a.window > SSIM_MAX_WINDOW)
    throw Error(1, "ssim: windows larger than " + std::to_string(SSIM_MAX_WINDOW) + " are not implemented, got " + std::to_string(a.window));
  const size_t tiles = (size_t)ceil_div(a.H, SSIM_TILE) * ceil_div(a.W, SSIM_TILE) * a.B * a.C;
  if (tiles > 0x7fffffffull) throw Error(1, "ssim: more than 2^31 - 1 tiles");
}
// L1_Charbonnier_loss (modules/losses/__init__.py:14-27): loss_sum = sum sqrt((x - y)^2 + eps) over n elements of any shape, one
// launch plus the finalize, fp64 partials; dx = gscalar (x - y) / sqrt((x - y)^2 + eps), dy = -dx (each optional).
struct CharbonnierArgs {
  const float* x = nullptr; const float* y = nullptr; size_t n = 0; float eps = 1e-6f, gscalar = 0.f;
  float* loss_sum = nullptr; float* dx = nullptr; float* dy = nullptr;
};
void charbonnier_loss(Stream& s, const CharbonnierArgs& a);

// ---- optimizer / parameter layout ------------------------------------------------------
struct AdamWArgs {
  float* p; const float* g; float* m; float* v; size_t n;
  float lr, beta1, beta2, eps, weight_decay;
  int step;   // 1-based
  // optional (captured training step): {lr / (1 - beta1^step), 1 / sqrt(1 - beta2^step)} of THIS step in device memory, as
  // adamw_schedule computes them; `step` is then ignored
  const float* sched_dev = nullptr;
  // which update adamw_step applies: 0 = AdamW, 1 = AdaBound (Luo et al., ICLR 2019, as adabound 0.0.5 runs it with amsbound off;
  // reference optimizers/__init__.py:37-60).  AdaBound: weight_decay is the COUPLED L2 term (g += wd * p), the per-element rate
  // step_size / (sqrt(v) + eps) is clamped to [lower, upper] of adabound_schedule, and sched_dev holds that schedule's three values.
  int kind = 0;
  float final_lr = 0.1f, base_lr = 0.f, gamma = 1e-3f;   // AdaBound only; base_lr = the lr the optimizer was constructed with
};
enum OptKind : int { OPT_ADAMW = 0, OPT_ADABOUND = 1 };
void adamw_step(Stream& s, const AdamWArgs& a);
void adamw_schedule(float lr, float beta1, float beta2, int step, float out[2]);
// AdaBound's per-step scalars {step_size, lower, upper}, in double like adamw_schedule.  Defined here (not in a backend's
// translation unit) because the engine fills StepParams with it and every backend links the engine.
inline void adabound_schedule(float lr, float beta1, float beta2, float final_lr, float base_lr, float gamma, int step, float out[3]) {
  const double bc1 = 1.0 - std::pow((double)beta1, step);
  const double bc2 = 1.0 - std::pow((double)beta2, step);
  const double fin = (double)final_lr * (double)lr / (double)base_lr;
  out[0] = (float)((double)lr * std::sqrt(bc2) / bc1);
  out[1] = (float)(fin * (1.0 - 1.0 / ((double)gamma * step + 1.0)));
  out[2] = (float)(fin * (1.0 + 1.0 / ((double)gamma * step)));
}

enum WKind : int { WK_CONV = 0, WK_CONVT = 1 };
// Packed weight layouts (all [K][Npad], row-major):
//  conv  (Co,Ci,KH,KW) : k = (kh*KW+kw)*Cip + ci , n = co
//  convT (Ci,Co,4,4)   : 4 phase blocks p=(a*2+b) of k = (dy*2+dx)*Cip + ci , n = co,
//                        tap (ky,kx) = (3-a-2dy, 3-b-2dx)
struct WShape {
  int kind, Co, Ci, KH, KW, Cip, Npad;
  // optional device table [Cip]: buffer channel -> reference input channel (or -1 = zero pad);
  // used where the NHWC buffer orders a torch.cat differently (D's conditional input).
  const int32_t* cimap = nullptr;
};
size_t packed_elems(const WShape& w);
void pack_weight(Stream& s, const WShape& w, const float* nchw, float* packed);
void unpack_weight(Stream& s, const WShape& w, const float* packed, float* nchw);
// dgrad operand derived from the forward-packed weights.  mode:
//  0 conv stride-2 k4 : 4 phase blocks [ (dy*2+dx)*Cop + co ][ci]        (Ndg = Ci)
//  1 conv stride-1    : [ ((KH-1-kh)*KW + (KW-1-kw))*Cop + co ][ci]
//  2 convT k4 s2      : [ (ky*4+kx)*Cop + co ][ci]
//  3 tail (x2 nearest upsample + ZeroPad(1,0,1,0) + conv k4 p1): 5x5 stride-2 effective
//    kernel  [ (r*5+c)*Cop + co ][ci] = sum_{a-ky+3=r, b-kx+3=c; a,b in {0,1}} W[ky][kx]
void repack_dgrad(Stream& s, const WShape& w, int mode, int Cop, int Ndgpad, const float* packed, float* dg);
size_t dgrad_elems(const WShape& w, int mode, int Cop, int Ndgpad);
// Tail conv (x2 nearest upsample + ZeroPad(1,0,1,0) + conv k4 p1, swapnet_modules.py:85-90) folded
// onto the un-upsampled input: output phase (a,b) = (y&1, x&1) is a (2+a)x(2+b) conv with
// pre-summed taps  r(a,ky) = a ? (ky+1)>>1 : ky>>1  (25 instead of 64 taps per 2x2 outputs).
// Layout: 4 phase blocks p = a*2+b, each [ (r*(2+b)+c)*Cip + ci ][Npad], at tail_fold_offset(p).
size_t tail_fold_offset(const WShape& w, int phase);       // in floats; phase 4 = total size
void tail_fold_weights(Stream& s, const WShape& w, const float* packed, float* folded);
// inverse for the weight gradient: dW[ky][kx] = sum over the 4 phases of dWfold[p][r(a,ky)][c(b,kx)]
void tail_unfold_wgrad(Stream& s, const WShape& w, const float* dfolded, float* dpacked);

// ---- PatchGAN's 1-channel k4 s1 p1 head conv (modules/discriminators.py:131) as "taps on the N axis" ----
// An implicit GEMM with N = 1 reads every input element 16 times (once per tap) for one MAC each: it is
// bound by the load path.  Instead Z[q][t] = sum_c x[q][c] w[t][c] (a 1x1 conv, N = 16 taps, x read
// once), then y[n,oy,ox] = b + sum_{kh,kw} Z[n, oy-1+kh, ox-1+kw][4 kh + kw].  Backward uses the adjoint
// gather dZ[n,iy,ix][4 kh + kw] = dY[n, iy+1-kh, ix+1-kw], dW = X^T dZ, dX = dZ W.
// wt: [Cip][16], wt2: [16][Cip] (both derived from the packed [(t*Cip + c)][Npad] weight, column 0)
void head_pack(Stream& s, const WShape& w, const float* packed, float* wt, float* wt2);
void head_unpack_grad(Stream& s, const WShape& w, const float* dwt, float* dpacked);     // dpacked column 0; pads zeroed
void head_gather(Stream& s, const TView& z, const float* bias, const TView& y);          // z.C = 16, y = (N, H-1, W-1, 4)
void head_scatter(Stream& s, const TView& dy, const TView& dz);

}  // namespace swn
