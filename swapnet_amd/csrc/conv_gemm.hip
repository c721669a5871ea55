// swapnet_amd -- fp32 implicit-GEMM convolution for gfx950 (CDNA4).
//
// One kernel family serves every dense contraction of the SwapNet G+D step
// (reference: modules/layers.py:15,31,132,137; modules/discriminators.py:110-131;
// modules/swapnet_modules.py:85-90; modules/pix2pix_modules.py:216-246 and the autograd
// backward of each):
//   * conv_fwd_kernel   C[m][n] = sum_k A[m][k] W[k][n]   m = output pixel, k = (kh,kw,ci)
//       - Conv2d forward (k4s2p1, k3s1 reflect, k4s1p1, x2-upsampled tail conv)
//       - ConvTranspose2d k4s2p1 forward as 4 sub-pixel phases of a 2x2 conv (OutMap scatter)
//       - every dgrad (the transposed op is again a gather conv over dY with re-packed weights)
//   * conv_wgrad_kernel dW[k][n] = sum_m A[m][k] dY[m][n]  (reduction over pixels)
// A is never materialised: the im2col tile is gathered from the NHWC activation straight
// into LDS (16-byte loads along the channel axis = full 128-B lines per 8 lanes).
//
// CDNA4 mapping: v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD); workgroups of 4 wave64
// (128 x {192,128,64,32} tiles) or 8 wave64 (256 x 128), wave tile 64 x 64; BK = 32 per LDS stage,
// double-buffered LDS with the next stage prefetched into VGPRs while the current one feeds the
// matrix pipe (one barrier per stage).  A-tile rows are padded to 36 floats (16-byte aligned,
// conflict-free ds_read_b128 of a lane's 16 k-values, k order permuted inside the stage); the
// W / dY tile is read along its contiguous axis.  Launch modes: batched (Winograd planes), the four
// sub-pixel phases of a stride-2 scatter in one grid, deterministic split-K / split-M slabs chosen by
// a wave-quantisation cost model.  Narrow outputs (Cout <= 32) use v_mfma_f32_4x4x1 kernels (one
// pixel / one k-row per lane); the folded tail conv has fused 4-phase kernels.  See DESIGN.md 4.
// This file: launch parameters, schedule planners, the SWN_* switches and the dispatchers conv_fwd / conv_wgrad.  The kernels and
// their launchers: conv_direct.hip, conv_ring.hip, conv_tail.hip (conv_gemm.h lists what they share).
#include <cmath>
#include <cstdlib>

#include "conv_gemm.h"

namespace swn {

// ---------------------------------------------------------------------------------------
// launch parameters
// ---------------------------------------------------------------------------------------
static GemmP make_params(const TView& x, const Gather& g, const TView& y, OutMap om, int phases = 0, int batch = 1) {
  if (phases) {
    if (phases != 4 || batch > 1 || om.ymul != 2 || om.xmul != 2) throw Error(1, "conv: bad sub-pixel phase launch");
    om.yoff = om.xoff = 1;               // bounds check below against the farthest phase
  }
  if (x.C % 4 || x.cs % 4 || y.cs % 4) throw Error(1, "conv: channel counts/strides must be multiples of 4");
  if (((uintptr_t)x.p & 15) || ((uintptr_t)y.p & 15)) throw Error(1, "conv: views must be 16-byte aligned");
  GemmP p{};
  p.x = x.p; p.xH = x.H; p.xW = x.W; p.xC = x.C; p.xcs = x.cs;
  p.KH = g.KH; p.KW = g.KW; p.stride = g.stride; p.pad_t = g.pad_t; p.pad_l = g.pad_l;
  p.pad_mode = g.pad_mode; p.ups = g.ups; p.Ho = g.Ho; p.Wo = g.Wo;
  p.M = x.N * g.Ho * g.Wo;
  p.K = g.KH * g.KW * x.C;
  p.y = y.p; p.yH = y.H; p.yW = y.W; p.ycs = y.cs; p.yC = y.C;
  p.ymul = om.ymul; p.yoff = om.yoff; p.xmul = om.xmul; p.xoff = om.xoff;
  p.splits = 1; p.per_split = 1 << 30;
  p.phases = phases;
  if (phases) p.yoff = p.xoff = 0;
  if ((g.Ho - 1) * om.ymul + om.yoff >= y.H || (g.Wo - 1) * om.xmul + om.xoff >= y.W || y.N != x.N)
    throw Error(1, "conv: output map exceeds the output view");
  return p;
}
// the operands every forward-type / weight-gradient launch takes from its arguments (batch strides: the dispatchers)
GemmP fwd_params(const ConvFwdArgs& a, const OutMap& om) {
  GemmP p = make_params(a.x, a.g, a.y, om, a.phases, a.batch);
  p.w = a.w; p.Npad = a.Npad; p.bias = a.bias; p.act = a.act; p.accumulate = a.accumulate; p.Cout = a.Cout;
  return p;
}
GemmP wgrad_params(const ConvWgradArgs& a, const OutMap& om) {
  GemmP p = make_params(a.x, a.g, a.dy, om, a.phases, a.batch);
  p.w = a.dw; p.Npad = a.Npad; p.Cout = a.Cout;
  return p;
}

// ---------------------------------------------------------------------------------------
// schedule planners
// ---------------------------------------------------------------------------------------
// Wave-quantisation-aware split factor.  `ntiles` output tiles, each `work` reduction steps
// long, run on `slots` concurrently resident workgroups (CUs x workgroups/CU).  A tile count just
// above a multiple of `slots` leaves most of the chip idle in the last round (e.g. 576 wgrad
// tiles of a resblock conv on 512 slots = 56 % efficiency); splitting the reduction s ways
// trades that for s slabs summed by a cheap second kernel.  Cost model: rounds x (steps per
// block + fixed prologue/epilogue) + slab traffic.
int choose_splits(int ntiles, int work, int slots, int min_work, size_t slab_bytes, size_t ws_bytes) {
  int best = 1;
  double best_cost = 1e300;
  const int max_s = std::max(1, std::min(512, work / std::max(min_work, 1)));
  for (int sp = 1; sp <= max_s; ++sp) {
    if (sp > 1 && slab_bytes * sp > ws_bytes) break;
    const int per = ceil_div(work, sp);
    const int eff = ceil_div(work, per);
    const double rounds = std::ceil((double)ntiles * eff / slots);
    double cost = rounds * (per + 4.0);
    if (eff > 1) cost += 0.02 * eff * ((double)ntiles / slots) + 1.0;   // slab write + reduce launch
    if (cost < best_cost * 0.97) { best_cost = cost; best = eff; }
  }
  return best;
}

// ---- LDS-DMA ring kernels: schedule -----------------------------------------------------------------------------------------
// T tiles of `work` stages on `slots` resident workgroups.  Whole rounds run one tile per unit; the remainder tiles
// (all tiles when T < slots) are split s ways along K so that the last round is as full as the others.
// `unit` = stage-time of this tile configuration relative to the 128x128 one (waves per SIMD / 3); *cost_out receives the
// estimated launch time in 128x128 stage units, comparable across tile configurations.
DmaSched plan_dma(int tiles_total, int tiles_per_z, int work, int slots, size_t tile_bytes, size_t ws_bytes, double* cost_out, double unit) {
  DmaSched sc{};
  sc.tiles_per_z = tiles_per_z;
  const int rounds = tiles_total / slots;
  int rem = tiles_total - rounds * slots;
  sc.full = rounds * slots; sc.tail_tiles = rem; sc.tail_s = 1; sc.per_split = work;
  if (cost_out) *cost_out = rounds * (work + 4.0) * unit;
  if (rem == 0) return sc;
  // A remainder behind at least one whole round runs UN-SPLIT (round 5).  The two-plane loops are bound by the chip's power, not
  // by issue (tools/tile_lab.hip: 1.13-1.24 GHz at > 85 % matrix-pipe occupancy on random operands, 2.1-2.4 GHz for the same
  // launch with the matrix instructions removed): a last round that occupies few CUs runs at nearly twice the clock, and the
  // split's slab round trip + reduce launch cost what it saves (36 Winograd planes of 512 x 1024 x 1024 = 1152 tiles on 1024
  // slots: 128 us un-split in the lab, 135 + 13 us split in the product; whole C2 step -0.29 ms, profiles/native_ab_r05.txt).
  // The same holds for a launch that fills at least half of the slots (two workgroups per CU in the 4-per-CU configuration): in the
  // lab 512 / 768 / 1024 tiles of the resblock shape take 51 / 72 / 95 us un-split -- the same 340-360 fp32-equivalent TFLOP/s, at
  // 1.51 / 1.36 / 1.10 GHz -- so splitting K to "fill the chip" buys nothing there either (below half, a CU runs too few waves to
  // keep its matrix pipe fed and the split still pays: 128 tiles 33 us).  SWN_TAIL_SPLIT=0 restores every split, =2 only the
  // behind-a-whole-round rule (A/B; read per launch).
  {
    const int mode = env_int(getenv("SWN_TAIL_SPLIT"), 1);
    if (mode != 0 && (rounds >= 1 || (mode == 1 && 2 * rem >= slots))) {
      sc.full = tiles_total; sc.tail_tiles = 0;
      if (cost_out) *cost_out += (work + 4.0) * unit * (rounds >= 1 ? 0.6 : (double)rem / slots);
      return sc;
    }
  }
  // cost in units of one stage-time of a resident workgroup (32 MFMAs per wave, three waves sharing a SIMD: ~2.7 us):
  // tail rounds x (stages per unit + ~4 of prologue / epilogue) + the slab round trip of the split tiles at ~5 TB/s
  // (13.5 MB per unit) + the reduce launch.  Calibrated on the Winograd-plane launches of the warp step (M 800 x 36
  // planes: 3 whole rounds 0.559 ms, 2 + a 3-way split tail 0.535 ms).
  int best = 1;
  double best_cost = 1e300;
  const int max_s = std::max(1, std::min(1024, work / 8));
  for (int sp = 1; sp <= max_s; ++sp) {
    if (sp > 1 && (size_t)rem * sp * tile_bytes > ws_bytes) break;
    const int per = ceil_div(work, sp), eff = ceil_div(work, per);
    const double tail_rounds = std::ceil((double)rem * eff / slots);
    double cost = tail_rounds * (per + 4.0);
    if (eff > 1) cost += (double)rem * eff * (double)tile_bytes * 2.0 / (13.5e6 * unit) + 2.0;
    if (cost < best_cost * 0.985) { best_cost = cost; best = eff; }
  }
  if (cost_out) *cost_out += best_cost * unit;
  sc.tail_s = best;
  sc.per_split = ceil_div(work, best);
  sc.tail_s = ceil_div(work, sc.per_split);
  if (sc.tail_s == 1) { sc.full = tiles_total; sc.tail_tiles = 0; }
  return sc;
}

// ---------------------------------------------------------------------------------------
// SWN_* switches.  Read once per process where a model is built around the answer, per launch where tests and A/B runs toggle it.
// ---------------------------------------------------------------------------------------
bool prof_detail() {
  static const bool on = getenv("SWN_PROF_DETAIL") != nullptr;
  return on || route_on();
}
// read per launch (tests and A/B measurements toggle it): 0 = v_mfma_f32_32x32x2_f32 main loop, default = bf16 split
bool split_on() { return env_on(getenv("SWN_SPLIT")); }
static bool dma_on() {
  static const bool on = env_on(getenv("SWN_DMA"));
  return on;
}

static int g_force_naive = 0;
void conv_force_naive(int on) { g_force_naive = on; }

// SWN_AMAX_FUSED=0: every launch takes the amax of its operands itself (A/B against the producer-side slots; read per launch)
bool amax_fused_on() { return env_on(getenv("SWN_AMAX_FUSED")); }
// SWN_PRECUT=0: no pre-cut ring kernel.  Read ONCE per process, here and by conv_precut_tile alike: the engine decides at build time
// which weight operands exist only in pre-cut form, and a launch that changed its mind later would run a fall-back on operands
// prepared for the pre-cut kernel (or fail at a model's epilogue statistics)
static bool pc_on() {
  static const bool on = env_on(getenv("SWN_PRECUT"));
  return on;
}
// 2 (default): two fp16 planes per operand, three MFMAs per product; 1: the reduced-precision configuration (one fp16 plane per
// operand, one MFMA: bench.py --precision f16, never the headline).  Read once: the operands a model holds are cut for one form.
static int pc_planes() {
  static const int pl = env_int(getenv("SWN_PC_PLANES"), 2) == 1 ? 1 : 2;
  return pl;
}
int conv_precut_planes() { return pc_planes(); }
bool wino_pair_planes() {
  static const bool on = env_on(getenv("SWN_PAIR"));
  return on && pc_planes() == 2 && dma_on() && split_on() && !g_force_naive && amax_fused_on();
}
static bool narrow_on() { return env_on(getenv("SWN_NARROW")); }      // read per launch: tests toggle it
static bool tail4_on() { return env_on(getenv("SWN_TAIL4")); }        // read per launch, by both dispatchers
// 2 (default): the weight-gradient ring kernel on two fp16 planes per operand, both scaled by powers of two from their amax (three
// MFMAs per product; tools/ring_lab.hip variants 18 / 19: 157-167 -> 266-268 fp32-equivalent TFLOP/s at 4.5e-7); 1: the
// reduced-precision configuration (one plane, bench.py --precision f16).  Read per launch (tests).
int wgrad_planes() { return env_int(getenv("SWN_WGRAD_PLANES"), 2) == 1 ? 1 : 2; }

// ---------------------------------------------------------------------------------------
// forward-type launches
// ---------------------------------------------------------------------------------------
// column tile of the pre-cut kernel by output width: 64 (256 x 64), 128 (128 x 128), or 192 for N in (128, 192] (the tail
// conv's input gradient into the 192-channel concat: one 128 x 192 tile instead of two 128-wide ones of which one is half empty)
static int pc_tile_for(int Npad) { return Npad <= 64 ? 64 : ((Npad > 128 && Npad <= 192) ? 192 : 128); }
int conv_fwd_stat_chunk(int xC, int Npad, int HoWo, int nimg, int K) {
  using T = PcTile<PC128_WGM, PC128_NB, PC128_NSTG>;       // the launch these statistics come out of
  if (pc_planes() != 2 || !pc_on() || conv_precut_tile(xC, Npad) != T::BN || Npad <= 64 || HoWo % T::BM || K % T::BK) return 0;
  // only where the launch runs every tile WHOLE anyway (C2 bs 32: 1024 / 2048 tiles; C3 bs 16: 512): the statistics come out of the
  // tile epilogue, and forcing a launch the planner would split along K onto whole tiles would trade its shorter fp32 accumulation
  // chains for one of K / 16 x 3 MFMAs per output -- measured on the MI355X at bs 2: the normalised output 4.3e-7 instead of 2.5e-7 from
  // float64, and the pinned gradients of the texture U-Net's deep levels 1e-4 instead of 2e-5 (tools/r06_stats_probe.py)
  const int tiles = (int)((size_t)nimg * HoWo / T::BM) * ceil_div(Npad, T::BN);
  const DmaSched sc = plan_pc<T, PC128_WGCU>(tiles, 1, K, (size_t)1 << 30);
  if (sc.tail_tiles > 0 && sc.tail_s > 1) return 0;
  return T::BM;
}
// ops.h: which column tile a forward-type launch over an input with xC channels into Npad columns wants its weight operand
// pre-cut for (0 = the launch does not take the pre-cut ring kernel: no operand needs to be produced)
int conv_precut_tile(int xC, int Npad) {
  if (!pc_on() || g_force_naive || !dma_on() || !split_on() || xC % 16 || Npad <= 32) return 0;
  return pc_tile_for(Npad);
}

// ConvFwdArgs::y_amax on a launch whose kernel has no folding epilogue: a pass over the output view
static void fold_output_amax(Stream& s, const ConvFwdArgs& a) {
  amax_partials(s, a.y.p, a.y.pixels(), a.y.C, (size_t)a.y.cs, 1, 0, a.y_amax, 1);
}

// the LDS-DMA kernel addresses activations through 32-bit buffer offsets and marks padding with offsets >= 2^31
static bool dma_ok(const ConvFwdArgs& a, const GemmP& p) {
  if (!dma_on() || a.x.C % 16 || a.Npad <= 32) return false;
  const size_t xbytes = (size_t)a.x.N * a.x.H * a.x.W * a.x.cs * 4, wbytes = (size_t)p.K * a.Npad * 4;
  return xbytes < ((size_t)1 << 31) && wbytes < ((size_t)1 << 31);
}

// per-phase form of a tail4 launch (ops.h): the reference path and the fallback of the fused kernels
template <class Args>
static Args tail_phase_args(const Args& a, int ph) {
  Args c = a;
  c.tail4 = 0;
  c.g.KH = 2 + (ph >> 1); c.g.KW = 2 + (ph & 1); c.g.stride = 1; c.g.pad_t = 1; c.g.pad_l = 1;
  c.om.ymul = 2; c.om.xmul = 2; c.om.yoff = ph >> 1; c.om.xoff = ph & 1;
  return c;
}
static size_t tail_panel_off(int ph, int xC, int Npad) {
  const int pre = ph == 0 ? 0 : (ph == 1 ? 4 : (ph == 2 ? 10 : 16));
  return (size_t)pre * xC * Npad;
}
static void check_tail4(const Gather& g, const OutMap& om, int batch, int phases) {
  if (g.KH != 3 || g.KW != 3 || g.stride != 1 || g.pad_t != 1 || g.pad_l != 1 || g.ups || g.pad_mode != PAD_ZERO ||
      om.ymul != 2 || om.xmul != 2 || batch > 1 || phases)
    throw Error(1, "conv: bad tail4 launch");
}
// column groups of 4 of the narrow kernels (v_mfma_f32_4x4x1) for a width of at most 32
static int narrow_groups(int Npad) { return Npad <= 4 ? 1 : (Npad <= 8 ? 2 : (Npad <= 16 ? 4 : (Npad <= 20 ? 5 : (Npad <= 24 ? 6 : 8)))); }

void conv_fwd(Stream& s, const ConvFwdArgs& a) {
  if (a.tail4) {
    check_tail4(a.g, a.om, a.batch, a.phases);
    if (g_force_naive || !tail4_on() || a.x.C % 32 || a.Npad > 20 || a.accumulate) {
      for (int ph = 0; ph < 4; ++ph) {
        ConvFwdArgs c = tail_phase_args(a, ph);
        c.w = a.w + tail_panel_off(ph, a.x.C, a.Npad);
        conv_fwd(s, c);
      }
      return;
    }
    OutMap om = a.om; om.yoff = om.xoff = 1;          // bounds check against the farthest phase
    GemmP p = fwd_params(a, om);
    p.tail4 = 1;
    launch_tail_fwd4(s, p);
    return;
  }
  if (g_force_naive) { conv_fwd_naive(s, a); if (a.y_amax) fold_output_amax(s, a); return; }
  GemmP p = fwd_params(a, a.om);
  p.y_amax = a.y_amax;
  p.stat = a.stat_partial;
  if (a.stat_partial && !(a.wpc && pc_planes() == 2 && pc_on() && a.Npad > 64 && (a.g.Ho * a.g.Wo) % 128 == 0 && a.wpc_bn == 128 && !a.phases && a.batch <= 1))
    throw Error(1, "conv_fwd: stat_partial on a launch outside the 128 x 128 pre-cut kernel");
  if (a.Npad % 4 || a.Cout > a.Npad) throw Error(1, "conv_fwd: bad Npad/Cout");
  if (a.accumulate && a.act != ACT_NONE) throw Error(1, "conv_fwd: accumulate with activation");
  const bool fast = (a.x.C % 32) == 0;
  p.x_bs = a.x_bs; p.w_bs = a.w_bs; p.y_bs = a.y_bs;
  const int nb = a.phases ? a.phases : std::max(a.batch, 1);
  if (dma_ok(a, p)) {
    // weight operand handed over pre-cut (conv_precut) for this launch's column tile: the round-3 kernel
    if (a.wpc && pc_on() && split_on() && a.wpc_bn == pc_tile_for(a.Npad) &&
        (size_t)(p.K / 16) * ceil_div(a.Npad, a.wpc_bn) * 12 * a.wpc_bn * 8 < ((size_t)1 << 31)) {
      const int bn = a.wpc_bn == 192 ? 192 : (a.Npad > 64 ? 128 : 64);
      // (the one-plane kernels have no pair-form instantiation: the operand is never stored in pairs then, wino_pair_planes)
      launch_fwd_pc(s, p, bn, pc_planes(), nb, a.wpc, a.wpc_bs, a.phases != 0, a.x_amax, pc_planes() == 2 ? a.x_pair_k : nullptr);
      return;
    }
    if (!a.w) throw Error(1, "conv_fwd: the weight operand exists in pre-cut form only, but this launch cannot take the pre-cut "
                             "kernel (SWN_SPLIT / SWN_PRECUT / SWN_DMA must not change after a model is built)");
    if (a.x_pair_k) throw Error(1, "conv_fwd: pair-form operand on a launch outside the pre-cut ring kernel");
    p.y_amax = nullptr;
    if (a.Npad > 64) {
      // 128 x 128 (4 waves, 3 workgroups / CU) unless the 128 x 256 tile (8 waves, 2 / CU: 512 slots instead of 768)
      // quantises the launch better: the resblock input gradient (M 800, N 1024 x 36 planes) is 2016 tiles = 2.6
      // rounds of 768 but 1008 = 1.97 rounds of 512
      const int wide = env_int(getenv("SWN_DMA_WIDE"), 1);   // 0 never, 1 by cost, 2 always (tests); per launch
      double c22 = 0, c24 = 0;
      // (with the split main loop the 8-wave tile spills at its 128-VGPR budget and measures slower: f32-MFMA form only)
      if (wide && (wide == 2 || !split_on()) && a.Npad % 256 == 0) { plan_fwd_dma<2, 2>(p, nb, s.ws_bytes, &c22); plan_fwd_dma<2, 4>(p, nb, s.ws_bytes, &c24); }
      if (c24 > 0 && (wide == 2 || c24 < 0.95 * c22)) launch_fwd_dma(s, p, RING_128x256, nb);
      else launch_fwd_dma(s, p, RING_128x128, nb);
    }
    else launch_fwd_dma(s, p, RING_256x64, nb);
    if (a.y_amax) fold_output_amax(s, a);
    return;
  }
  if (!a.w) throw Error(1, "conv_fwd: pre-cut-only weight operand on a launch outside the ring kernel's shapes");
  if (a.x_pair_k) throw Error(1, "conv_fwd: pair-form operand on a launch outside the pre-cut ring kernel");
  p.y_amax = nullptr;
  // every register-staged route: the amax of the output, if asked for, by a pass behind the launch
  // N in (128, 192] (the tail conv's input gradient into the 192-channel concat): a 128x192 tile instead
  // of two 128-wide column tiles of which the second is half empty
  if (a.Npad > 128 && a.Npad <= 192) launch_fwd_direct(s, p, FWD_128x192, fast, nb);
  else if (a.Npad > 64 && fast && p.M >= 2048) launch_fwd_direct(s, p, FWD_256x128, fast, nb);
  else if (a.Npad > 64) launch_fwd_direct(s, p, FWD_128x128, fast, nb);
  else if (a.Npad > 32) launch_fwd_direct(s, p, FWD_128x64, fast, nb);
  else if (!narrow_on()) launch_fwd_direct(s, p, FWD_128x32, fast, nb);
  // (SWN_PHASE4=0, read per launch: one narrow launch per phase, as before round 5)
  else if (a.phases == 4 && a.Npad <= 20 && p.KH == 2 && p.KW == 2 && p.stride == 1 && !p.ups && p.pad_mode == PAD_ZERO && a.x.C % 16 == 0 &&
           env_on(getenv("SWN_PHASE4")))
    launch_fwd_phase4(s, p, narrow_groups(a.Npad));
  else launch_fwd_narrow(s, p, narrow_groups(a.Npad), fast, nb);
  if (a.y_amax) fold_output_amax(s, a);
}

// ---------------------------------------------------------------------------------------
// weight-gradient launches
// ---------------------------------------------------------------------------------------
// the ring kernel's k-tile is 128 rows (N > 64) or 256 rows (N <= 64): shapes that would leave a quarter or more of the tile rows
// empty (the K = 64 / 320 / 384 first-layer weight gradients) stay on the 128-row register-staged kernel
// (128-row tiles from 0.75: K = 192, the tail conv's Winograd-domain weight gradient, is 1.5 tiles of a long reduction).
// One rule for the engine's build-time question (conv_wgrad_takes_pairs) and the launch: a layer must not store pair-form planes
// that the launcher then refuses.
static bool wgrad_ring_fills(int K, int Npad) {
  const int bmk = Npad > 64 ? 128 : 256;
  const double fillf = (double)K / (double)(ceil_div(K, bmk) * bmk);
  return fillf > 0.8 || (bmk == 128 && fillf >= 0.75);
}
// ops.h: would a batched plane launch with these dimensions take the kernels that read pair-form operands?  (The engine decides the
// storage form of a layer's Winograd planes with these when the layer is built; the launchers re-check and throw on a mismatch.)
bool conv_fwd_takes_pairs(int xC, int Npad) { return wino_pair_planes() && conv_precut_tile(xC, Npad) != 0; }
bool conv_wgrad_takes_pairs(size_t T, int K, int Npad) {
  if (!wino_pair_planes() || wgrad_planes() != 2 || Npad <= 32 || K % 4 || Npad % 4 || T % 16 || T * (size_t)std::max(K, Npad) * 4 >= ((size_t)1 << 31))
    return false;
  return wgrad_ring_fills(K, Npad);
}
// stage geometry the LDS-DMA wgrad kernel needs: 16 consecutive pixels inside one image at fixed offsets from the first
static bool wgrad_dma_ok(const ConvWgradArgs& a, const GemmP& p) {
  if (!dma_on() || a.Npad <= 32 || a.dy.C % 4 || a.x.C % 4) return false;
  const bool geom = (p.Wo % 16 == 0) || (16 % p.Wo == 0 && (p.Ho * p.Wo) % 16 == 0);
  const size_t xbytes = (size_t)a.x.N * a.x.H * a.x.W * a.x.cs * 4, ybytes = (size_t)a.dy.N * a.dy.H * a.dy.W * a.dy.cs * 4;
  return geom && wgrad_ring_fills(p.K, a.Npad) && p.M % 16 == 0 && xbytes < ((size_t)1 << 31) && ybytes < ((size_t)1 << 31);
}

void conv_wgrad(Stream& s, const ConvWgradArgs& a) {
  if (a.tail4) {
    check_tail4(a.g, a.om, a.batch, a.phases);
    if (g_force_naive || !tail4_on() || a.x.C != 192 || a.Npad > 20 || a.g.Wo % 16 || a.g.Wo != a.x.W || a.g.Ho != a.x.H) {
      for (int ph = 0; ph < 4; ++ph) {
        ConvWgradArgs c = tail_phase_args(a, ph);
        c.dw = a.dw + tail_panel_off(ph, a.x.C, a.Npad);
        conv_wgrad(s, c);
      }
      return;
    }
    OutMap om = a.om; om.yoff = om.xoff = 1;
    GemmP p = wgrad_params(a, om);
    p.tail4 = 1;
    launch_tail_wgrad4(s, p);
    return;
  }
  if (g_force_naive) { conv_wgrad_naive(s, a); return; }
  GemmP p = wgrad_params(a, a.om);
  if (a.Npad % 4 || a.Cout > a.Npad || a.dy.C % 4) throw Error(1, "conv_wgrad: bad Npad/Cout");
  p.x_bs = a.x_bs; p.y_bs = a.dy_bs; p.w_bs = a.dw_bs;
  const int nb = a.phases ? a.phases : std::max(a.batch, 1);
  if (wgrad_dma_ok(a, p)) {
    launch_wgrad_dma(s, p, a.Npad > 64 ? RING_128x128 : RING_256x64, nb, a);
    return;
  }
  if (a.x_pair_k || a.dy_pair_k) throw Error(1, "conv_wgrad: pair-form operands on a launch outside the ring kernel");
  // 8-wave 256x128 tile: +3 % on the single-GEMM layers, -7 % on the batched Winograd planes (measured)
  if (a.Npad > 64 && p.K >= 512 && nb == 1) launch_wgrad_direct(s, p, WGRAD_256x128, nb);
  else if (a.Npad > 64) launch_wgrad_direct(s, p, WGRAD_128x128, nb);
  else if (a.Npad > 32) launch_wgrad_direct(s, p, WGRAD_128x64, nb);
  // narrow variant only where it measured faster (N <= 8: PatchGAN's 1-channel head); at N = 19 both
  // forms are bound by the im2col load path (2 N FLOP per loaded float), not by the matrix pipe
  else if (narrow_on() && a.Npad <= 4) launch_wgrad_direct(s, p, WGRAD_256x4, nb);
  else if (narrow_on() && a.Npad <= 8) launch_wgrad_direct(s, p, WGRAD_256x8, nb);
  else launch_wgrad_direct(s, p, WGRAD_128x32, nb);
}

}  // namespace swn
