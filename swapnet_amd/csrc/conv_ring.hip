// swapnet_amd -- implicit-GEMM convolution on the LDS-DMA ring: the forward-type kernel on fp32 operands, the one that takes its
// weight operand pre-cut, the producer of that operand and the operand amax pass, and the weight-gradient kernel.  Forward and
// weight gradient share this unit on purpose: between them they call scale_exp (conv_gemm.h) with both PC_TOP_A and PC_TOP_B.  In a
// unit that sees one of the two only, the optimiser folds the constant into the function before it is inlined, and the two-plane
// kernels come out as a different (equivalent) instruction sequence than the one that was measured (tools/isa_diff.py).
// Overview: conv_gemm.hip; shared: conv_gemm.h.
#include "conv_gemm.h"

namespace swn {

// ---------------------------------------------------------------------------------------
// forward-type kernel, LDS-DMA ring (round 2).  Same contraction as conv_fwd_kernel<FAST>, different machine:
//   * global -> LDS by `buffer_load_dwordx4 ... lds` (no staging VGPRs, no ds_write pass); padding taps and rows past M
//     are fetched OUT OF RANGE of the buffer descriptor, which the hardware returns as zeros;
//   * BK = 16, three LDS stages, two of them in flight across every barrier (counted s_waitcnt vmcnt, raw s_barrier);
//   * 64-byte A rows XOR-swizzled on the SOURCE side (lane l of a row fetches chunk (l & 3) ^ ((row >> 2) & 3)) so that
//     the 16-lane groups of ds_read_b128 touch 16 distinct 4-bank groups: conflict-free without padding;
//   * B fragments are ds_read_b64 of two ADJACENT columns, i.e. a lane's two 32x32 MFMA blocks hold columns
//     (2c, 2c+1) of its wave's 64 -> the epilogue stores float2 (256 contiguous bytes per row and wave);
//   * ~95 VGPRs: three 4-wave workgroups (128x128 tile, 48 KB) per CU = three independent waves per SIMD, so one
//     workgroup's barrier / epilogue / prologue is covered by the MFMAs of the other two.  (The register-staged
//     256x128 kernel above runs ONE 8-wave workgroup per CU -- 194 VGPRs, 105 KB -- and idles the matrix pipe a third
//     of the time; measured on the Winograd-plane and k4s2 shapes of this model: 87-105 -> 104-144 TFLOP/s.)
// The LDS-DMA is issued from an asm statement on purpose: hipcc's waitcnt pass puts `s_waitcnt vmcnt(0)` in front of every
// ds_read that follows an LDS-DMA *builtin* (one pending LDS write = "may alias"), which drains the ring each stage.
// Scheduling: tiles beyond a whole number of chip-fills ("the tail round") are split along K so that the last round is
// as full as the others (hybrid data-parallel / split-K); their partial tiles go to a compact slab that
// conv_dma_reduce_kernel sums in fixed order (deterministic) and finishes with the usual epilogue.
// ---------------------------------------------------------------------------------------
template <int WGM, int WGN, bool SPLIT>
// (hipcc's second launch-bound is waves per SIMD: the 8-wave tile needs 2 workgroups = 4 waves per SIMD, <= 128 VGPRs)
__global__ __launch_bounds__(64 * WGM * WGN, (WGM * WGN >= 8 ? 4 : 3)) void conv_fwd_dma_kernel(GemmP p, DmaSched sc) {
#if defined(__HIP_DEVICE_COMPILE__)
  using T = DmaTile<WGM, WGN>;
  constexpr int BM = T::BM, BN = T::BN, BK = T::BK, NST = T::NST, AI = T::AI, BI = T::BI;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wid / WGN, wn = wid % WGN;

  // ---- work unit -> (tile, K range)
  int u = blockIdx.x, gtile, split = 0, nsplit = 1, tt = 0;
  if (u < sc.full) {
    gtile = xcd_swizzle(u, sc.full);
  } else {
    u -= sc.full;
    tt = u / sc.tail_s; split = u - tt * sc.tail_s; nsplit = sc.tail_s;
    gtile = sc.full + tt;
  }
  const int z = gtile / sc.tiles_per_z, tile = gtile - z * sc.tiles_per_z;
  const int tile_n = tile % p.tiles_n, tile_m = tile / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  p.x += (size_t)z * p.x_bs; p.w += (size_t)z * p.w_bs; p.y += (size_t)z * p.y_bs;
  if (p.phases) { const int a = z >> 1, b = z & 1; p.pad_t -= a; p.pad_l -= b; p.yoff = a; p.xoff = b; }
  const int nkb_all = p.K / BK;
  const int kb_begin = nsplit > 1 ? split * sc.per_split : 0;
  const int kb_end = nsplit > 1 ? min(nkb_all, kb_begin + sc.per_split) : nkb_all;

  const unsigned x_bytes = (unsigned)((((size_t)p.xH * p.xW * (size_t)(p.M / (p.Ho * p.Wo)) - 1) * p.xcs + p.xC) * 4);
  const i32x4 rsA = make_rsrc(p.x, x_bytes), rsB = make_rsrc(p.w, (unsigned)((size_t)p.K * p.Npad * 4));
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;

  // ---- loader state.  A: this lane owns AI rows (row = 16 q + lane / 4, q = wid * AI + r) and one swizzled chunk of each.
  int a_iy0[AI], a_ix0[AI], a_base[AI];
  unsigned a_voff[AI], b_voff[BI];
  const int HoWo = p.Ho * p.Wo;
  const int He = p.xH << p.ups, We = p.xW << p.ups;
#pragma unroll
  for (int r = 0; r < AI; ++r) {
    const int row = 16 * (wid * AI + r) + (lane >> 2);
    const int m = m0 + row;
    if (m < p.M) {
      const int n = m / HoWo, rem = m - n * HoWo;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      a_iy0[r] = oy * p.stride - p.pad_t;
      a_ix0[r] = ox * p.stride - p.pad_l;
      a_base[r] = n * p.xH * p.xW * p.xcs + 4 * ((lane & 3) ^ ((row >> 2) & 3));     // + inverse-swizzled chunk
    } else {
      a_iy0[r] = 0; a_ix0[r] = 0; a_base[r] = -1;
    }
  }
#pragma unroll
  for (int r = 0; r < BI; ++r) {
    const int krow = T::RPI * (wid * BI + r) + lane / T::LPR;
    const int nn = n0 + 4 * (lane % T::LPR);
    b_voff[r] = nn < p.Npad ? (unsigned)(krow * p.Npad + nn) * 4u : DMA_OOB;
  }
  auto set_tap = [&](int tap) {
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
#pragma unroll
    for (int r = 0; r < AI; ++r) {
      unsigned off = DMA_OOB;
      if (a_base[r] >= 0) {
        const int sy = src_coord(a_iy0[r] + kh, He, p.pad_mode, p.ups);
        const int sx = src_coord(a_ix0[r] + kw, We, p.pad_mode, p.ups);
        if (sy >= 0 && sx >= 0) off = (unsigned)(a_base[r] + (sy * p.xW + sx) * p.xcs) * 4u;
      }
      a_voff[r] = off;
    }
  };
  // stages are issued strictly in order kb_begin, kb_begin + 1, ...: (tap, ci) of the next stage to issue
  int ld_tap = (kb_begin * BK) / p.xC, ld_ci = kb_begin * BK - ld_tap * p.xC;
  set_tap(ld_tap);
  auto issue = [&](int st, int kb) {
    const unsigned As = lds0 + (unsigned)(st * T::ST_FL) * 4u, Bs = As + T::A_FL * 4u;
#pragma unroll
    for (int r = 0; r < AI; ++r) lds_dma16(a_voff[r], rsA, (unsigned)ld_ci * 4u, As + (unsigned)(wid * AI + r) * 1024u);
#pragma unroll
    for (int r = 0; r < BI; ++r)
      lds_dma16(b_voff[r], rsB, (unsigned)kb * (unsigned)(BK * 4) * (unsigned)p.Npad, Bs + (unsigned)(wid * BI + r) * 1024u);
    ld_ci += BK;
    if (ld_ci >= p.xC) { ld_ci = 0; ld_tap += 1; if (ld_tap < p.KH * p.KW) set_tap(ld_tap); }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int h = lane >> 5, l31 = lane & 31;
  const int f = (l31 >> 2) & 3;
  const int a_rd = (wm * 64 + l31) * BK;
  const int a_c0 = ((2 * h) ^ f) * 4, a_c1 = ((2 * h + 1) ^ f) * 4;
  const int b_rd = T::A_FL + (8 * h) * BN + wn * 64 + 2 * l31;
  // k order inside a stage: step s multiplies k = s (lanes 0-31) and k = 8 + s (lanes 32-63)
  auto compute = [&](int st) {
    const float* S = smem + st * T::ST_FL;
    float af[2][8], bf[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float4 v0 = *reinterpret_cast<const float4*>(S + a_rd + i * 32 * BK + a_c0);
      const float4 v1 = *reinterpret_cast<const float4*>(S + a_rd + i * 32 * BK + a_c1);
      af[i][0] = v0.x; af[i][1] = v0.y; af[i][2] = v0.z; af[i][3] = v0.w;
      af[i][4] = v1.x; af[i][5] = v1.y; af[i][6] = v1.z; af[i][7] = v1.w;
    }
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) {
      const float2 b = *reinterpret_cast<const float2*>(S + b_rd + s8 * BN);
      bf[0][s8] = b.x; bf[1][s8] = b.y;
    }
    if (SPLIT) {
      split_mma_2x2(acc, af, bf);
    } else {
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s8], bf[j][s8], acc[i][j], 0, 0, 0);
    }
  };

  if (kb_begin < kb_end) {
    issue(0, kb_begin);
    if (kb_begin + 1 < kb_end) issue(1, kb_begin + 1);
    int st = 0;
    for (int kb = kb_begin; kb < kb_end; ++kb) {
      // this wave's share of stage kb has landed: only the next stage's AI + BI loads may still be in flight
      if (kb + 1 < kb_end) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(AI + BI) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();          // everybody's share landed; everybody finished reading stage kb - 1
      asm volatile("" ::: "memory");
      int st2 = st + 2; if (st2 >= NST) st2 -= NST;
      if (kb + 2 < kb_end) issue(st2, kb + 2);         // overwrites the stage read in iteration kb - 1
      compute(st);
      st = st + 1 == NST ? 0 : st + 1;
    }
  }

  // ---- epilogue.  lane: columns (c, c+1) = n0 + wn*64 + 2*l31 + {0,1}; rows wm*64 + i*32 + (e&3) + 8*(e>>2) + 4*h
  const int colr = wn * 64 + 2 * l31;                   // column inside the tile
  if (nsplit > 1) {
    float* slab = p.slab + ((size_t)(tt * nsplit + split) * BM) * BN;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        *reinterpret_cast<float2*>(slab + (size_t)row * BN + colr) = make_float2(acc[i][0][e], acc[i][1][e]);
      }
    return;
  }
  __syncthreads();                                      // the ring is dead: reuse it for the per-row output offsets
  int* rowoff = reinterpret_cast<int*>(smem);
  if (t < BM) {
    const int m = m0 + t;
    int off = -1;
    if (m < p.M) {
      const int n = m / HoWo, rem = m - n * HoWo;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      off = ((n * p.yH + oy * p.ymul + p.yoff) * p.yW + ox * p.xmul + p.xoff) * p.ycs;
    }
    rowoff[t] = off;
  }
  __syncthreads();
  const int col = n0 + colr;
  const bool c0ok = col < p.Cout, c1ok = col + 1 < p.Cout;
  float b0 = 0.f, b1 = 0.f;
  if (p.bias) { if (c0ok) b0 = p.bias[col]; if (c1ok) b1 = p.bias[col + 1]; }
  if (c0ok) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int off = rowoff[wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h];
        if (off < 0) continue;
        float v0 = act_apply(acc[i][0][e] + b0, p.act), v1 = act_apply(acc[i][1][e] + b1, p.act);
        float* dst = p.y + (size_t)off + col;
        if (c1ok) {
          if (p.accumulate) { const float2 o = *reinterpret_cast<const float2*>(dst); v0 += o.x; v1 += o.y; }
          *reinterpret_cast<float2*>(dst) = make_float2(v0, v1);
        } else {
          if (p.accumulate) v0 += *dst;
          *dst = v0;
        }
      }
  }
#endif
}

// sums the partial tiles of the split tail in fixed order and applies the epilogue; one float4 of a tile row per thread
template <int BM, int BN>
__global__ __launch_bounds__(256) void conv_dma_reduce_kernel(GemmP p, DmaSched sc) {
  const int tt = blockIdx.y;
  const int e4 = blockIdx.x * 256 + threadIdx.x;
  if (e4 >= BM * BN / 4) return;
  const int r = e4 / (BN / 4), c4 = (e4 - r * (BN / 4)) * 4;
  const int gtile = sc.full + tt;
  const int z = sc.zfast ? gtile % sc.zfast : gtile / sc.tiles_per_z, tile = sc.zfast ? gtile / sc.zfast : gtile - z * sc.tiles_per_z;
  const int tile_n = tile % p.tiles_n, tile_m = tile / p.tiles_n;
  const int m = tile_m * BM + r, col = tile_n * BN + c4;
  if (m >= p.M || col >= p.Cout) return;
  p.y += (size_t)z * p.y_bs;
  if (p.phases) { p.yoff = z >> 1; p.xoff = z & 1; }
  const float* sl = p.slab + ((size_t)tt * sc.tail_s * BM + r) * BN + c4;
  float4 a = *reinterpret_cast<const float4*>(sl);
  for (int s = 1; s < sc.tail_s; ++s) {
    const float4 b = *reinterpret_cast<const float4*>(sl + (size_t)s * BM * BN);
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  }
  float v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p.bias && col + j < p.Cout) v[j] += p.bias[col + j];
    v[j] = act_apply(v[j], p.act);
  }
  const int HoWo = p.Ho * p.Wo;
  const int n = m / HoWo, rem = m - n * HoWo;
  const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
  float* dst = p.y + (size_t)((n * p.yH + oy * p.ymul + p.yoff) * p.yW + ox * p.xmul + p.xoff) * p.ycs + col;
  float am = 0.f;
  if (col + 3 < p.Cout) {
    float4 o = make_float4(v[0], v[1], v[2], v[3]);
    if (p.accumulate) {
      const float4 old = *reinterpret_cast<const float4*>(dst);
      o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
    }
    *reinterpret_cast<float4*>(dst) = o;
    am = f4amax(o);
  } else {
    for (int j = 0; j < 4 && col + j < p.Cout; ++j) { const float o = p.accumulate ? dst[j] + v[j] : v[j]; dst[j] = o; am = fmaxf(am, fabsf(o)); }
  }
  // (threads that returned above hold nothing: a per-thread atomic with the pre-check costs a load for all but a few)
  if (p.y_amax && am > 0.f) amax_store(am, p.y_amax, blockIdx.x + blockIdx.y * gridDim.x);
}


// ---------------------------------------------------------------------------------------
// forward-type kernel on the LDS-DMA ring with the weight operand PRE-CUT (round 3).  conv_fwd_dma_kernel<SPLIT> spends
// 176 of its ~290 instructions per wave and 16-k stage cutting fragments, and half of that on the WEIGHT fragment: the same
// bf16 pieces of the same weights, recomputed by every workgroup of every launch.  Here whoever produces the weight operand
// (conv_precut after an optimizer step / a re-pack) hands it over as three bf16 planes already in MFMA operand order, and
// the waves are laid out WGM x 1: each wave owns 32 rows x ALL BN columns of the tile, so ONE activation-fragment cut (44
// VALU) feeds 6 NB MFMAs, the B fragments are plain ds_read_b128 (no VALU), and a wave only ever reads the A rows it
// fetched itself.  ~115 instructions per wave-stage instead of ~290 (tools/ring_lab.hip, same box, fp32-equivalent TFLOP/s:
// Winograd planes 157 -> 179, 8192x512x4096 133 -> 169, 131072x128x1024 163 -> 190, 131072x64x1536 (256 x 64 tile) 96 -> 139).
// Pre-cut layout (conv_precut): Wp[stage = k / 16][tile_n][kq 2][plane 3][pos BN][8 k] bf16, pos = (n % NB) * 32 + n / NB
// inside a BN-column tile: the lane at position l31 of column block j holds column NB * l31 + j, i.e. NB adjacent columns
// over its NB accumulators -> 16-byte epilogue stores.  One (stage, tile_n) block is 12 * BN / 128 contiguous KiB = the
// LDS image of the stage, fetched by plain consecutive 1-KiB LDS-DMA pieces.
// Everything else (gather through out-of-range zero fill, XOR-swizzled A rows, hybrid split-K schedule, epilogue) is
// conv_fwd_dma_kernel's.
// ---------------------------------------------------------------------------------------
// 256 partial maxima of |x| over [batch][rows][C] (row stride rs, batch stride bs floats; C % 4 == 0, 16-byte aligned rows).
// 256 blocks x 1024 threads, four independent 16-byte loads in flight per thread (64 KB per CU); `flat`: the region is one
// dense array of `total4` float4s (no index arithmetic).  No atomics: the consumers reduce the 256 partials themselves.
__device__ __forceinline__ float amax4(const float4& v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }
// fold != 0: the block maxima are folded into the slot `out` (atomic max, hip_util.h amax_store) instead of overwriting it;
// floor: a value the result is at least (a known bound of what another producer writes into the same buffer)
__global__ __launch_bounds__(1024) void amax_partials_kernel(const float* x, size_t rows, int C4, size_t rs, int batch, size_t bs, int flat,
                                                             float* out, int fold, float floor) {
  const size_t total = (size_t)batch * rows * C4;
  constexpr size_t S = (size_t)256 * 1024;
  float m = floor;
  auto at = [&](size_t i) -> const float4* {
    if (flat) return reinterpret_cast<const float4*>(x) + i;
    const size_t r = i / C4; const int c = (int)(i - r * C4);
    const size_t b = r / rows, rr = r - b * rows;
    return reinterpret_cast<const float4*>(x + b * bs + rr * rs + 4 * c);
  };
  size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x;
  for (; i + 3 * S < total; i += 4 * S) {
    const float4 v0 = *at(i), v1 = *at(i + S), v2 = *at(i + 2 * S), v3 = *at(i + 3 * S);
    m = fmaxf(m, fmaxf(fmaxf(amax4(v0), amax4(v1)), fmaxf(amax4(v2), amax4(v3))));
  }
  for (; i < total; i += S) m = fmaxf(m, amax4(*at(i)));
#pragma unroll
  for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float red[16];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x < 16) {
    float r = red[threadIdx.x];
#pragma unroll
    for (int o = 8; o; o >>= 1) r = fmaxf(r, __shfl_xor(r, o));
    if (threadIdx.x == 0) {
      if (fold) amax_store(r, out, blockIdx.x);
      else out[blockIdx.x] = r;
    }
  }
}

// WGCU = workgroups per CU the tile is sized for (LDS) -> waves per SIMD the register allocation must allow
// APAIR: the activation operand arrives in pair form (a_kscale = the exponent its producer scaled it by): no cut in the loop
template <int WGM, int NB, int NSTG, int WGCU, int PL, bool APAIR = false>
__global__ __launch_bounds__(64 * WGM, WGCU * WGM / 4) void conv_fwd_pc_kernel(GemmP p, DmaSched sc, const unsigned short* wpc, size_t wpc_bs,
                                                                               const float* a_amax, const int* a_kscale) {
#if defined(__HIP_DEVICE_COMPILE__)
  using T = PcTile<WGM, NB, NSTG, PL>;
  constexpr int BM = T::BM, BN = T::BN, BK = T::BK, NST = T::NST, AI = T::AI, BI = T::BI, BREM = T::BREM;
  extern __shared__ __attribute__((aligned(16))) char smem_c[];
  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);

  // ---- work unit -> (tile, K range)
  int u = blockIdx.x, gtile, split = 0, nsplit = 1, tt = 0;
  if (u < sc.full) {
    gtile = xcd_swizzle(u, sc.full);
  } else {
    u -= sc.full;
    tt = u / sc.tail_s; split = u - tt * sc.tail_s; nsplit = sc.tail_s;
    gtile = sc.full + tt;
  }
  const int z = sc.zfast ? gtile % sc.zfast : gtile / sc.tiles_per_z, tile = sc.zfast ? gtile / sc.zfast : gtile - z * sc.tiles_per_z;
  const int tile_n = tile % p.tiles_n, tile_m = tile / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  p.x += (size_t)z * p.x_bs; p.y += (size_t)z * p.y_bs;
  wpc += (size_t)z * wpc_bs;
  if (p.phases) { const int a = z >> 1, b = z & 1; p.pad_t -= a; p.pad_l -= b; p.yoff = a; p.xoff = b; }
  const int nkb_all = p.K / BK;
  const int kb_begin = nsplit > 1 ? split * sc.per_split : 0;
  const int kb_end = nsplit > 1 ? min(nkb_all, kb_begin + sc.per_split) : nkb_all;

  const unsigned x_bytes = (unsigned)((((size_t)p.xH * p.xW * (size_t)(p.M / (p.Ho * p.Wo)) - 1) * p.xcs + p.xC) * 4);
  const unsigned b_stage = (unsigned)p.tiles_n * T::B_BYTES;        // bytes of one 16-k stage of the pre-cut panel
  const i32x4 rsA = make_rsrc(p.x, x_bytes), rsB = make_rsrc(wpc, (unsigned)nkb_all * b_stage);
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem_c;
  // two-plane form: the power-of-two operand scales (A from the partial maxima of this launch, B from the panel's trailer)
  int kA = 0, kB = 0;
  {
    if constexpr (APAIR) kA = __builtin_amdgcn_readfirstlane(*a_kscale);
    else kA = __builtin_amdgcn_readfirstlane(scale_exp(amax256(a_amax, lane), PC_TOP_A));
    kB = *reinterpret_cast<const int*>(wpc + (size_t)nkb_all * (b_stage / 2));
  }
  const float sa = pow2f(kA);

  // ---- loader state.  A: this lane owns AI rows of its OWN wave's 32 (row = 32 wid + 16 r + lane / 4) and one swizzled chunk.
  int a_iy0[AI], a_ix0[AI], a_base[AI];
  unsigned a_voff[AI];
  const int HoWo = p.Ho * p.Wo;
  const int He = p.xH << p.ups, We = p.xW << p.ups;
#pragma unroll
  for (int r = 0; r < AI; ++r) {
    const int row = 16 * (wid * AI + r) + (lane >> 2);
    const int m = m0 + row;
    if (m < p.M) {
      const int n = m / HoWo, rem = m - n * HoWo;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      a_iy0[r] = oy * p.stride - p.pad_t;
      a_ix0[r] = ox * p.stride - p.pad_l;
      a_base[r] = n * p.xH * p.xW * p.xcs + 4 * ((lane & 3) ^ ((row >> 2) & 3));
    } else {
      a_iy0[r] = 0; a_ix0[r] = 0; a_base[r] = -1;
    }
  }
  auto set_tap = [&](int tap) {
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
#pragma unroll
    for (int r = 0; r < AI; ++r) {
      unsigned off = DMA_OOB;
      if (a_base[r] >= 0) {
        const int sy = src_coord(a_iy0[r] + kh, He, p.pad_mode, p.ups);
        const int sx = src_coord(a_ix0[r] + kw, We, p.pad_mode, p.ups);
        if (sy >= 0 && sx >= 0) off = (unsigned)(a_base[r] + (sy * p.xW + sx) * p.xcs) * 4u;
      }
      a_voff[r] = off;
    }
  };
  int ld_tap = (kb_begin * BK) / p.xC, ld_ci = kb_begin * BK - ld_tap * p.xC;
  set_tap(ld_tap);
  const bool extra = BREM > 0 && wid < BREM;
  const unsigned b_voff = (unsigned)lane * 16u;
  const unsigned b_tile = (unsigned)tile_n * T::B_BYTES;
  auto issue = [&](int st, int kb) {
    const unsigned S = lds0 + (unsigned)(st * T::ST_BYTES), SB = S + T::A_BYTES;
    const unsigned bsrc = (unsigned)kb * b_stage + b_tile;
#pragma unroll
    for (int r = 0; r < AI; ++r) lds_dma16c(a_voff[r], rsA, (unsigned)ld_ci * 4u, S + (unsigned)(wid * AI + r) * 1024u);
#pragma unroll
    for (int r = 0; r < BI; ++r) lds_dma16c(b_voff, rsB, bsrc + (unsigned)(wid * BI + r) * 1024u, SB + (unsigned)(wid * BI + r) * 1024u);
    if (extra) lds_dma16c(b_voff, rsB, bsrc + (unsigned)(WGM * BI + wid) * 1024u, SB + (unsigned)(WGM * BI + wid) * 1024u);
    ld_ci += BK;
    if (ld_ci >= p.xC) { ld_ci = 0; ld_tap += 1; if (ld_tap < p.KH * p.KW) set_tap(ld_tap); }
  };

  f32x16 acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  const int h = lane >> 5, l31 = lane & 31;
  const int f = (l31 >> 2) & 3;
  const int a_rd = (wid * 32 + l31) * 64;
  const int a_c0 = ((2 * h) ^ f) * 16, a_c1 = ((2 * h + 1) ^ f) * 16;
  const int b_rd = T::A_BYTES + (h * PL * BN + l31) * 16;                  // + (plane * BN + 32 j) * 16
  auto compute = [&](int st) {
    const char* S = smem_c + st * T::ST_BYTES;
    float af[8];
    {
      const float4 v0 = *reinterpret_cast<const float4*>(S + a_rd + a_c0);
      const float4 v1 = *reinterpret_cast<const float4*>(S + a_rd + a_c1);
      af[0] = v0.x; af[1] = v0.y; af[2] = v0.z; af[3] = v0.w; af[4] = v1.x; af[5] = v1.y; af[6] = v1.z; af[7] = v1.w;
    }
    if constexpr (PL == 1) {
      u32x4 bh[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) bh[j] = *reinterpret_cast<const u32x4*>(S + b_rd + (32 * j) * 16);
      u32x4 ah;
      split8h1(af, sa, ah);
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[j] = mma_f16(ah, bh[j], acc[j]);
      return;
    }
    if constexpr (PL == 2) {
      u32x4 bh[NB], bl[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        bh[j] = *reinterpret_cast<const u32x4*>(S + b_rd + (0 * BN + 32 * j) * 16);
        bl[j] = *reinterpret_cast<const u32x4*>(S + b_rd + (1 * BN + 32 * j) * 16);
      }
      u32x4 ah, al;
      if constexpr (APAIR) pair8(af, ah, al);
      else split8h(af, sa, ah, al);
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        f32x16 c = acc[j];
        c = mma_f16(al, bh[j], c); c = mma_f16(ah, bl[j], c); c = mma_f16(ah, bh[j], c);          // smallest terms first
        acc[j] = c;
      }
      return;
    }
    static_assert(PL == 1 || PL == 2, "one or two fp16 planes");
  };

  if (kb_begin < kb_end) {
#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
      if (kb_begin + s < kb_end) issue(s, kb_begin + s);
    int st = 0;
    for (int kb = kb_begin; kb < kb_end; ++kb) {
      // this wave's share of stage kb has landed: only the (at most NST - 2) younger stages may still be in flight
      const int younger = min(NST - 2, kb_end - 1 - kb);
      if (extra) {
        if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * (AI + BI + 1)) : "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(AI + BI + 1) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else {
        if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * (AI + BI)) : "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(AI + BI) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();          // everybody's share of B landed; everybody finished reading stage kb - 1
      asm volatile("" ::: "memory");
      int stn = st + NST - 1; if (stn >= NST) stn -= NST;
      if (kb + NST - 1 < kb_end) issue(stn, kb + NST - 1);
      compute(st);
      st = st + 1 == NST ? 0 : st + 1;
    }
  }

  {                                                       // remove the operand scales (two exact power-of-two factors)
    const float ca = pow2f(-kA), cb = pow2f(-kB);
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][e] = (acc[j][e] * ca) * cb;
  }
  // ---- epilogue.  lane: rows wid*32 + (e&3) + 8*(e>>2) + 4*h, columns n0 + NB*l31 + j
  const int colr = NB * l31;
  if (nsplit > 1) {
    float* slab = p.slab + ((size_t)(tt * nsplit + split) * BM) * BN;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wid * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      float* dst = slab + (size_t)row * BN + colr;
      if constexpr (NB == 4) *reinterpret_cast<float4*>(dst) = make_float4(acc[0][e], acc[1][e], acc[2][e], acc[3][e]);
      else {
#pragma unroll
        for (int j = 0; j < NB; j += 2) *reinterpret_cast<float2*>(dst + j) = make_float2(acc[j][e], acc[j + 1][e]);
      }
    }
    return;
  }
  __syncthreads();                                      // the ring is dead: reuse it for the per-row output offsets
  int* rowoff = reinterpret_cast<int*>(smem_c);
  if (t < BM) {
    const int m = m0 + t;
    int off = -1;
    if (m < p.M) {
      const int n = m / HoWo, rem = m - n * HoWo;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      off = ((n * p.yH + oy * p.ymul + p.yoff) * p.yW + ox * p.xmul + p.xoff) * p.ycs;
    }
    rowoff[t] = off;
  }
  __syncthreads();
  const int col = n0 + colr;
  float am = 0.f;
  if (col < p.Cout) {
    float bj[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) bj[j] = (p.bias && col + j < p.Cout) ? p.bias[col + j] : 0.f;
    const bool full = col + NB - 1 < p.Cout;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int off = rowoff[wid * 32 + (e & 3) + 8 * (e >> 2) + 4 * h];
      if (off < 0) continue;
      float v[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) v[j] = act_apply(acc[j][e] + bj[j], p.act);
      float* dst = p.y + (size_t)off + col;
      if (full) {
        if constexpr (NB == 4) {
          float4 o = make_float4(v[0], v[1], v[2], v[3]);
          if (p.accumulate) { const float4 q = *reinterpret_cast<const float4*>(dst); o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w; }
          *reinterpret_cast<float4*>(dst) = o;
          am = fmaxf(am, f4amax(o));
        } else {
#pragma unroll
          for (int j = 0; j < NB; j += 2) {
            float2 o = make_float2(v[j], v[j + 1]);
            if (p.accumulate) { const float2 q = *reinterpret_cast<const float2*>(dst + j); o.x += q.x; o.y += q.y; }
            *reinterpret_cast<float2*>(dst + j) = o;
            am = fmaxf(am, fmaxf(fabsf(o.x), fabsf(o.y)));
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < NB; ++j)
          if (col + j < p.Cout) { const float o = p.accumulate ? dst[j] + v[j] : v[j]; dst[j] = o; am = fmaxf(am, fabsf(o)); }
      }
    }
  }
  if (p.y_amax) amax_fold_wave(am, p.y_amax, blockIdx.x * WGM + wid);        // (every wave arrives here converged)
  if constexpr (WGM == 4 && NB == 4) {
    // Conv + InstanceNorm fusion (modules/layers.py:12-24): the statistics' partial sums of this tile's 128 output rows (one image:
    // the launcher checked Ho * Wo % 128 == 0), per column, in fp64 -- lane: 16 rows x 4 columns, then the two half-waves (rows
    // + 4 h), then the four waves through LDS in wave order.  Fixed order: run-to-run identical.  What is summed is what was stored.
    if (p.stat) {
      double sm[NB], sq[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) { sm[j] = 0.0; sq[j] = 0.0; }
      if (col < p.Cout) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          if (rowoff[wid * 32 + (e & 3) + 8 * (e >> 2) + 4 * h] < 0) continue;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const double v = (col + j < p.Cout) ? (double)(acc[j][e] + ((p.bias && col + j < p.Cout) ? p.bias[col + j] : 0.f)) : 0.0;
            sm[j] += v; sq[j] += v * v;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) { sm[j] += __shfl_xor(sm[j], 32); sq[j] += __shfl_xor(sq[j], 32); }
      __syncthreads();                                    // rowoff is dead
      double* red = reinterpret_cast<double*>(smem_c);    // [wave 4][column 128][2]
      if (h == 0) {
#pragma unroll
        for (int j = 0; j < NB; ++j) { red[(wid * BN + colr + j) * 2] = sm[j]; red[(wid * BN + colr + j) * 2 + 1] = sq[j]; }
      }
      __syncthreads();
      if (t < BN && n0 + t < p.yC) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int w = 0; w < WGM; ++w) { a += red[(w * BN + t) * 2]; b += red[(w * BN + t) * 2 + 1]; }
        double* o = p.stat + ((size_t)tile_m * p.yC + n0 + t) * 2;
        o[0] = a; o[1] = b;
      }
    }
  }
#endif
}

// producer of the pre-cut operand: one thread per (k / 8, tile_n, pos) writes the 16-byte plane entries: two fp16 planes (one in the
// reduced-precision configuration) of w * 2^kB with kB from the 256 partial maxima of the source, stored in the panel's trailer
__global__ __launch_bounds__(256) void conv_precut_kernel(const float* w, unsigned short* out, int K, int Npad, int BN, size_t w_bs,
                                                          size_t out_bs, const float* wamax, int planes) {
  const int NBc = BN / 32;
  const int tiles_n = (Npad + BN - 1) / BN;
  const size_t total = (size_t)(K / 8) * tiles_n * BN;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  int kB = 0;
  if (wamax) kB = scale_exp(amax256(wamax, threadIdx.x & 63), PC_TOP_B);      // (before any lane leaves)
  if (i >= total) return;
  const int nl = (int)(i % BN); const size_t q = i / BN;               // consecutive threads: consecutive columns (coalesced reads)
  const int tn = (int)(q % tiles_n), kq = (int)(q / tiles_n);
  const int n = tn * BN + nl;
  const int pos = (nl % NBc) * 32 + nl / NBc;                          // operand position of column nl
  w += (size_t)blockIdx.y * w_bs; out += (size_t)blockIdx.y * out_bs;
  u32x4* o = reinterpret_cast<u32x4*>(out);
  if (wamax) {
    const float sb = pow2f(kB);
    unsigned hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) x[e] = (n < Npad ? w[(size_t)(kq * 8 + 2 * j + e) * Npad + n] : 0.f) * sb;
      const f16x2 hh = f16x2{(_Float16)x[0], (_Float16)x[1]};
      hi[j] = __builtin_bit_cast(unsigned, hh);
      lo[j] = __builtin_bit_cast(unsigned, f16x2{(_Float16)(x[0] - (float)hh[0]), (_Float16)(x[1] - (float)hh[1])});
    }
    // [stage = kq / 2][tile_n][kq & 1][plane 1 or 2][pos][8 f16], then the trailer
    const size_t base = ((((size_t)(kq >> 1) * tiles_n + tn) * 2 + (kq & 1)) * planes) * BN;
    o[base + pos] = u32x4{hi[0], hi[1], hi[2], hi[3]};
    if (planes == 2) o[base + (size_t)BN + pos] = u32x4{lo[0], lo[1], lo[2], lo[3]};
    if (i == 0) *reinterpret_cast<int*>(out + (size_t)(K / 16) * tiles_n * 2 * planes * BN * 8) = kB;
  }
}

// ---------------------------------------------------------------------------------------
// wgrad-type kernel on the LDS-DMA ring: dW[k][n] = sum_m A[m][k] dY[m][n], tile = BMK k-rows x BN columns, reduction
// over 16-pixel stages.  Both LDS tiles are pixel-major ([16 px][BMK] and [16 px][BN]), i.e. plain images of what the
// lanes fetch: a lane owns one 16-byte chunk of k (fixed tap and channels for the whole kernel, so it works for any
// Cin % 4 == 0, also across taps) or of n, and one or more pixels of the stage.  A stage's 16 pixels lie in one image
// (Wo % 16 == 0, or Wo | 16 with Ho*Wo % 16 == 0): its first pixel is tracked by a scalar cursor and every lane adds a
// fixed (dy, dx).  Fragments are ds_read_b64 of two adjacent k-rows / columns (conflict-free, no transposes):
// a lane's MFMA blocks i = 0, 1 hold k-rows (2r, 2r+1), blocks j = 0, 1 columns (2c, 2c+1).
// ---------------------------------------------------------------------------------------
template <int WGM, int WGN>
struct DmaWgTile {
  static constexpr int NW = WGM * WGN, BMK = 64 * WGM, BN = 64 * WGN, PX = 16, NST = 3;
  static constexpr int A_FL = PX * BMK, B_FL = PX * BN, ST_FL = A_FL + B_FL;
  static constexpr int LPRA = BMK / 4, LPRB = BN / 4;              // lanes per pixel row
  static constexpr int PPIA = 64 / LPRA > 0 ? 64 / LPRA : 1, PPIB = 64 / LPRB;   // pixels per instruction
  static constexpr int AI = (PX * LPRA / 64) / NW, BI = (PX * LPRB / 64) / NW;   // instructions per wave per stage
  static constexpr int SMEM = NST * ST_FL * 4;
  static_assert(LPRA <= 64 && AI >= 1 && BI >= 1, "tile shape");
};

// SPLIT: 0 = v_mfma_f32_32x32x2_f32, 1 = three bf16 planes per operand (six MFMAs per product), 2 = two fp16 planes of the operands
// scaled by powers of two from their amax (three MFMAs; x_amax / dy_amax: 256 floats each whose maximum is the operand's amax),
// 3 = ONE fp16 plane of the scaled operands (one MFMA: the reduced-precision configuration)
// PLANE: both operands are plain [M][C] matrices (the batched Winograd-domain reductions dU[p] = V[p]^T dM[p]: 1x1 taps, stride 1,
// no padding, output map = the row index).  The generic loader recomputes the im2col source of every piece every stage (~90 VALU
// + ~60 SALU per wave and stage, measured: the wave spends 41 % of its time issuing, 123 % of a SIMD's port at 3 waves); here a
// piece's offset is a per-lane constant and the stage advances through the scalar offset of the buffer load.
// PAIR (bit 0: x, bit 1: dy): that operand is stored in pair form, x_amax / dy_amax then point at the int exponent of its producer
template <int WGM, int WGN, int SPLIT, bool PLANE = false, int PAIR = 0>
__global__ __launch_bounds__(64 * WGM * WGN) void conv_wgrad_dma_kernel(GemmP p, DmaSched sc, const float* x_amax, const float* dy_amax) {
#if defined(__HIP_DEVICE_COMPILE__)
  using T = DmaWgTile<WGM, WGN>;
  constexpr int BMK = T::BMK, BN = T::BN, PX = T::PX, NST = T::NST, AI = T::AI, BI = T::BI;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wid / WGN, wn = wid % WGN;

  int u = blockIdx.x, gtile, split = 0, nsplit = 1, tt = 0;
  if (u < sc.full) {
    gtile = xcd_swizzle(u, sc.full);
  } else {
    u -= sc.full;
    tt = u / sc.tail_s; split = u - tt * sc.tail_s; nsplit = sc.tail_s;
    gtile = sc.full + tt;
  }
  const int z = gtile / sc.tiles_per_z, tile = gtile - z * sc.tiles_per_z;
  const int tile_n = tile % p.tiles_n, tile_k = tile / p.tiles_n;
  const int kt0 = tile_k * BMK, n0 = tile_n * BN;
  p.x += (size_t)z * p.x_bs; p.y += (size_t)z * p.y_bs; p.w += (size_t)z * p.w_bs;
  if (p.phases) { const int a = z >> 1, b = z & 1; p.pad_t -= a; p.pad_l -= b; p.yoff = a; p.xoff = b; }
  const int HoWo = p.Ho * p.Wo;
  const int nimg = p.M / HoWo;
  const int nmb_all = p.M / PX;
  const int mb_begin = nsplit > 1 ? split * sc.per_split : 0;
  const int mb_end = nsplit > 1 ? min(nmb_all, mb_begin + sc.per_split) : nmb_all;

  const unsigned x_bytes = (unsigned)((((size_t)p.xH * p.xW * nimg - 1) * p.xcs + p.xC) * 4);
  const unsigned y_bytes = (unsigned)((((size_t)p.yH * p.yW * nimg - 1) * p.ycs + p.yC) * 4);
  const i32x4 rsA = make_rsrc(p.x, x_bytes), rsB = make_rsrc(p.y, y_bytes);
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)smem;
  const int He = p.xH << p.ups, We = p.xW << p.ups;
  const bool wide = (p.Wo % PX) == 0;

  // ---- per-lane constants: A chunk -> (tap, ci); pixel offsets (dy, dx) of the lane's pixels inside a stage
  const int ak = kt0 + 4 * (lane % T::LPRA);
  const bool kvalid = ak < p.K;
  const int atap = ak / p.xC, aci = ak - atap * p.xC;
  const int akh = atap / p.KW, akw = atap - akh * p.KW;
  int a_dy[AI], a_dx[AI], b_dy[BI], b_dx[BI];
#pragma unroll
  for (int r = 0; r < AI; ++r) {
    const int j = (wid * AI + r) * T::PPIA + lane / T::LPRA;
    a_dy[r] = wide ? 0 : j / p.Wo; a_dx[r] = wide ? j : j % p.Wo;
  }
  const int bn = n0 + 4 * (lane % T::LPRB);
  const bool nvalid = bn < p.yC;
#pragma unroll
  for (int r = 0; r < BI; ++r) {
    const int j = (wid * BI + r) * T::PPIB + lane / T::LPRB;
    b_dy[r] = wide ? 0 : j / p.Wo; b_dx[r] = wide ? j : j % p.Wo;
  }
  // scalar cursor of the next stage to issue
  int c_n, c_oy, c_ox;
  {
    const int mbase = mb_begin * PX;
    c_n = mbase / HoWo; const int rem = mbase - c_n * HoWo;
    c_oy = rem / p.Wo; c_ox = rem - c_oy * p.Wo;
  }
  const int rows_per_stage = wide ? 0 : PX / p.Wo;
  // PLANE: per-lane byte offsets of the lane's pieces inside a stage (pixel j of the stage, its 16-byte chunk); out of range = zero fill
  unsigned pa_voff[AI], pb_voff[BI];
  unsigned p_stage = (unsigned)mb_begin;          // next stage to issue
  if constexpr (PLANE) {
#pragma unroll
    for (int r = 0; r < AI; ++r) pa_voff[r] = kvalid ? (unsigned)(a_dx[r] * p.xcs + ak) * 4u : DMA_OOB;
#pragma unroll
    for (int r = 0; r < BI; ++r) pb_voff[r] = nvalid ? (unsigned)(b_dx[r] * p.ycs + bn) * 4u : DMA_OOB;
  }
  auto issue = [&](int st) {
    const unsigned As = lds0 + (unsigned)(st * T::ST_FL) * 4u, Bs = As + T::A_FL * 4u;
    if constexpr (PLANE) {
      const unsigned sa = p_stage * (unsigned)(PX * 4) * (unsigned)p.xcs, sb = p_stage * (unsigned)(PX * 4) * (unsigned)p.ycs;
#pragma unroll
      for (int r = 0; r < AI; ++r) lds_dma16c(pa_voff[r], rsA, sa, As + (unsigned)(wid * AI + r) * 1024u);
#pragma unroll
      for (int r = 0; r < BI; ++r) lds_dma16c(pb_voff[r], rsB, sb, Bs + (unsigned)(wid * BI + r) * 1024u);
      p_stage += 1;
      return;
    }
    const int xin = c_n * p.xH * p.xW, yin = c_n * p.yH;
#pragma unroll
    for (int r = 0; r < AI; ++r) {
      unsigned off = DMA_OOB;
      const int sy = src_coord((c_oy + a_dy[r]) * p.stride - p.pad_t + akh, He, p.pad_mode, p.ups);
      const int sx = src_coord((c_ox + a_dx[r]) * p.stride - p.pad_l + akw, We, p.pad_mode, p.ups);
      if (kvalid && sy >= 0 && sx >= 0) off = (unsigned)((xin + sy * p.xW + sx) * p.xcs + aci) * 4u;
      lds_dma16(off, rsA, 0u, As + (unsigned)(wid * AI + r) * 1024u);
    }
#pragma unroll
    for (int r = 0; r < BI; ++r) {
      unsigned off = DMA_OOB;
      if (nvalid)
        off = (unsigned)(((yin + (c_oy + b_dy[r]) * p.ymul + p.yoff) * p.yW + (c_ox + b_dx[r]) * p.xmul + p.xoff) * p.ycs + bn) * 4u;
      lds_dma16(off, rsB, 0u, Bs + (unsigned)(wid * BI + r) * 1024u);
    }
    if (wide) {
      c_ox += PX;
      if (c_ox >= p.Wo) { c_ox = 0; c_oy += 1; if (c_oy >= p.Ho) { c_oy = 0; c_n += 1; } }
    } else {
      c_oy += rows_per_stage;
      if (c_oy >= p.Ho) { c_oy = 0; c_n += 1; }
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  int kx = 0, ky = 0;
  if constexpr (SPLIT >= 2) {
    if constexpr (PAIR & 1) kx = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(x_amax));
    else kx = __builtin_amdgcn_readfirstlane(scale_exp(amax256(x_amax, lane), PC_TOP_A));
    if constexpr (PAIR & 2) ky = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(dy_amax));
    else ky = __builtin_amdgcn_readfirstlane(scale_exp(amax256(dy_amax, lane), PC_TOP_A));
  }
  const float sx = pow2f(kx), sy = pow2f(ky);
  const int h = lane >> 5, l31 = lane & 31;
  const int a_rd = (8 * h) * BMK + wm * 64 + 2 * l31;
  const int b_rd = T::A_FL + (8 * h) * BN + wn * 64 + 2 * l31;
  // pixel order inside a stage: step s multiplies pixel s (lanes 0-31) and pixel 8 + s (lanes 32-63)
  auto compute = [&](int st) {
    const float* S = smem + st * T::ST_FL;
    float af[2][8], bf[2][8];
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) {
      const float2 a = *reinterpret_cast<const float2*>(S + a_rd + s8 * BMK);
      const float2 b = *reinterpret_cast<const float2*>(S + b_rd + s8 * BN);
      af[0][s8] = a.x; af[1][s8] = a.y; bf[0][s8] = b.x; bf[1][s8] = b.y;
    }
    if constexpr (SPLIT == 3) {
      split_mma_2x2_h1(acc, af, bf, sx, sy);
    } else if constexpr (SPLIT == 2 && PAIR != 0) {
      u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if constexpr (PAIR & 1) pair8(af[i], ah[i], al[i]); else split8h(af[i], sx, ah[i], al[i]);
        if constexpr (PAIR & 2) pair8(bf[i], bh[i], bl[i]); else split8h_rn(bf[i], sy, bh[i], bl[i]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x16 c = acc[i][j];
          c = mma_f16(al[i], bh[j], c); c = mma_f16(ah[i], bl[j], c); c = mma_f16(ah[i], bh[j], c);
          acc[i][j] = c;
        }
    } else if constexpr (SPLIT == 2) {
      split_mma_2x2_h(acc, af, bf, sx, sy);
    } else {
      static_assert(SPLIT == 0, "0: f32 MFMA, 2: two fp16 planes, 3: one fp16 plane");
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s8], bf[j][s8], acc[i][j], 0, 0, 0);
    }
  };

  if (mb_begin < mb_end) {
    issue(0);
    if (mb_begin + 1 < mb_end) issue(1);
    int st = 0;
    for (int mb = mb_begin; mb < mb_end; ++mb) {
      if (mb + 1 < mb_end) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(AI + BI) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      int st2 = st + 2; if (st2 >= NST) st2 -= NST;
      if (mb + 2 < mb_end) issue(st2);
      compute(st);
      st = st + 1 == NST ? 0 : st + 1;
    }
  }

  if constexpr (SPLIT >= 2) {                              // remove the operand scales (two exact power-of-two factors)
    const float cx = pow2f(-kx), cy = pow2f(-ky);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = (acc[i][j][e] * cx) * cy;
  }
  // ---- epilogue: lane holds k-rows kt0 + wm*64 + 2*rr + i (rr = (e&3) + 8*(e>>2) + 4*h), columns n0 + wn*64 + 2*l31 + j
  const int colr = wn * 64 + 2 * l31;
  if (nsplit > 1) {
    float* slab = p.slab + ((size_t)(tt * nsplit + split) * BMK) * BN;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wm * 64 + 2 * ((e & 3) + 8 * (e >> 2) + 4 * h) + i;
        *reinterpret_cast<float2*>(slab + (size_t)row * BN + colr) = make_float2(acc[i][0][e], acc[i][1][e]);
      }
    return;
  }
  float* out = const_cast<float*>(p.w);
  const int col = n0 + colr;
  if (col < p.Npad) {                           // Npad % 4 == 0 and col even: col + 1 < Npad too
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = kt0 + wm * 64 + 2 * ((e & 3) + 8 * (e >> 2) + 4 * h) + i;
        if (row < p.K) *reinterpret_cast<float2*>(out + (size_t)row * p.Npad + col) = make_float2(acc[i][0][e], acc[i][1][e]);
      }
  }
#endif
}

template <int BMK, int BN>
__global__ __launch_bounds__(256) void wgrad_dma_reduce_kernel(GemmP p, DmaSched sc) {
  const int tt = blockIdx.y;
  const int e4 = blockIdx.x * 256 + threadIdx.x;
  if (e4 >= BMK * BN / 4) return;
  const int r = e4 / (BN / 4), c4 = (e4 - r * (BN / 4)) * 4;
  const int gtile = sc.full + tt;
  const int z = gtile / sc.tiles_per_z, tile = gtile - z * sc.tiles_per_z;
  const int tile_n = tile % p.tiles_n, tile_k = tile / p.tiles_n;
  const int row = tile_k * BMK + r, col = tile_n * BN + c4;
  if (row >= p.K || col >= p.Npad) return;
  const float* sl = p.slab + ((size_t)tt * sc.tail_s * BMK + r) * BN + c4;
  float4 a = *reinterpret_cast<const float4*>(sl);
  for (int s = 1; s < sc.tail_s; ++s) {
    const float4 b = *reinterpret_cast<const float4*>(sl + (size_t)s * BMK * BN);
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  }
  float* out = const_cast<float*>(p.w) + (size_t)z * p.w_bs;
  *reinterpret_cast<float4*>(out + (size_t)row * p.Npad + col) = a;
}


// ---------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------
float* ws_amax(Stream& s, int which) {
  if (!s.ws || s.ws_bytes < (1u << 20)) throw Error(1, "two-plane pre-cut kernels need the stream scratch");
  return reinterpret_cast<float*>(s.ws + s.ws_bytes - PC_WS_TAIL + (size_t)which * 1024);
}
void amax_partials(Stream& s, const float* x, size_t rows, int C, size_t rs, int batch, size_t bs, float* out, int fold, float floor) {
  if (C % 4 || rs % 4 || bs % 4 || ((uintptr_t)x & 15)) throw Error(1, "amax_partials: operand not 16-byte aligned");
  const int flat = rs == (size_t)C && (batch == 1 || bs == rows * (size_t)C);
  hipLaunchKernelGGL(amax_partials_kernel, dim3(256), dim3(1024), 0, hs(s), x, rows, C / 4, rs, batch, bs, flat, out, fold, floor);
  check_launch("amax_partials");
}
void tensor_amax(Stream& s, const TView& x, float* slot, float floor) {
  amax_partials(s, x.p, x.pixels(), x.C, (size_t)x.cs, 1, 0, slot, 0, floor);
}

// ---- slot audit (hip_util.h) ------------------------------------------------------------------------------------------------
static void audit_needs_sync(Stream& s, const char* launch) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  SWN_HIP_CHECK(hipStreamIsCapturing(hs(s), &st));
  if (st != hipStreamCaptureStatusNone)
    throw Error(1, std::string("slot audit: ") + launch + " on a stream with an open capture (the audit reads back: switch it off, swn_slot_audit(0))");
}
static float audit_slot_max(Stream& s, const float* slot) {
  float h[AMAX_SLOT];
  dev_download(s, h, slot, sizeof h);
  float m = 0.f;
  for (float v : h) m = (v > m || v != v) ? v : m;       // (a NaN entry makes the maximum NaN, as the consumers read it)
  return m;
}
void audit_slot(Stream& s, const char* launch, const float* slot, const float* x, size_t rows, int C, size_t rs, int batch, size_t bs) {
  audit_needs_sync(s, launch);
  float* part = static_cast<float*>(dev_alloc(AMAX_SLOT * sizeof(float)));
  float sv = 0.f, am = 0.f;
  try {
    amax_partials(s, x, rows, C, rs, batch, bs, part);
    am = audit_slot_max(s, part);
    sv = audit_slot_max(s, slot);
  } catch (...) { dev_free(part); throw; }
  dev_free(part);
  char msg[256];
  if (!(sv >= am) || (am > 0.f && !(sv <= 4096.f * am))) {
    snprintf(msg, sizeof msg, "slot audit: %s: slot %.9g, operand amax %.9g (need amax <= slot <= 4096 * amax)", launch, (double)sv, (double)am);
    throw Error(1, msg);
  }
}
// max |h + l| over pair words {h | l << 16} (wino.hip pair4): the planes as stored, i.e. already times 2^k; an infinite or NaN
// half reads as +inf
__global__ __launch_bounds__(256) void pair_plane_amax_kernel(const unsigned* w, size_t n, float* out) {
  float am = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const unsigned u = w[i];
    const _Float16 h = __builtin_bit_cast(_Float16, (unsigned short)(u & 0xffffu)), l = __builtin_bit_cast(_Float16, (unsigned short)(u >> 16));
    float v = fabsf((float)h + (float)l);
    if (v != v) v = __builtin_inff();
    am = fmaxf(am, v);
  }
  amax_fold(am, out);
}
void audit_pair_planes(Stream& s, const char* launch, const float* planes, size_t elems, const int* kscale) {
  audit_needs_sync(s, launch);
  float* part = static_cast<float*>(dev_alloc(AMAX_SLOT * sizeof(float)));      // (zero-filled)
  float pm = 0.f;
  int k = 0;
  try {
    const unsigned grid = (unsigned)std::min<size_t>((elems + 255) / 256, 1024);
    hipLaunchKernelGGL(pair_plane_amax_kernel, dim3(grid ? grid : 1), dim3(256), 0, hs(s), reinterpret_cast<const unsigned*>(planes), elems, part);
    check_launch("pair_plane_amax");
    pm = audit_slot_max(s, part);
    dev_download(s, &k, kscale, sizeof k);
  } catch (...) { dev_free(part); throw; }
  dev_free(part);
  if (!(pm < 65504.f)) {
    char msg[256];
    snprintf(msg, sizeof msg, "slot audit: %s: pair-form planes reach %.9g at the published scale 2^%d: past fp16's 65504", launch, (double)pm, k);
    throw Error(1, msg);
  }
}

// trailer of a ring launch whose tail round was split along K: the partial tiles summed in fixed order, then the epilogue
template <int BM, int BN>
static void reduce_ring_tail(Stream& s, const GemmP& p, const DmaSched& sc) {
  if (!(sc.tail_tiles > 0 && sc.tail_s > 1)) return;
  hipLaunchKernelGGL((conv_dma_reduce_kernel<BM, BN>), dim3(BM * BN / 4 / 256, sc.tail_tiles), dim3(256), 0, hs(s), p, sc);
  check_launch("conv_dma_reduce");
}

// ---- LDS-DMA forward kernel (schedule: conv_gemm.hip plan_dma) -----------------------------------------------------------
template <int WGM, int WGN>
static void launch_fwd_dma_t(Stream& s, GemmP& p, int nb) {
  using T = DmaTile<WGM, WGN>;
  const int tiles_m = ceil_div(p.M, T::BM);
  p.tiles_n = ceil_div(p.Npad, T::BN);
  p.ntiles = tiles_m * p.tiles_n;
  const DmaSched sc = plan_fwd_dma<WGM, WGN>(p, nb, s.ws_bytes, nullptr);
  p.slab = reinterpret_cast<float*>(s.ws);
  p.splits = sc.tail_s;
  static bool once = (set_smem(conv_fwd_dma_kernel<WGM, WGN, true>, T::SMEM), set_smem(conv_fwd_dma_kernel<WGM, WGN, false>, T::SMEM), true);
  (void)once;
  char pname[128];
  prof_name(pname, "conv_fwd_dma_%dx%d", "[M%d,N%d,K%d,b%d,full%d,tail%dx%d]", T::BM, T::BN, p.M, p.Cout, p.K, nb, sc.full,
            sc.tail_tiles, sc.tail_s);
  ProfScope prof(s, pname, 2.0 * p.M * p.Cout * p.K * nb);
  const int units = sc.full + sc.tail_tiles * sc.tail_s;
  if (split_on()) hipLaunchKernelGGL((conv_fwd_dma_kernel<WGM, WGN, true>), dim3(units), dim3(64 * T::NW), T::SMEM, hs(s), p, sc);
  else hipLaunchKernelGGL((conv_fwd_dma_kernel<WGM, WGN, false>), dim3(units), dim3(64 * T::NW), T::SMEM, hs(s), p, sc);
  check_launch("conv_fwd_dma");
  reduce_ring_tail<T::BM, T::BN>(s, p, sc);
}
void launch_fwd_dma(Stream& s, GemmP& p, RingTile tile, int nb) {
  switch (tile) {
    case RING_128x128: return launch_fwd_dma_t<2, 2>(s, p, nb);
    case RING_128x256: return launch_fwd_dma_t<2, 4>(s, p, nb);
    case RING_256x64: return launch_fwd_dma_t<4, 1>(s, p, nb);
  }
  throw Error(1, "conv_fwd: unknown ring tile");
}

// ---- pre-cut ring kernel ---------------------------------------------------------------------------------------------------
template <int WGM, int NB, int NSTG, int WGCU, int PL>
static void launch_fwd_pc_t(Stream& s, GemmP& p, int nb, const unsigned short* wpc, size_t wpc_bs, bool phases, const float* x_amax,
                            const int* x_pair_k) {
  using T = PcTile<WGM, NB, NSTG, PL>;
  const int tiles_m = ceil_div(p.M, T::BM);
  p.tiles_n = ceil_div(p.Npad, T::BN);
  p.ntiles = tiles_m * p.tiles_n;
  static_assert(WGCU * T::SMEM <= 160 * 1024, "tile does not fit a CU");
  const size_t ws_cap = s.ws_bytes - PC_WS_TAIL;
  const float* a_amax = nullptr;
  if (x_pair_k && PL != 2) throw Error(1, "conv_fwd: a pair-form operand needs the two-plane kernel");
  if (x_pair_k) {
    // (the producer scaled and cut the operand: nothing to take the amax of)
  } else if (x_amax && amax_fused_on()) {
    a_amax = x_amax;          // the producer of the operand left its amax (256 floats, maximum = amax) in a slot: no pass of our own
    if (slot_audit_on())
      audit_slot(s, "conv_fwd", x_amax, p.x, (size_t)(p.M / (p.Ho * p.Wo)) * p.xH * p.xW, p.xC, (size_t)p.xcs, phases ? 1 : nb, p.x_bs);
  } else {
    // |A|max over the whole input tensor of the launch (all images, all channels the gather reads; batched planes too)
    float* part = ws_amax(s, 0);
    amax_partials(s, p.x, (size_t)(p.M / (p.Ho * p.Wo)) * p.xH * p.xW, p.xC, (size_t)p.xcs, phases ? 1 : nb, p.x_bs, part);
    a_amax = part;
  }
  DmaSched sc = plan_pc<T, WGCU>(p.ntiles, nb, p.K, ws_cap);
  if (phases && env_on(getenv("SWN_PHASE_ZFAST"))) sc.zfast = nb;     // (A/B, read per launch)
  if (p.stat) {       // the statistics come out of the tile epilogue: every tile whole
    if (!(WGM == 4 && NB == 4) || nb != 1 || p.accumulate || p.act != ACT_NONE || (p.Ho * p.Wo) % T::BM)
      throw Error(1, "conv_fwd: stat_partial on a launch that cannot emit statistics (ask conv_fwd_stat_chunk first)");
    sc.full = p.ntiles * nb; sc.tail_tiles = 0; sc.tail_s = 1; sc.per_split = p.K / T::BK;
  }
  p.slab = reinterpret_cast<float*>(s.ws);
  p.splits = sc.tail_s;
  static bool once = (set_smem(conv_fwd_pc_kernel<WGM, NB, NSTG, WGCU, PL>, T::SMEM), true);
  (void)once;
  char pname[128];
  // (_ap: the operand arrives in pair form, cut by its producer; _as: its scale comes from the producer's amax slot)
  prof_name(pname, "conv_fwd_pc_%dx%d", "%s[M%d,N%d,K%d,b%d,full%d,tail%dx%d]", T::BM, T::BN, x_pair_k ? "_ap" : (a_amax == x_amax ? "_as" : ""), p.M, p.Cout, p.K, nb,
            sc.full, sc.tail_tiles, sc.tail_s);
  ProfScope prof(s, pname, 2.0 * p.M * p.Cout * p.K * nb);
  const int units = sc.full + sc.tail_tiles * sc.tail_s;
  if constexpr (PL == 2 && NSTG <= 3) {
    if (x_pair_k) {
      static bool once2 = (set_smem(conv_fwd_pc_kernel<WGM, NB, NSTG, WGCU, 2, true>, T::SMEM), true);
      (void)once2;
      hipLaunchKernelGGL((conv_fwd_pc_kernel<WGM, NB, NSTG, WGCU, 2, true>), dim3(units), dim3(64 * T::NW), T::SMEM, hs(s), p, sc, wpc, wpc_bs,
                         a_amax, x_pair_k);
    } else {
      hipLaunchKernelGGL((conv_fwd_pc_kernel<WGM, NB, NSTG, WGCU, PL>), dim3(units), dim3(64 * T::NW), T::SMEM, hs(s), p, sc, wpc, wpc_bs,
                         a_amax, x_pair_k);
    }
  } else {
    if (x_pair_k) throw Error(1, "conv_fwd: no pair-form instantiation of this tile configuration");
    hipLaunchKernelGGL((conv_fwd_pc_kernel<WGM, NB, NSTG, WGCU, PL>), dim3(units), dim3(64 * T::NW), T::SMEM, hs(s), p, sc, wpc, wpc_bs,
                       a_amax, x_pair_k);
  }
  check_launch("conv_fwd_pc");
  reduce_ring_tail<T::BM, T::BN>(s, p, sc);
}
// the tile of a column width, for either plane count: 128 x 192, 128 x 128 (conv_gemm.h PC128_*), 256 x 64
template <int PL>
static void launch_fwd_pc_planes(Stream& s, GemmP& p, int bn, int nb, const unsigned short* wpc, size_t wpc_bs, bool phases,
                                 const float* x_amax, const int* x_pair_k) {
  switch (bn) {
    case 192: return launch_fwd_pc_t<4, 6, 2, 2, PL>(s, p, nb, wpc, wpc_bs, phases, x_amax, x_pair_k);
    case 128: return launch_fwd_pc_t<PC128_WGM, PC128_NB, PC128_NSTG, PC128_WGCU, PL>(s, p, nb, wpc, wpc_bs, phases, x_amax, x_pair_k);
    case 64: return launch_fwd_pc_t<8, 2, 3, 2, PL>(s, p, nb, wpc, wpc_bs, phases, x_amax, x_pair_k);
  }
  throw Error(1, "conv_fwd: unknown pre-cut tile");
}
void launch_fwd_pc(Stream& s, GemmP& p, int bn, int planes, int nb, const unsigned short* wpc, size_t wpc_bs, bool phases,
                   const float* x_amax, const int* x_pair_k) {
  if (planes == 1) launch_fwd_pc_planes<1>(s, p, bn, nb, wpc, wpc_bs, phases, x_amax, x_pair_k);
  else launch_fwd_pc_planes<2>(s, p, bn, nb, wpc, wpc_bs, phases, x_amax, x_pair_k);
}

// ---- producer of the pre-cut operand (ops.h) -------------------------------------------------------------------------------
size_t conv_precut_elems(int K, int Npad, int bn) {
  return (size_t)(K / 16) * ceil_div(Npad, bn) * 2 * conv_precut_planes() * bn * 8 + PC_TRAILER;
}
const float* conv_precut_amax(Stream& s, const float* src, size_t rows, int C, int batch, size_t bs) {
  float* part = ws_amax(s, 1);
  amax_partials(s, src, rows, C, (size_t)C, batch, bs, part);
  return part;
}
void conv_precut(Stream& s, const float* w, int K, int Npad, int bn, int batch, size_t w_bs, uint16_t* out, const float** amax_io) {
  if (K % 16 || (bn != 64 && bn != 128 && bn != 192)) throw Error(1, "conv_precut: K must be a multiple of 16, tile 64, 128 or 192");
  const size_t total = (size_t)(K / 8) * ceil_div(Npad, bn) * bn;
  // two-plane form: one scale for all `batch` panels of the launch (they are cut from one weight tensor)
  const float* wamax = (amax_io && *amax_io) ? *amax_io : conv_precut_amax(s, w, (size_t)K, Npad, batch, w_bs);
  if (amax_io) *amax_io = wamax;
  hipLaunchKernelGGL(conv_precut_kernel, dim3((unsigned)((total + 255) / 256), batch), dim3(256), 0, hs(s), w, out, K, Npad, bn, w_bs,
                     conv_precut_elems(K, Npad, bn), wamax, conv_precut_planes());
  check_launch("conv_precut");
}

// ---- weight-gradient ring kernel -------------------------------------------------------------------------------------------
template <int WGM, int WGN>
static void launch_wgrad_dma_t(Stream& s, GemmP& p, int nb, const ConvWgradArgs& a) {
  using T = DmaWgTile<WGM, WGN>;
  const int tiles_k = ceil_div(p.K, T::BMK);
  p.tiles_n = ceil_div(p.Npad, T::BN);
  p.ntiles = tiles_k * p.tiles_n;
  const int nmb = p.M / T::PX;
  const int wg_per_cu = std::min(160 * 1024 / T::SMEM, 12 / T::NW);
  const int wpl = wgrad_planes();
  const bool two = split_on() && wpl <= 2 && s.ws && s.ws_bytes >= (1u << 20);        // fp16 planes: scaled operands
  const float *xa = nullptr, *ya = nullptr;
  if (two) {
    // both operands are activations: their amax over the whole tensors the gather / the dY rows come from -- left in a slot by
    // whoever produced the tensor (ConvWgradArgs::x_amax / dy_amax), else taken here
    const int nbb = a.phases ? 1 : nb;
    const size_t nimg = (size_t)(p.M / (p.Ho * p.Wo));
    const bool fused = amax_fused_on();
    if (a.x_pair_k) xa = reinterpret_cast<const float*>(a.x_pair_k);
    else if (a.x_amax && fused) {
      xa = a.x_amax;
      if (slot_audit_on()) audit_slot(s, "conv_wgrad (x)", a.x_amax, a.x.p, nimg * a.x.H * a.x.W, a.x.C, (size_t)a.x.cs, nbb, a.x_bs);
    }
    else { float* px = ws_amax(s, 0); amax_partials(s, a.x.p, nimg * a.x.H * a.x.W, a.x.C, (size_t)a.x.cs, nbb, a.x_bs, px); xa = px; }
    if (a.dy_pair_k) ya = reinterpret_cast<const float*>(a.dy_pair_k);
    else if (a.dy_amax && fused) {
      ya = a.dy_amax;
      if (slot_audit_on()) audit_slot(s, "conv_wgrad (dy)", a.dy_amax, a.dy.p, nimg * a.dy.H * a.dy.W, a.dy.C, (size_t)a.dy.cs, nbb, a.dy_bs);
    }
    else { float* py = ws_amax(s, 1); amax_partials(s, a.dy.p, nimg * a.dy.H * a.dy.W, a.dy.C, (size_t)a.dy.cs, nbb, a.dy_bs, py); ya = py; }
  }
  const DmaSched sc = plan_dma(p.ntiles * nb, p.ntiles, nmb, 256 * wg_per_cu, (size_t)T::BMK * T::BN * 4, two ? s.ws_bytes - PC_WS_TAIL : s.ws_bytes);
  p.slab = reinterpret_cast<float*>(s.ws);
  p.splits = sc.tail_s;
  static bool once = (set_smem(conv_wgrad_dma_kernel<WGM, WGN, 2>, T::SMEM), set_smem(conv_wgrad_dma_kernel<WGM, WGN, 0>, T::SMEM),
                      set_smem(conv_wgrad_dma_kernel<WGM, WGN, 3>, T::SMEM), true);
  (void)once;
  // plain [M][C] operands (batched Winograd planes): the loader without im2col arithmetic
  const bool plane = p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad_t == 0 && p.pad_l == 0 && !p.ups && !p.phases && p.Ho == 1 &&
                     p.Wo % T::PX == 0 && p.xH == 1 && p.yH == 1 && p.xW == p.Wo && p.yW == p.Wo && p.ymul == 1 && p.xmul == 1 &&
                     p.yoff == 0 && p.xoff == 0 && p.M == p.Wo;
  const bool two_plane = two && wpl == 2 && plane;
  const int pairm = (a.x_pair_k ? 1 : 0) | (a.dy_pair_k ? 2 : 0);
  // (_sx / _sy / _sxy behind the plane form: the scale of x / dy / both comes from the producer's amax slot, not from a pass of ours)
  const int slotm = (two && xa && xa == a.x_amax ? 1 : 0) | (two && ya && ya == a.dy_amax ? 2 : 0);
  char pname[128];
  prof_name(pname, "conv_wgrad_dma_%dx%d", "%s%s[M%d,N%d,K%d,b%d,full%d,tail%dx%d]", T::BMK, T::BN,
            two ? (wpl == 1 ? "_h1" : (two_plane ? (pairm == 3 ? "_h2pp" : (pairm ? "_h2p1" : "_h2p")) : "_h2")) : "",
            slotm == 3 ? "_sxy" : (slotm == 2 ? "_sy" : (slotm == 1 ? "_sx" : "")), p.M, p.Cout, p.K, nb,
            sc.full, sc.tail_tiles, sc.tail_s);
  ProfScope prof(s, pname, 2.0 * p.M * p.Cout * p.K * nb);
  const int units = sc.full + sc.tail_tiles * sc.tail_s;
  if (pairm && !two_plane) throw Error(1, "conv_wgrad: pair-form operands need the two-plane plane-form kernel");
  if (two_plane) {
    static bool once2 = (set_smem(conv_wgrad_dma_kernel<WGM, WGN, 2, true, 0>, T::SMEM), set_smem(conv_wgrad_dma_kernel<WGM, WGN, 2, true, 1>, T::SMEM),
                         set_smem(conv_wgrad_dma_kernel<WGM, WGN, 2, true, 2>, T::SMEM), set_smem(conv_wgrad_dma_kernel<WGM, WGN, 2, true, 3>, T::SMEM), true);
    (void)once2;
    const dim3 g(units), b(64 * T::NW);
    if (pairm == 3) hipLaunchKernelGGL((conv_wgrad_dma_kernel<WGM, WGN, 2, true, 3>), g, b, T::SMEM, hs(s), p, sc, xa, ya);
    else if (pairm == 2) hipLaunchKernelGGL((conv_wgrad_dma_kernel<WGM, WGN, 2, true, 2>), g, b, T::SMEM, hs(s), p, sc, xa, ya);
    else if (pairm == 1) hipLaunchKernelGGL((conv_wgrad_dma_kernel<WGM, WGN, 2, true, 1>), g, b, T::SMEM, hs(s), p, sc, xa, ya);
    else hipLaunchKernelGGL((conv_wgrad_dma_kernel<WGM, WGN, 2, true, 0>), g, b, T::SMEM, hs(s), p, sc, xa, ya);
  }
  else if (two && wpl == 1) hipLaunchKernelGGL((conv_wgrad_dma_kernel<WGM, WGN, 3>), dim3(units), dim3(64 * T::NW), T::SMEM, hs(s), p, sc, xa, ya);
  else if (two) hipLaunchKernelGGL((conv_wgrad_dma_kernel<WGM, WGN, 2>), dim3(units), dim3(64 * T::NW), T::SMEM, hs(s), p, sc, xa, ya);
  else hipLaunchKernelGGL((conv_wgrad_dma_kernel<WGM, WGN, 0>), dim3(units), dim3(64 * T::NW), T::SMEM, hs(s), p, sc, xa, ya);
  check_launch("conv_wgrad_dma");
  if (sc.tail_tiles > 0 && sc.tail_s > 1) {
    hipLaunchKernelGGL((wgrad_dma_reduce_kernel<T::BMK, T::BN>), dim3(T::BMK * T::BN / 4 / 256, sc.tail_tiles), dim3(256), 0, hs(s), p, sc);
    check_launch("wgrad_dma_reduce");
  }
}
void launch_wgrad_dma(Stream& s, GemmP& p, RingTile tile, int nb, const ConvWgradArgs& a) {
  switch (tile) {
    case RING_128x128: return launch_wgrad_dma_t<2, 2>(s, p, nb, a);    // 128 k-rows x 128 columns
    case RING_256x64: return launch_wgrad_dma_t<4, 1>(s, p, nb, a);
    default: break;
  }
  throw Error(1, "conv_wgrad: unknown ring tile");
}

}  // namespace swn
