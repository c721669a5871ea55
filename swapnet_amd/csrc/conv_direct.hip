// swapnet_amd -- implicit-GEMM convolution, register-staged kernels: the wide forward-type and weight-gradient kernels, their
// narrow-N (Cout <= 32) forms, the split-K reductions and the naive references.  Overview: conv_gemm.hip; shared: conv_gemm.h.
#include "conv_gemm.h"

namespace swn {

template <int MT, int NT, int WGM, int WGN>
struct Tile {
  static constexpr int BM = 32 * MT * WGM;
  static constexpr int BN = 32 * NT * WGN;
  static constexpr int BK = 32;
  static constexpr int AS = BK + 4;   // 16-byte aligned rows; 36*i mod 64 banks distinct for 16 rows (b128)
  static constexpr int A_FLOATS = ((BM * AS + 3) / 4) * 4;
  static constexpr int B_FLOATS = BK * BN;
  static constexpr int SMEM_FWD = (2 * A_FLOATS + 2 * B_FLOATS + BM) * 4;
  // wgrad: A' tile [32 pixels][BM], B' tile [32 pixels][BN]
  static constexpr int SMEM_WG = (2 * BK * BM + 2 * BK * BN) * 4;
};

// ---------------------------------------------------------------------------------------
// forward-type kernel
// ---------------------------------------------------------------------------------------
template <int MT, int NT, int WGM, int WGN, bool FAST>
__global__ __launch_bounds__(64 * WGM * WGN) void conv_fwd_kernel(GemmP p) {
  using T = Tile<MT, NT, WGM, WGN>;
  constexpr int BM = T::BM, BN = T::BN, AS = T::AS;
  constexpr int NTHR = 64 * WGM * WGN;
  constexpr int AROWS = NTHR / 8;        // A-tile rows covered by one pass (8 lanes x 16 B per row)
  constexpr int RA = BM / AROWS;
  constexpr int B4 = BN / 4;             // float4 per B-tile row
  constexpr int RB = 32 * B4 / NTHR;     // float4 of the 32 x BN weight tile per thread (element i = t + r * NTHR)
  static_assert(32 * B4 % NTHR == 0, "B tile must divide evenly over the workgroup");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;
  float* Bs = smem + 2 * T::A_FLOATS;
  int* rowoff = (int*)(Bs + 2 * T::B_FLOATS);

  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int wm = wid / WGN, wn = wid % WGN;
  const int tile = xcd_swizzle(blockIdx.x, p.ntiles);
  const int tile_n = tile % p.tiles_n, tile_m = tile / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int split = blockIdx.y;
  p.x += (size_t)blockIdx.z * p.x_bs; p.w += (size_t)blockIdx.z * p.w_bs;
  p.y += (size_t)blockIdx.z * p.y_bs; p.slab += (size_t)blockIdx.z * p.slab_bs;
  apply_phase(p);

  const int q = t & 7, p0 = t >> 3;
  int a_iy0[RA], a_ix0[RA], a_base[RA];
  const int HoWo = p.Ho * p.Wo;
#pragma unroll
  for (int r = 0; r < RA; ++r) {
    const int m = m0 + p0 + AROWS * r;
    if (m < p.M) {
      const int n = m / HoWo, rem = m - n * HoWo;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      a_iy0[r] = oy * p.stride - p.pad_t;
      a_ix0[r] = ox * p.stride - p.pad_l;
      a_base[r] = n * p.xH * p.xW * p.xcs;
    } else {
      a_iy0[r] = 0; a_ix0[r] = 0; a_base[r] = -1;
    }
  }
  const int He = p.xH << p.ups, We = p.xW << p.ups;

  float4 ra[RA], rb[RB];
  // FAST (Cin % 32 == 0): a 32-wide k block never straddles a tap, and the tap changes only every Cin/32
  // stages (never for the 1x1 batched Winograd GEMMs).  The per-row source offsets of the current tap are
  // therefore cached; a stage only advances the channel offset.  This keeps ~100 VALU/SALU instructions
  // (tap decode, padding rules, 64-bit address math per row) out of every stage -- issue slots the matrix
  // pipe waits for when both waves of a SIMD sit behind the same workgroup barrier.
  int b_row[RB], b_off[RB];               // this thread's rows of the 32 x BN weight tile; offset inside the panel
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const int bi = t + r * NTHR;
    const int n = n0 + (bi % B4) * 4;
    b_row[r] = bi / B4;
    b_off[r] = n < p.Npad ? b_row[r] * p.Npad + n : -1;
  }
  int a_off[RA];                          // element offset of this row's pixel for the cached tap, -1 = zero fill
  int ld_tap = -1, ld_ci = 0;             // wave-uniform loader state
  int g_tap = -1, g_ci = 0;               // generic path: per-thread (tap, ci)
  const int q32 = 32 / p.xC, r32 = 32 - q32 * p.xC;
  const int rcpKW = (65536 + p.KW - 1) / p.KW;
  auto set_tap = [&](int tap) {
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
#pragma unroll
    for (int r = 0; r < RA; ++r) {
      int off = -1;
      if (a_base[r] >= 0) {
        const int sy = src_coord(a_iy0[r] + kh, He, p.pad_mode, p.ups);
        const int sx = src_coord(a_ix0[r] + kw, We, p.pad_mode, p.ups);
        if (sy >= 0 && sx >= 0) off = a_base[r] + (sy * p.xW + sx) * p.xcs + 4 * q;
      }
      a_off[r] = off;
    }
    ld_tap = tap;
  };
  auto load_tiles = [&](int kb) {
    const int k0 = kb * 32;
    if (FAST) {
      if (ld_tap < 0) {                    // first stage of this block (split-K blocks start anywhere)
        const int tap = k0 / p.xC;
        ld_ci = k0 - tap * p.xC;
        set_tap(tap);
      } else {                             // stages are visited in order
        ld_ci += 32;
        if (ld_ci >= p.xC) { ld_ci = 0; set_tap(ld_tap + 1); }
      }
#pragma unroll
      for (int r = 0; r < RA; ++r)
        ra[r] = a_off[r] >= 0 ? *reinterpret_cast<const float4*>(p.x + (size_t)(unsigned)a_off[r] + ld_ci)
                              : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      // generic path (Cin % 32 != 0): every thread tracks the (tap, ci) of its own 4-channel group and
      // advances it by 32 channels per stage with the precomputed quotient / remainder of 32 by Cin --
      // no per-stage integer divisions (tap -> (kh, kw) by a 16-bit reciprocal, exact for tap < 4096)
      if (g_tap < 0) {
        const int k = k0 + 4 * q;
        g_tap = k / p.xC;
        g_ci = k - g_tap * p.xC;
      } else {
        g_tap += q32; g_ci += r32;
        if (g_ci >= p.xC) { g_ci -= p.xC; ++g_tap; }
      }
      const bool kvalid = k0 + 4 * q < p.K;
      const int tap = g_tap, ci = g_ci;
      const int kh = (tap * rcpKW) >> 16, kw = tap - kh * p.KW;
#pragma unroll
      for (int r = 0; r < RA; ++r) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a_base[r] >= 0 && kvalid) {
          const int sy = src_coord(a_iy0[r] + kh, He, p.pad_mode, p.ups);
          const int sx = src_coord(a_ix0[r] + kw, We, p.pad_mode, p.ups);
          if (sy >= 0 && sx >= 0)
            v = *reinterpret_cast<const float4*>(p.x + (size_t)a_base[r] + (size_t)(sy * p.xW + sx) * p.xcs + ci);
        }
        ra[r] = v;
      }
    }
    const float* wk = p.w + (size_t)k0 * p.Npad;          // uniform part of the weight-panel address
#pragma unroll
    for (int r = 0; r < RB; ++r)
      rb[r] = (b_off[r] >= 0 && k0 + b_row[r] < p.K) ? *reinterpret_cast<const float4*>(wk + b_off[r])
                                                     : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto store_tiles = [&](int buf) {
    float* A = As + buf * T::A_FLOATS;
#pragma unroll
    for (int r = 0; r < RA; ++r) *reinterpret_cast<float4*>(A + (p0 + AROWS * r) * AS + 4 * q) = ra[r];
    float* B = Bs + buf * T::B_FLOATS;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int bi = t + r * NTHR;
      *reinterpret_cast<float4*>(B + (bi / B4) * BN + (bi % B4) * 4) = rb[r];
    }
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // One LDS stage = 16 MFMA k-steps.  The reduction order inside the stage is permuted so that
  // step s consumes k = s (lanes 0-31) and k = 16 + s (lanes 32-63): a lane's 16 A values are
  // then contiguous in its row -> 4 ds_read_b128 instead of 16 ds_read_b32.  All fragments of the
  // stage are fetched before the first MFMA (64 VGPRs) so LDS latency is paid once per stage,
  // not once per k-step.
  auto compute = [&](int buf) {
    const int h = lane >> 5;
    const float* A = As + buf * T::A_FLOATS + (wm * MT * 32 + (lane & 31)) * AS + 16 * h;
    const float* B = Bs + buf * T::B_FLOATS + (16 * h) * BN + wn * NT * 32 + (lane & 31);
    float af[MT][16], bf[NT][16];
    // issue order = consumption order (k-steps 0-3 of every fragment first, then 4-7, ...): LDS returns
    // in order, so the first MFMAs wait for a quarter of the reads only and the rest land under them
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(A + i * 32 * AS + 4 * g);
        af[i][4 * g] = v.x; af[i][4 * g + 1] = v.y; af[i][4 * g + 2] = v.z; af[i][4 * g + 3] = v.w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < NT; ++j) bf[j][4 * g + e] = B[(4 * g + e) * BN + j * 32];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int st = 0; st < 16; ++st)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][st], bf[j][st], acc[i][j], 0, 0, 0);
  };

  const int nkb = (p.K + 31) / 32;
  const int kb_begin = split * p.per_split;
  const int kb_end = min(nkb, kb_begin + p.per_split);
  if (kb_begin < kb_end) {
    load_tiles(kb_begin);
    store_tiles(0);
    __syncthreads();
    int cur = 0;
    for (int kb = kb_begin; kb < kb_end; ++kb) {
      const bool more = kb + 1 < kb_end;
      if (more) load_tiles(kb + 1);
      compute(cur);
      if (more) store_tiles(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }

  // ---- epilogue
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
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = n0 + wn * NT * 32 + j * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wm * MT * 32 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        float v = acc[i][j][e];
        if (p.splits > 1) {
          if (m0 + row < p.M && col < p.Npad)
            p.slab[((size_t)split * p.M + (m0 + row)) * p.Npad + col] = v;
        } else {
          const int off = rowoff[row];
          if (off >= 0 && col < p.Cout) {
            if (p.bias) v += p.bias[col];
            v = act_apply(v, p.act);
            float* dst = p.y + (size_t)off + col;
            if (p.accumulate) v += *dst;
            *dst = v;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// narrow-N forward-type kernel (Cout <= 32: the 19-channel tail conv, PatchGAN's 1-channel
// prediction conv, dgrads into few-channel inputs).  The 32-wide MFMA tile wastes 13/32 of
// the matrix pipe at N = 19; v_mfma_f32_4x4x1 (16 independent 4x4 blocks per wave, same
// FLOP rate) has a 4-column granularity instead: each LANE owns one output pixel (B operand
// = its im2col value), the weights W[k][4g..4g+3] sit in lanes 4g..4g+3 of one VGPR and are
// broadcast to all 16 blocks (cbsz = 4, abid = g), and the result is, per lane, a float4 of
// 4 consecutive output channels of its pixel -- a 16-byte NHWC store.  Layout verified by
// tools/mfma_probe.hip.
// ---------------------------------------------------------------------------------------
struct NarrowTile {
  static constexpr int BM = 256, BK = 16, AS = BK + 4;      // 20*l mod 64 distinct for 16 lanes (b128)
  static constexpr int A_FLOATS = BM * AS, B_FLOATS = 32 * AS;
  static constexpr int SMEM = (2 * A_FLOATS + 2 * B_FLOATS) * 4;
};

template <int NG, bool FAST>
__global__ __launch_bounds__(256) void conv_fwd_narrow_kernel(GemmP p) {
  using T = NarrowTile;
  constexpr int AS = T::AS, RA = 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                       // [2][256 pixels][16 k]
  float* Bt = smem + 2 * T::A_FLOATS;     // [2][32 n][16 k]   (weights, transposed)

  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int tile = xcd_swizzle(blockIdx.x, p.ntiles);
  const int m0 = tile * T::BM;
  const int split = blockIdx.y;
  p.x += (size_t)blockIdx.z * p.x_bs; p.w += (size_t)blockIdx.z * p.w_bs;
  p.y += (size_t)blockIdx.z * p.y_bs; p.slab += (size_t)blockIdx.z * p.slab_bs;
  apply_phase(p);

  const int q = t & 3, p0 = t >> 2;       // 4 lanes x 16 B per tile row, 64 rows per pass
  int a_iy0[RA], a_ix0[RA], a_base[RA];
  const int HoWo = p.Ho * p.Wo;
#pragma unroll
  for (int r = 0; r < RA; ++r) {
    const int m = m0 + p0 + 64 * r;
    if (m < p.M) {
      const int n = m / HoWo, rem = m - n * HoWo;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      a_iy0[r] = oy * p.stride - p.pad_t;
      a_ix0[r] = ox * p.stride - p.pad_l;
      a_base[r] = n * p.xH * p.xW * p.xcs;
    } else {
      a_iy0[r] = 0; a_ix0[r] = 0; a_base[r] = -1;
    }
  }
  const int brow = t & 15, bcol = (t >> 4) * 4;     // threads 0..127 move the 16 x 32 weight tile; this mapping
                                                    // makes the transposed LDS stores ((bcol+i)*20 + brow) conflict-free
  const int He = p.xH << p.ups, We = p.xW << p.ups;

  float4 ra[RA], rb;
  auto load_tiles = [&](int kb) {
    const int k0 = kb * 16;
    int kh, kw, ci;
    bool kvalid = true;
    if (FAST) {
      const int tap = k0 / p.xC;           // xC % 32 == 0: a 16-wide k block never straddles a tap
      ci = k0 - tap * p.xC + 4 * q;
      kh = tap / p.KW; kw = tap - kh * p.KW;
    } else {
      const int k = k0 + 4 * q;
      kvalid = k < p.K;
      const int tap = k / p.xC;
      ci = k - tap * p.xC;
      kh = tap / p.KW; kw = tap - kh * p.KW;
    }
#pragma unroll
    for (int r = 0; r < RA; ++r) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a_base[r] >= 0 && kvalid) {
        const int sy = src_coord(a_iy0[r] + kh, He, p.pad_mode, p.ups);
        const int sx = src_coord(a_ix0[r] + kw, We, p.pad_mode, p.ups);
        if (sy >= 0 && sx >= 0)
          v = *reinterpret_cast<const float4*>(p.x + (size_t)a_base[r] + (size_t)(sy * p.xW + sx) * p.xcs + ci);
      }
      ra[r] = v;
    }
    rb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < 128 && k0 + brow < p.K && bcol < p.Npad)
      rb = *reinterpret_cast<const float4*>(p.w + (size_t)(k0 + brow) * p.Npad + bcol);
  };
  auto store_tiles = [&](int buf) {
    float* A = As + buf * T::A_FLOATS;
#pragma unroll
    for (int r = 0; r < RA; ++r) *reinterpret_cast<float4*>(A + (p0 + 64 * r) * AS + 4 * q) = ra[r];
    if (t < 128) {
      float* B = Bt + buf * T::B_FLOATS + bcol * AS + brow;
      B[0] = rb.x; B[AS] = rb.y; B[2 * AS] = rb.z; B[3 * AS] = rb.w;
    }
  };

  f32x4 acc[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int buf) {
    const float* A = As + buf * T::A_FLOATS + (wid * 64 + lane) * AS;      // this lane's pixel
    const float* B = Bt + buf * T::B_FLOATS + (lane & 31) * AS;            // W[.][lane]
    float xv[16], wv[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 a = *reinterpret_cast<const float4*>(A + 4 * g);
      const float4 b = *reinterpret_cast<const float4*>(B + 4 * g);
      xv[4 * g] = a.x; xv[4 * g + 1] = a.y; xv[4 * g + 2] = a.z; xv[4 * g + 3] = a.w;
      wv[4 * g] = b.x; wv[4 * g + 1] = b.y; wv[4 * g + 2] = b.z; wv[4 * g + 3] = b.w;
    }
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) NarrowMac<0, NG>::run(acc, wv[kk], xv[kk]);
  };

  const int nkb = (p.K + 15) / 16;
  const int kb_begin = split * p.per_split;
  const int kb_end = min(nkb, kb_begin + p.per_split);
  if (kb_begin < kb_end) {
    load_tiles(kb_begin);
    store_tiles(0);
    __syncthreads();
    int cur = 0;
    for (int kb = kb_begin; kb < kb_end; ++kb) {
      const bool more = kb + 1 < kb_end;
      if (more) load_tiles(kb + 1);
      compute(cur);
      if (more) store_tiles(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }

  // ---- epilogue: one output pixel per lane
  const int m = m0 + wid * 64 + lane;
  if (m >= p.M) return;
  if (p.splits > 1) {
    float* dst = p.slab + ((size_t)split * p.M + m) * p.Npad;
#pragma unroll
    for (int g = 0; g < NG; ++g)
      if (4 * g < p.Npad) *reinterpret_cast<float4*>(dst + 4 * g) = make_float4(acc[g][0], acc[g][1], acc[g][2], acc[g][3]);
    return;
  }
  const int n = m / HoWo, rem = m - n * HoWo;
  const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
  float* dst = p.y + (size_t)((n * p.yH + oy * p.ymul + p.yoff) * p.yW + ox * p.xmul + p.xoff) * p.ycs;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int col = 4 * g;
    if (col >= p.Cout) break;
    float v[4] = {acc[g][0], acc[g][1], acc[g][2], acc[g][3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (p.bias && col + j < p.Cout) v[j] += p.bias[col + j];
      v[j] = act_apply(v[j], p.act);
    }
    if (col + 3 < p.Cout) {
      float4 o = make_float4(v[0], v[1], v[2], v[3]);
      if (p.accumulate) {
        const float4 old = *reinterpret_cast<const float4*>(dst + col);
        o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
      }
      *reinterpret_cast<float4*>(dst + col) = o;
    } else {
      for (int j = 0; j < 4 && col + j < p.Cout; ++j) dst[col + j] = p.accumulate ? dst[col + j] + v[j] : v[j];
    }
  }
}

// sums the K-split slabs in fixed order and applies the epilogue (4 output channels per thread)
__global__ void conv_fwd_reduce_kernel(GemmP p) {
  p.y += (size_t)blockIdx.z * p.y_bs; p.slab += (size_t)blockIdx.z * p.slab_bs;
  apply_phase(p);
  const int C4 = (p.Cout + 3) >> 2;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)p.M * C4;
  if (i >= total) return;
  const int m = (int)(i / C4), col = (int)(i - (size_t)m * C4) * 4;
  float4 a = *reinterpret_cast<const float4*>(p.slab + (size_t)m * p.Npad + col);   // Npad % 4 == 0
  for (int s = 1; s < p.splits; ++s) {
    const float4 b = *reinterpret_cast<const float4*>(p.slab + ((size_t)s * p.M + m) * p.Npad + col);
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
// wgrad-type kernel: rows = k (BM of them), cols = co, reduction over pixels
// ---------------------------------------------------------------------------------------
// NG > 0: narrow-N variant (Tile<2,1,4,1>: 256 k-rows x <= 32 channels): one k-row per lane,
// dY[m][4g..4g+3] broadcast from lanes 4g..4g+3, v_mfma_f32_4x4x1 as in conv_fwd_narrow_kernel.
// ROWU: Wo % 32 == 0, or Wo | 32 with Ho*Wo % 32 == 0: the 32 pixels of a stage lie inside one image at fixed
// offsets from its first pixel, whose decode is wave-uniform.
template <int MT, int NT, int WGM, int WGN, int NG = 0, bool ROWU = false>
__global__ __launch_bounds__(64 * WGM * WGN) void conv_wgrad_kernel(GemmP p) {
  using T = Tile<MT, NT, WGM, WGN>;
  constexpr int BM = T::BM, BN = T::BN;
  constexpr int NTHR = 64 * WGM * WGN;
  constexpr int AROWS = NTHR / (BM / 4), BROWS = NTHR / (BN / 4);   // pixel rows of the [32][BM] / [32][BN] tiles per pass
  constexpr int RA = 32 / AROWS;       // float4 per thread
  constexpr int RB = 32 / BROWS;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                    // [2][32*BM]
  float* Bs = smem + 2 * 32 * BM;      // [2][32*BN]

  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int wm = wid / WGN, wn = wid % WGN;
  const int tile = xcd_swizzle(blockIdx.x, p.ntiles);
  const int tile_n = tile % p.tiles_n, tile_k = tile / p.tiles_n;
  const int kt0 = tile_k * BM, n0 = tile_n * BN;
  const int split = blockIdx.y;
  p.x += (size_t)blockIdx.z * p.x_bs; p.y += (size_t)blockIdx.z * p.y_bs;
  p.w += (size_t)blockIdx.z * p.w_bs; p.slab += (size_t)blockIdx.z * p.slab_bs;
  apply_phase(p);

  // this thread's k (fixed for the whole kernel)
  const int acol = (t % (BM / 4)) * 4, arow0 = t / (BM / 4);
  const int k = kt0 + acol;
  const bool kvalid = k < p.K;
  const int tap = k / p.xC, ci = k - tap * p.xC;
  const int kh = tap / p.KW, kw = tap - kh * p.KW;
  const int bcol = (t % (BN / 4)) * 4, brow0 = t / (BN / 4);
  const bool nvalid = (n0 + bcol) < p.yC;
  const int He = p.xH << p.ups, We = p.xW << p.ups;
  const int HoWo = p.Ho * p.Wo;

  // per-row pixel cursors (n, oy, ox), advanced by 32 pixels per stage instead of being
  // re-derived with two integer divisions per row per stage
  const int nmb = (p.M + 31) / 32;
  const int mb_begin = split * p.per_split;
  const int mb_end = min(nmb, mb_begin + p.per_split);
  int an[RA], aoy[RA], aox[RA], bn[RB], boy[RB], box[RB];
  auto decode = [&](int m, int& n, int& oy, int& ox) {
    n = m / HoWo; const int rem = m - n * HoWo;
    oy = rem / p.Wo; ox = rem - oy * p.Wo;
  };
  auto advance = [&](int& n, int& oy, int& ox) {
    ox += 32;
    if (ox >= p.Wo) {
      const int q = ox / p.Wo;
      ox -= q * p.Wo; oy += q;
      if (oy >= p.Ho) { const int r = oy / p.Ho; oy -= r * p.Ho; n += r; }
    }
  };
  // ROWU: offsets of this thread's rows inside a 32-pixel stage (the stage starts at ox = 0 unless Wo % 32 == 0)
  int a_dy[RA], a_dx[RA], b_dy[RB], b_dx[RB];
  if constexpr (ROWU) {
    const bool wide = (p.Wo & 31) == 0;
#pragma unroll
    for (int r = 0; r < RA; ++r) {
      const int j = arow0 + r * AROWS;
      a_dy[r] = wide ? 0 : j / p.Wo; a_dx[r] = wide ? j : j % p.Wo;
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int j = brow0 + r * BROWS;
      b_dy[r] = wide ? 0 : j / p.Wo; b_dx[r] = wide ? j : j % p.Wo;
    }
  }
  if constexpr (!ROWU) {
#pragma unroll
    for (int r = 0; r < RA; ++r) decode(mb_begin * 32 + arow0 + r * AROWS, an[r], aoy[r], aox[r]);
#pragma unroll
    for (int r = 0; r < RB; ++r) decode(mb_begin * 32 + brow0 + r * BROWS, bn[r], boy[r], box[r]);
  }
  const int ximg = p.xH * p.xW * p.xcs;

  float4 ra[RA], rb[RB];
  auto load_tiles = [&](int mb) {
    const int mbase = mb * 32;
    if constexpr (ROWU) {
      // one scalar decode per stage; a thread's rows sit at fixed (dy, dx) from the stage's first pixel
      const int n = mbase / HoWo, rem = mbase - n * HoWo;
      const int oy0 = rem / p.Wo, ox0 = rem - oy0 * p.Wo;
      const bool live = mbase < p.M;                       // M % 32 == 0 here: a stage is all-valid or empty
      const float* ximg_p = p.x + (size_t)n * ximg + ci;
      const bool arow_ok = live && kvalid;
#pragma unroll
      for (int r = 0; r < RA; ++r) {
        const int sy = src_coord((oy0 + a_dy[r]) * p.stride - p.pad_t + kh, He, p.pad_mode, p.ups);
        const int sx = src_coord((ox0 + a_dx[r]) * p.stride - p.pad_l + kw, We, p.pad_mode, p.ups);
        ra[r] = (arow_ok && sy >= 0 && sx >= 0) ? *reinterpret_cast<const float4*>(ximg_p + (size_t)(sy * p.xW + sx) * p.xcs)
                                                : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      const float* yimg_p = p.y + ((size_t)(n * p.yH + p.yoff) * p.yW + p.xoff) * p.ycs + n0 + bcol;
      const bool brow_ok = live && nvalid;
#pragma unroll
      for (int r = 0; r < RB; ++r)
        rb[r] = brow_ok ? *reinterpret_cast<const float4*>(
                              yimg_p + (size_t)((oy0 + b_dy[r]) * p.ymul * p.yW + (ox0 + b_dx[r]) * p.xmul) * p.ycs)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
      return;
    }
#pragma unroll
    for (int r = 0; r < RA; ++r) {
      const int m = mbase + arow0 + r * AROWS;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < p.M && kvalid) {
        const int sy = src_coord(aoy[r] * p.stride - p.pad_t + kh, He, p.pad_mode, p.ups);
        const int sx = src_coord(aox[r] * p.stride - p.pad_l + kw, We, p.pad_mode, p.ups);
        if (sy >= 0 && sx >= 0)
          v = *reinterpret_cast<const float4*>(p.x + (size_t)an[r] * ximg + (size_t)(sy * p.xW + sx) * p.xcs + ci);
      }
      ra[r] = v;
      advance(an[r], aoy[r], aox[r]);
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int m = mbase + brow0 + r * BROWS;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < p.M && nvalid)
        v = *reinterpret_cast<const float4*>(
            p.y + (size_t)((bn[r] * p.yH + boy[r] * p.ymul + p.yoff) * p.yW + box[r] * p.xmul + p.xoff) * p.ycs + n0 + bcol);
      rb[r] = v;
      advance(bn[r], boy[r], box[r]);
    }
  };
  auto store_tiles = [&](int buf) {
    float* A = As + buf * 32 * BM;
#pragma unroll
    for (int r = 0; r < RA; ++r) *reinterpret_cast<float4*>(A + (arow0 + r * AROWS) * BM + acol) = ra[r];
    float* B = Bs + buf * 32 * BN;
#pragma unroll
    for (int r = 0; r < RB; ++r) *reinterpret_cast<float4*>(B + (brow0 + r * BROWS) * BN + bcol) = rb[r];
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  f32x4 nacc[NG > 0 ? NG : 1];
#pragma unroll
  for (int g = 0; g < (NG > 0 ? NG : 1); ++g) nacc[g] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int buf) {
    if constexpr (NG > 0) {
      const float* A = As + buf * 32 * BM + wid * 64 + lane;     // im2col column k of this lane
      const float* B = Bs + buf * 32 * BN + (lane & 31);         // dY[.][lane]
      float xv[32], dv[32];
#pragma unroll
      for (int st = 0; st < 32; ++st) { xv[st] = A[st * BM]; dv[st] = B[st * BN]; }
#pragma unroll
      for (int st = 0; st < 32; ++st) NarrowMac<0, (NG > 0 ? NG : 1)>::run(nacc, dv[st], xv[st]);
      return;
    }
    const float* A = As + buf * 32 * BM + (lane >> 5) * BM + wm * MT * 32 + (lane & 31);
    const float* B = Bs + buf * 32 * BN + (lane >> 5) * BN + wn * NT * 32 + (lane & 31);
    float af[MT][16], bf[NT][16];
#pragma unroll
    for (int st = 0; st < 16; ++st) {
#pragma unroll
      for (int i = 0; i < MT; ++i) af[i][st] = A[2 * st * BM + i * 32];
#pragma unroll
      for (int j = 0; j < NT; ++j) bf[j][st] = B[2 * st * BN + j * 32];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int st = 0; st < 16; ++st)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][st], bf[j][st], acc[i][j], 0, 0, 0);
  };

  if (mb_begin < mb_end) {
    load_tiles(mb_begin);
    store_tiles(0);
    __syncthreads();
    int cur = 0;
    for (int mb = mb_begin; mb < mb_end; ++mb) {
      const bool more = mb + 1 < mb_end;
      if (more) load_tiles(mb + 1);
      compute(cur);
      if (more) store_tiles(cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }
  }
  float* out = p.splits > 1 ? p.slab + (size_t)split * p.K * p.Npad : const_cast<float*>(p.w);
  if constexpr (NG > 0) {
    const int row = kt0 + wid * 64 + lane;
    if (row < p.K) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (4 * g < p.Npad)
          *reinterpret_cast<float4*>(out + (size_t)row * p.Npad + 4 * g) = make_float4(nacc[g][0], nacc[g][1], nacc[g][2], nacc[g][3]);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = n0 + wn * NT * 32 + j * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = kt0 + wm * MT * 32 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (row < p.K && col < p.Npad) out[(size_t)row * p.Npad + col] = acc[i][j][e];
      }
    }
}

// sums the `splits` slabs of n floats: 16 outputs (float4) x 16 slab groups per block -- group g adds slabs g, g+16, ...
// in index order, then the 16 group sums are added in index order (fixed order: deterministic).  With hundreds of slabs
// of a small weight tensor (first-layer weight gradients: 250-500 slabs of 24 K floats) one thread per output walking
// all slabs is latency-bound (98 us); spreading the slab axis over the block makes it a 10 us kernel.
__global__ __launch_bounds__(256) void slab_sum_kernel(const float* slab, float* out, size_t n, int splits, size_t slab_bs, size_t out_bs) {
  __shared__ float4 red[256];
  slab += (size_t)blockIdx.y * slab_bs; out += (size_t)blockIdx.y * out_bs;
  const int o = threadIdx.x & 15, g = threadIdx.x >> 4;
  const size_t i = ((size_t)blockIdx.x * 16 + o) * 4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n)
    for (int sp = g; sp < splits; sp += 16) {
      const float4 b = *reinterpret_cast<const float4*>(slab + (size_t)sp * n + i);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
  red[threadIdx.x] = a;
  __syncthreads();
  if (g == 0 && i < n) {
    float4 t = red[o];
    for (int k = 1; k < 16; ++k) { const float4 b = red[k * 16 + o]; t.x += b.x; t.y += b.y; t.z += b.z; t.w += b.w; }
    *reinterpret_cast<float4*>(out + i) = t;
  }
}

// ---------------------------------------------------------------------------------------
// naive references (verification only)
// ---------------------------------------------------------------------------------------
__global__ void conv_fwd_naive_kernel(GemmP p) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)p.M * p.Cout) return;
  const int m = (int)(i / p.Cout), co = (int)(i - (size_t)m * p.Cout);
  const int HoWo = p.Ho * p.Wo;
  const int n = m / HoWo, rem = m - n * HoWo;
  const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
  const int He = p.xH << p.ups, We = p.xW << p.ups;
  float acc = 0.f;
  for (int kh = 0; kh < p.KH; ++kh)
    for (int kw = 0; kw < p.KW; ++kw) {
      const int sy = src_coord(oy * p.stride - p.pad_t + kh, He, p.pad_mode, p.ups);
      const int sx = src_coord(ox * p.stride - p.pad_l + kw, We, p.pad_mode, p.ups);
      if (sy < 0 || sx < 0) continue;
      const float* xp = p.x + (size_t)n * p.xH * p.xW * p.xcs + (size_t)(sy * p.xW + sx) * p.xcs;
      const float* wp = p.w + (size_t)((kh * p.KW + kw) * p.xC) * p.Npad + co;
      for (int ci = 0; ci < p.xC; ++ci) acc = fmaf(xp[ci], wp[(size_t)ci * p.Npad], acc);
    }
  if (p.bias) acc += p.bias[co];
  acc = act_apply(acc, p.act);
  float* dst = p.y + (size_t)((n * p.yH + oy * p.ymul + p.yoff) * p.yW + ox * p.xmul + p.xoff) * p.ycs + co;
  if (p.accumulate) acc += *dst;
  *dst = acc;
}

__global__ void conv_wgrad_naive_kernel(GemmP p) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)p.K * p.Npad) return;
  const int k = (int)(i / p.Npad), co = (int)(i - (size_t)k * p.Npad);
  float* dw = const_cast<float*>(p.w);
  if (co >= p.Cout) { dw[i] = 0.f; return; }
  const int tap = k / p.xC, ci = k - tap * p.xC;
  const int kh = tap / p.KW, kw = tap - kh * p.KW;
  const int He = p.xH << p.ups, We = p.xW << p.ups;
  const int HoWo = p.Ho * p.Wo;
  double acc = 0.0;
  for (int m = 0; m < p.M; ++m) {
    const int n = m / HoWo, rem = m - n * HoWo;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    const int sy = src_coord(oy * p.stride - p.pad_t + kh, He, p.pad_mode, p.ups);
    const int sx = src_coord(ox * p.stride - p.pad_l + kw, We, p.pad_mode, p.ups);
    if (sy < 0 || sx < 0) continue;
    const float xv = p.x[(size_t)n * p.xH * p.xW * p.xcs + (size_t)(sy * p.xW + sx) * p.xcs + ci];
    const float dv = p.y[(size_t)((n * p.yH + oy * p.ymul + p.yoff) * p.yW + ox * p.xmul + p.xoff) * p.ycs + co];
    acc += (double)xv * dv;
  }
  dw[i] = (float)acc;
}

// ---------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------
// trailer of a forward-type launch that split K: the slabs summed in fixed order, then the epilogue
static void reduce_split_k(Stream& s, const GemmP& p, int batch) {
  if (p.splits <= 1) return;
  const size_t total = (size_t)p.M * ((p.Cout + 3) / 4);
  hipLaunchKernelGGL(conv_fwd_reduce_kernel, dim3((unsigned)((total + 255) / 256), 1, batch), dim3(256), 0, hs(s), p);
  check_launch("conv_fwd_reduce");
}

template <int MT, int NT, int WGM, int WGN>
static void launch_fwd(Stream& s, GemmP& p, bool fast, int batch) {
  using T = Tile<MT, NT, WGM, WGN>;
  const int tiles_m = ceil_div(p.M, T::BM);
  p.tiles_n = ceil_div(p.Npad, T::BN);
  p.ntiles = tiles_m * p.tiles_n;
  const int nkb = ceil_div(p.K, 32);
  const int slots = 256 * (T::SMEM_FWD > 80 * 1024 ? 1 : (T::SMEM_FWD > 64 * 1024 ? 2 : 3));
  const int splits = choose_splits(p.ntiles * batch, nkb, slots, 8, (size_t)p.M * p.Npad * 4 * batch, s.ws_bytes);
  p.per_split = ceil_div(nkb, splits);
  p.splits = ceil_div(nkb, p.per_split);
  p.slab = reinterpret_cast<float*>(s.ws);
  p.slab_bs = (size_t)p.M * p.Npad * p.splits;      // per batch
  dim3 grid(p.ntiles, p.splits, batch);
  char pname[128];
  prof_name(pname, "conv_fwd_%dx%d_%s", "[M%d,N%d,K%d,s%d]", T::BM, T::BN, fast ? "fast" : "generic", p.M, p.Cout, p.K, p.splits);
  ProfScope prof(s, pname, 2.0 * p.M * p.Cout * p.K * batch);
  if (fast) {
    static bool once = (set_smem(conv_fwd_kernel<MT, NT, WGM, WGN, true>, T::SMEM_FWD), true);
    (void)once;
    hipLaunchKernelGGL((conv_fwd_kernel<MT, NT, WGM, WGN, true>), grid, dim3(64 * WGM * WGN), T::SMEM_FWD, hs(s), p);
  } else {
    static bool once = (set_smem(conv_fwd_kernel<MT, NT, WGM, WGN, false>, T::SMEM_FWD), true);
    (void)once;
    hipLaunchKernelGGL((conv_fwd_kernel<MT, NT, WGM, WGN, false>), grid, dim3(64 * WGM * WGN), T::SMEM_FWD, hs(s), p);
  }
  check_launch("conv_fwd");
  reduce_split_k(s, p, batch);
}
void launch_fwd_direct(Stream& s, GemmP& p, FwdTile tile, bool fast, int batch) {
  switch (tile) {
    case FWD_128x192: return launch_fwd<2, 3, 2, 2>(s, p, fast, batch);
    case FWD_256x128: return launch_fwd<2, 2, 4, 2>(s, p, fast, batch);
    case FWD_128x128: return launch_fwd<2, 2, 2, 2>(s, p, fast, batch);
    case FWD_128x64: return launch_fwd<2, 1, 2, 2>(s, p, fast, batch);   // (a 2-wave 128x64 tile with 64x64 wave tiles measured 4 % slower)
    case FWD_128x32: return launch_fwd<1, 1, 4, 1>(s, p, fast, batch);
  }
  throw Error(1, "conv_fwd: unknown register-staged tile");
}

template <int NG>
static void launch_fwd_narrow_ng(Stream& s, GemmP& p, bool fast, int batch) {
  using T = NarrowTile;
  p.tiles_n = 1;
  p.ntiles = ceil_div(p.M, T::BM);
  const int nkb = ceil_div(p.K, T::BK);
  const int slots = 256 * 3;
  const int splits = choose_splits(p.ntiles * batch, nkb, slots, 16, (size_t)p.M * p.Npad * 4 * batch, s.ws_bytes);
  p.per_split = ceil_div(nkb, splits);
  p.splits = ceil_div(nkb, p.per_split);
  p.slab = reinterpret_cast<float*>(s.ws);
  p.slab_bs = (size_t)p.M * p.Npad * p.splits;
  dim3 grid(p.ntiles, p.splits, batch);
  char pname[128];
  prof_name(pname, "conv_fwd_narrow%d_%s", "[M%d,N%d,K%d,s%d]", 4 * NG, fast ? "fast" : "generic", p.M, p.Cout, p.K, p.splits);
  ProfScope prof(s, pname, 2.0 * p.M * p.Cout * p.K * batch);
  if (fast) hipLaunchKernelGGL((conv_fwd_narrow_kernel<NG, true>), grid, dim3(256), T::SMEM, hs(s), p);
  else hipLaunchKernelGGL((conv_fwd_narrow_kernel<NG, false>), grid, dim3(256), T::SMEM, hs(s), p);
  check_launch("conv_fwd_narrow");
  reduce_split_k(s, p, batch);
}
void launch_fwd_narrow(Stream& s, GemmP& p, int ng, bool fast, int batch) {
  switch (ng) {
    case 1: return launch_fwd_narrow_ng<1>(s, p, fast, batch);
    case 2: return launch_fwd_narrow_ng<2>(s, p, fast, batch);
    case 4: return launch_fwd_narrow_ng<4>(s, p, fast, batch);
    case 5: return launch_fwd_narrow_ng<5>(s, p, fast, batch);
    case 6: return launch_fwd_narrow_ng<6>(s, p, fast, batch);
    case 8: return launch_fwd_narrow_ng<8>(s, p, fast, batch);
  }
  throw Error(1, "conv_fwd: unknown narrow tile");
}

void slab_sum(Stream& s, const float* slab, float* out, size_t n, int splits, int batch, size_t slab_bs, size_t out_bs) {
  hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)((n / 4 + 15) / 16), batch), dim3(256), 0, hs(s), slab, out, n, splits, slab_bs, out_bs);
  check_launch("slab_sum");
}

template <int MT, int NT, int WGM, int WGN, int NG = 0, bool ROWU = false>
static void launch_wgrad(Stream& s, GemmP& p, int batch) {
  if constexpr (!ROWU) {
    // a 32-pixel stage lies inside one image and starts at a row start (or inside one row)
    const bool rowu = p.M % 32 == 0 && (p.Wo % 32 == 0 || (32 % p.Wo == 0 && (p.Ho * p.Wo) % 32 == 0));
    if (rowu) { launch_wgrad<MT, NT, WGM, WGN, NG, true>(s, p, batch); return; }
  }
  using T = Tile<MT, NT, WGM, WGN>;
  const int tiles_k = ceil_div(p.K, T::BM);
  p.tiles_n = ceil_div(p.Npad, T::BN);
  p.ntiles = tiles_k * p.tiles_n;
  const int nmb = ceil_div(p.M, 32);
  const int slots = 256 * (T::SMEM_WG > 80 * 1024 ? 1 : (T::SMEM_WG >= 64 * 1024 ? 2 : (T::SMEM_WG >= 48 * 1024 ? 3 : 4)));
  const int splits = choose_splits(p.ntiles * batch, nmb, slots, 8, (size_t)p.K * p.Npad * 4 * batch, s.ws_bytes);
  p.per_split = ceil_div(nmb, splits);
  p.splits = ceil_div(nmb, p.per_split);
  p.slab = reinterpret_cast<float*>(s.ws);
  p.slab_bs = (size_t)p.K * p.Npad * p.splits;
  static bool once = (set_smem(conv_wgrad_kernel<MT, NT, WGM, WGN, NG, ROWU>, T::SMEM_WG), true);
  (void)once;
  char pname[128];
  prof_name(pname, "conv_wgrad_%dx%d", "[M%d,N%d,K%d,s%d]", T::BM, NG > 0 ? 4 * NG : T::BN, p.M, p.Cout, p.K, p.splits);
  ProfScope prof(s, pname, 2.0 * p.M * p.Cout * p.K * batch);
  hipLaunchKernelGGL((conv_wgrad_kernel<MT, NT, WGM, WGN, NG, ROWU>), dim3(p.ntiles, p.splits, batch), dim3(64 * WGM * WGN),
                     T::SMEM_WG, hs(s), p);
  check_launch("conv_wgrad");
  if (p.splits > 1) slab_sum(s, p.slab, const_cast<float*>(p.w), (size_t)p.K * p.Npad, p.splits, batch, p.slab_bs, p.w_bs);
}
void launch_wgrad_direct(Stream& s, GemmP& p, WgradTile tile, int batch) {
  switch (tile) {
    case WGRAD_256x128: return launch_wgrad<2, 2, 4, 2>(s, p, batch);
    case WGRAD_128x128: return launch_wgrad<2, 2, 2, 2>(s, p, batch);
    case WGRAD_128x64: return launch_wgrad<2, 1, 2, 2>(s, p, batch);
    case WGRAD_128x32: return launch_wgrad<1, 1, 4, 1>(s, p, batch);
    case WGRAD_256x4: return launch_wgrad<2, 1, 4, 1, 1>(s, p, batch);
    case WGRAD_256x8: return launch_wgrad<2, 1, 4, 1, 2>(s, p, batch);
  }
  throw Error(1, "conv_wgrad: unknown register-staged tile");
}

static void host_phase(GemmP& q, int ph) {
  if (!q.phases) return;
  q.pad_t -= ph >> 1; q.pad_l -= ph & 1; q.yoff = ph >> 1; q.xoff = ph & 1;
  q.phases = 0;
}

void conv_fwd_naive(Stream& s, const ConvFwdArgs& a) {
  GemmP p = fwd_params(a, a.om);
  const size_t total = (size_t)p.M * p.Cout;
  for (int b = 0; b < (a.phases ? a.phases : std::max(a.batch, 1)); ++b) {
    GemmP q = p;
    host_phase(q, b);
    q.x += (size_t)b * a.x_bs; q.w += (size_t)b * a.w_bs; q.y += (size_t)b * a.y_bs;
    hipLaunchKernelGGL(conv_fwd_naive_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, hs(s), q);
  }
  check_launch("conv_fwd_naive");
}

void conv_wgrad_naive(Stream& s, const ConvWgradArgs& a) {
  GemmP p = wgrad_params(a, a.om);
  const size_t total = (size_t)p.K * p.Npad;
  for (int b = 0; b < (a.phases ? a.phases : std::max(a.batch, 1)); ++b) {
    GemmP q = p;
    host_phase(q, b);
    q.x += (size_t)b * a.x_bs; q.y += (size_t)b * a.dy_bs; q.w += (size_t)b * a.dw_bs;
    hipLaunchKernelGGL(conv_wgrad_naive_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, hs(s), q);
  }
  check_launch("conv_wgrad_naive");
}

}  // namespace swn
