// swapnet_amd -- what the implicit-GEMM convolution units share.  Internal: the engine sees ops.h only.
//   conv_gemm.hip        launch parameters, schedule planners, SWN_* switches, the dispatchers conv_fwd / conv_wgrad
//   conv_direct.hip      register-staged kernels (wide, narrow-N, naive references) and their split-K reductions
//   conv_ring.hip        kernels on the LDS-DMA ring: forward-type (fp32 and pre-cut weight operand), weight gradient; operand amax, pre-cut
//   conv_tail.hip        fused four-phase kernels (folded tail conv, narrow transposed convs)
//   prof.hip             per-launch event profiling, the MFMA throughput probe
// A kernel is instantiated by the unit that holds it; the dispatchers name a tile by an enum (or its column width) and the unit's
// exported launcher maps that back to the template.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "hip_util.h"

namespace swn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct GemmP {
  const float* x; int xH, xW, xC, xcs;
  int KH, KW, stride, pad_t, pad_l, pad_mode, ups;
  int Ho, Wo, M, K;
  const float* w; int Npad;
  const float* bias; int act; int accumulate;
  float* y; int yH, yW, ycs; int ymul, yoff, xmul, xoff; int Cout; int yC;
  int splits; int per_split; float* slab;
  int tiles_n; int ntiles;
  size_t x_bs, w_bs, y_bs, slab_bs;   // batched mode (blockIdx.z)
  int phases;                         // sub-pixel phase mode: blockIdx.z = 2a + b shifts pads / output offsets
  int tail4;                          // fused folded-tail kernels
  float* y_amax;                      // optional amax slot of everything the launch stores (pre-cut ring kernel + its reduce)
  double* stat;                       // optional InstanceNorm partial sums of the output (ops.h ConvFwdArgs::stat_partial): 128 x 128 pre-cut kernel
};

__device__ __forceinline__ void apply_phase(GemmP& p) {
  if (p.phases) {
    const int a = blockIdx.z >> 1, b = blockIdx.z & 1;
    p.pad_t -= a; p.pad_l -= b; p.yoff = a; p.xoff = b;
  }
}

__device__ __forceinline__ int src_coord(int e, int ext, int pad_mode, int ups) {
  if (pad_mode == PAD_REFLECT) {
    if (e < 0) e = -e;
    else if (e >= ext) e = 2 * ext - 2 - e;
  } else if (e < 0 || e >= ext) {
    return -1;
  }
  return e >> ups;
}

// XCD-aware tile order: the dispatcher round-robins consecutive workgroups over the 8
// XCDs; give each XCD a contiguous run of tiles so neighbouring tiles (same A rows /
// same weight panel) share one L2.  Bijective for any tile count.
__device__ __forceinline__ int xcd_swizzle(int bid, int n) {
  const int q = n >> 3, r = n & 7, xcd = bid & 7, i = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
}

// ---- LDS-DMA ring (conv_ring.hip): global -> LDS by `buffer_load_dwordx4 ... lds` -----------------------
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// raw buffer descriptor: stride 0, num_records = bytes, gfx9 raw-buffer flags; offsets >= bytes read 0
__device__ __forceinline__ i32x4 make_rsrc(const void* ptr, unsigned bytes) {
  const unsigned long long a = (unsigned long long)ptr;
  i32x4 r;
  r[0] = (int)(unsigned)(a & 0xffffffffull); r[1] = (int)(unsigned)((a >> 32) & 0xffffull); r[2] = (int)bytes; r[3] = 0x00020000;
  return r;
}
// one LDS-DMA instruction: lane i fetches 16 bytes at base + voff + soff, the wave's 1 KiB lands at LDS byte lds_dst + 16 i
__device__ __forceinline__ void lds_dma16(unsigned voff, i32x4 rsrc, unsigned soff, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(lds_dst), "s"(soff) : "memory");
}
constexpr unsigned DMA_OOB = 0x80000000u;      // > any buffer this library addresses (checked by the launcher)

// ---- fp32 products on the bf16 matrix cores ("split" main loop) ------------------------------------------------------
// x = hi + mid + lo with 8 mantissa bits each, cut by TRUNCATION, so the split itself is exact (24 bits in, 24 bits out).
// a*b = sum of 9 partial products; the 6 with weight >= 2^-16 relative to hi*hi are formed by
// v_mfma_f32_32x32x16_bf16 (each bf16 x bf16 product is exact in fp32, accumulation is fp32); the three dropped ones
// (mid*lo, lo*mid, lo*lo) are below 2^-24 |a||b|, i.e. below the rounding of an fp32 product.  Measured against an
// fp64-accumulated reference the result is slightly MORE accurate than v_mfma_f32_32x32x2_f32 (5.0e-7 vs 5.7e-7 rel-L2
// at K = 1024: 16 products per accumulator rounding instead of 2), and the 6 MFMAs per 16 k cost 192 cycles of the
// matrix pipe against 512 for the f32 form (tools/gemm_lab_split.hip: 110 -> 162 fp32-equivalent TFLOP/s; the loop is
// then bound by the ~5.5 VALU instructions per element of the split).  A lane's 8 fragment values are k = 8h .. 8h+7
// of its row / column -- exactly the operand layout of the 32x32x16 instruction.  SWN_SPLIT=0 selects the f32 MFMA.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void split8(const float* v, u32x4& hi, u32x4& mid, u32x4& lo) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned x0 = __float_as_uint(v[2 * q]), x1 = __float_as_uint(v[2 * q + 1]);
    hi[q] = __builtin_amdgcn_perm(x1, x0, 0x07060302u);                 // {x1[31:16], x0[31:16]}
    const float r0 = v[2 * q] - __uint_as_float(x0 & 0xffff0000u), r1 = v[2 * q + 1] - __uint_as_float(x1 & 0xffff0000u);
    const unsigned y0 = __float_as_uint(r0), y1 = __float_as_uint(r1);
    mid[q] = __builtin_amdgcn_perm(y1, y0, 0x07060302u);
    const float s0 = r0 - __uint_as_float(y0 & 0xffff0000u), s1 = r1 - __uint_as_float(y1 & 0xffff0000u);
    lo[q] = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
  }
}
__device__ __forceinline__ f32x16 mma_bf16(u32x4 a, u32x4 b, f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
#else
  return c;
#endif
}
// acc[i][j] += A_i (rows) x B_j (columns) over the lane's 8 k values, i, j in {0, 1}
__device__ __forceinline__ void split_mma_2x2(f32x16 (&acc)[2][2], const float (&af)[2][8], const float (&bf)[2][8]) {
  u32x4 ah[2], am[2], al[2], bh[2], bm[2], bl[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) { split8(af[i], ah[i], am[i], al[i]); split8(bf[i], bh[i], bm[i], bl[i]); }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f32x16 c = acc[i][j];
      c = mma_bf16(al[i], bh[j], c); c = mma_bf16(ah[i], bl[j], c); c = mma_bf16(am[i], bm[j], c);     // smallest terms first
      c = mma_bf16(am[i], bh[j], c); c = mma_bf16(ah[i], bm[j], c); c = mma_bf16(ah[i], bh[j], c);
      acc[i][j] = c;
    }
}


struct DmaSched {            // hybrid schedule, computed by the launcher
  int full;                  // work units [0, full): one whole tile each
  int tail_tiles, tail_s;    // then tail_tiles tiles split tail_s ways along K
  int per_split;             // stages per split of a tail tile
  int tiles_per_z;           // tiles of one batch element / phase
  // > 0 (the four sub-pixel phases of one launch, pre-cut ring kernel): z is the FAST index of the tile order, gtile = tile * zfast + z.
  // The phases of a launch gather the same input through different tap offsets: with z slow, an XCD's contiguous run of tiles
  // (xcd_swizzle) is part of ONE phase and the same input region is fetched by the four XCDs that hold its four phases
  int zfast;
};

template <int WGM, int WGN>
struct DmaTile {
  static constexpr int NW = WGM * WGN, BM = 64 * WGM, BN = 64 * WGN, BK = 16, NST = 3;
  static constexpr int A_FL = BM * BK, B_FL = BK * BN, ST_FL = A_FL + B_FL;
  static constexpr int AI = 4 / WGN, BI = 4 / WGM;       // LDS-DMA instructions per wave per stage
  static constexpr int LPR = BN / 4, RPI = 64 / LPR;     // lanes per B row, B rows per instruction
  static constexpr int SMEM = NST * ST_FL * 4;
  static_assert(4 % WGN == 0 && 4 % WGM == 0, "tile shape");
};

// the same instruction with m0 declared clobbered instead of saved and restored (the pre-cut and the plane-form loaders)
__device__ __forceinline__ void lds_dma16c(unsigned voff, i32x4 rsrc, unsigned soff, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
               : : "v"(voff), "s"(rsrc), "s"(lds_dst), "s"(soff) : "memory", "m0");
}

// ---- two fp16 planes instead of three bf16 ones (round 3, late; tools/ring_lab.hip gemm_h) -------------------------------------
// The six-term bf16 loop sits on the chip's POWER cap, not on an issue limit: with random operands every lab variant (no VALU
// at all, 16x16x32 MFMAs, 8 accumulators, one barrier per 32 k) lands at 180-200 fp32-equivalent TFLOP/s while the shader clock
// falls to 1.1-1.3 GHz (s_memtime / s_memrealtime inside the kernel), and zero-filled operands run the same binary at
// 1.7-2.0 GHz and 233-269 (profiles/ring_lab_r03_clock.txt).  So the remaining factor is in the matrix work per product:
// x = h + l with h = fp16(x), l = fp16(x - h) carries 22 mantissa bits, and h h + h l + l h is THREE MFMAs at an error of the
// dropped l l term, 2^-22 relative (lab: 3.9e-7 rel-L2 against 5.0e-7 for the six bf16 terms, 300-325 TFLOP/s against 183).
// fp16's exponent range is what this costs: each operand is scaled by a power of two chosen from its amax (exact, removed
// from the fp32 accumulators in the epilogue): A -- the activations / gradients cut in the loop -- from 256 partial maxima
// that amax_partials_kernel leaves in the stream scratch right before the launch (amax * 2^kA in [2^11, 2^12): overflow-free
// with a factor 16 to spare, 22 bits for every element within 2^-14 of the largest, an ABSOLUTE floor of amax * 2^-37
// below); B -- the pre-cut weight operand -- by its producer (amax of the source * 2^kB in [2^9, 2^10), derived operands
// such as Winograd-transformed filters stay within a factor 32 of that), which stores kB in a 16-byte trailer of the panel.
// Unscaled gradient-magnitude operands lose everything (lab: 1.2e-1), a scale off by 2^-8 costs two digits (3.7e-5), a
// scale too large by 2^8 nothing: profiles/ring_lab_r03_range.txt.  SWN_PC_PLANES=3 keeps the bf16 form.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x16 mma_f16(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// The low plane of two elements, l = fp16(x - h), as one v_fma_mix{lo,hi}_f16 each (round 6).  x - h is exact in fp32 whatever the rounding
// of h (h holds x's leading 11 bits: the difference has at most 13 significant bits), so the single rounding of the fused x * 1 - h equals
// the v_cvt_f32_f16 / v_sub_f32 / v_cvt_f16_f32 sequence bit for bit (tools/mix_cut_check.hip on the MI355X: 0 mismatches over
// truncated and nearest h, normal and subnormal values) -- 4 VALU per pair with the packed multiply instead of the 8 the compiler
// emitted for most elements: the loops that cut an operand per 16-k step are VALU-bound (the generic weight-gradient loader:
// 146 VALU against 12 MFMAs per wave and stage).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned resid_pack(float x0, float x1, unsigned h) {
  unsigned l;
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(l) : "v"(x0), "v"(h));
  asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(x1), "v"(h));
  return l;
}
// h by truncation (one v_cvt_pkrtz for two elements), l rounded to nearest
__device__ __forceinline__ void split8h(const float* v, float sa, u32x4& hi, u32x4& lo) {
  const f32x2 s2 = f32x2{sa, sa};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x2 x = f32x2{v[2 * q], v[2 * q + 1]} * s2;
    const unsigned h = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(x[0], x[1]));
    hi[q] = h;
    lo[q] = resid_pack(x[0], x[1], h);
  }
}
// h rounded to NEAREST (v_cvt_pk_f16_f32): the residual l then has no preferred sign.  With both operands cut by truncation the
// dropped l_a l_b term always carries the sign of a b -- a relative bias of ~2^-22.6 on one-signed operands (measured: -1.5e-7 on
// post-ReLU x against positive dY); one operand rounded to nearest makes the term zero-mean.
__device__ __forceinline__ void split8h_rn(const float* v, float sa, u32x4& hi, u32x4& lo) {
  const f32x2 s2 = f32x2{sa, sa};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x2 x = f32x2{v[2 * q], v[2 * q + 1]} * s2;
    const unsigned h = __builtin_bit_cast(unsigned, f16x2{(_Float16)x[0], (_Float16)x[1]});
    hi[q] = h;
    lo[q] = resid_pack(x[0], x[1], h);
  }
}
// operand stored in PAIR form by its producer (wino.hip pair_word: {h | l << 16} per element): the two MFMA operands of 8
// consecutive k are byte permutes of the 8 words -- 8 VALU instead of the 32 of split8h
__device__ __forceinline__ void pair8(const float* w, u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned w0 = __float_as_uint(w[2 * q]), w1 = __float_as_uint(w[2 * q + 1]);
    hi[q] = __builtin_amdgcn_perm(w1, w0, 0x05040100u);                 // {w1[15:0], w0[15:0]}
    lo[q] = __builtin_amdgcn_perm(w1, w0, 0x07060302u);                 // {w1[31:16], w0[31:16]}
  }
}
// ONE fp16 plane (SWN_PC_PLANES=1 / SWN_WGRAD_PLANES=1, the reduced-precision configuration): h = fp16(x * 2^k) rounded to
// nearest, the low plane is not formed -- one MFMA per product, operands carry 11 mantissa bits (bf16 carries 8)
__device__ __forceinline__ void split8h1(const float* v, float sa, u32x4& hi) {
#pragma unroll
  for (int q = 0; q < 4; ++q) hi[q] = __builtin_bit_cast(unsigned, f16x2{(_Float16)(v[2 * q] * sa), (_Float16)(v[2 * q + 1] * sa)});
}
__device__ __forceinline__ void split_mma_2x2_h1(f32x16 (&acc)[2][2], const float (&af)[2][8], const float (&bf)[2][8], float sa, float sb) {
  u32x4 ah[2], bh[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) { split8h1(af[i], sa, ah[i]); split8h1(bf[i], sb, bh[i]); }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = mma_f16(ah[i], bh[j], acc[i][j]);
}
// both operands fp32 in LDS (the weight-gradient kernel): acc[i][j] += A_i x B_j over the lane's 8 k values, two fp16 planes each
__device__ __forceinline__ void split_mma_2x2_h(f32x16 (&acc)[2][2], const float (&af)[2][8], const float (&bf)[2][8], float sa, float sb) {
  u32x4 ah[2], al[2], bh[2], bl[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) { split8h(af[i], sa, ah[i], al[i]); split8h_rn(bf[i], sb, bh[i], bl[i]); }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f32x16 c = acc[i][j];
      c = mma_f16(al[i], bh[j], c); c = mma_f16(ah[i], bl[j], c); c = mma_f16(ah[i], bh[j], c);          // smallest terms first
      acc[i][j] = c;
    }
}
// k with amax * 2^k in [2^(top-1), 2^top); 0 for an all-zero (or non-finite) operand.  |k| <= 100 keeps 2^k a normal float.
__host__ __device__ __forceinline__ int scale_exp(float amax, int top) {
  if (!(amax > 0.f) || amax > 3.0e38f) return 0;
  unsigned bits; memcpy(&bits, &amax, 4);
  const int e = (int)((bits >> 23) & 255u) - 127;
  const int k = top - 1 - e;
  return k < -100 ? -100 : (k > 100 ? 100 : k);
}
__device__ __forceinline__ float pow2f(int k) { return __uint_as_float((unsigned)(127 + k) << 23); }
// every lane ends up with the maximum of the 256 partials (whole wave active)
__device__ __forceinline__ float amax256(const float* part, int lane) {
  float m = fmaxf(fmaxf(part[lane], part[lane + 64]), fmaxf(part[lane + 128], part[lane + 192]));
#pragma unroll
  for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  return m;
}
constexpr int PC_TOP_A = 12, PC_TOP_B = 10;
constexpr int PC_TRAILER = 8;           // bf16/f16 elements (16 bytes) behind a two-plane panel: int kB

template <int WGM, int NB, int NSTG, int PL = 2>
struct PcTile {
  static constexpr int NW = WGM, BM = 32 * WGM, BN = 32 * NB, BK = 16, NST = NSTG;
  static constexpr int A_BYTES = BM * BK * 4, B_BYTES = 2 * PL * BN * 16, ST_BYTES = A_BYTES + B_BYTES;
  static constexpr int APC = A_BYTES / 1024, BPC = B_BYTES / 1024;
  static constexpr int AI = APC / WGM, BI = BPC / WGM, BREM = BPC % WGM;   // pieces per wave; waves < BREM carry one more of B
  static constexpr int SMEM = NST * ST_BYTES;
  static_assert(APC % WGM == 0 && NB % 2 == 0 && (PL == 1 || PL == 2), "tile shape");
};

// v_mfma_f32_4x4x1 over NG column groups of 4 (conv_direct.hip narrow kernels, conv_tail.hip): acc[g] += w x for g = 0 .. NG-1
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int G, int NG>
struct NarrowMac {
  static __device__ __forceinline__ void run(f32x4* acc, float w, float x) {
    acc[G] = __builtin_amdgcn_mfma_f32_4x4x1f32(w, x, acc[G], 4, G, 0);
    NarrowMac<G + 1, NG>::run(acc, w, x);
  }
};
template <int NG>
struct NarrowMac<NG, NG> {
  static __device__ __forceinline__ void run(f32x4*, float, float) {}
};

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// per-launch profiling (prof.hip): HIP events on the launch stream around everything a launcher enqueues while the scope lives;
// the constructor also notes `name` in the route trace
struct ProfRec { std::string name; double flops; hipEvent_t a, b; };
struct ProfScope {
  hipStream_t st; bool on; ProfRec r;
  ProfScope(const Stream& s, const char* name, double flops);
  ~ProfScope();
};
// name of a launch for the profiler and the route trace: `base`, followed by `detail` (variant suffix and dimensions) when
// prof_detail(); printf-style, the arguments of both formats in order
void prof_name(char (&buf)[128], const char* base, const char* detail, ...);

template <typename K>
inline void set_smem(K kernel, int bytes) {
  SWN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
}

// ---- conv_gemm.hip
GemmP fwd_params(const ConvFwdArgs& a, const OutMap& om);        // checked launch parameters of a forward-type launch with output map om
GemmP wgrad_params(const ConvWgradArgs& a, const OutMap& om);
int choose_splits(int ntiles, int work, int slots, int min_work, size_t slab_bytes, size_t ws_bytes);
DmaSched plan_dma(int tiles_total, int tiles_per_z, int work, int slots, size_t tile_bytes, size_t ws_bytes,
                  double* cost_out = nullptr, double unit = 1.0);
bool prof_detail();
bool split_on();
bool amax_fused_on();
int wgrad_planes();

// resident workgroups per CU: LDS (160 KB) and registers -- the kernels use ~104 VGPRs: 4 waves per SIMD (16 per CU) for
// the 8-wave tiles, and 3 per SIMD are kept for the 4-wave tiles (3 x 48 KB of LDS)
template <int WGM, int WGN>
constexpr int dma_wg_per_cu() {
  using T = DmaTile<WGM, WGN>;
  return T::NW >= 8 ? std::min(160 * 1024 / T::SMEM, 16 / T::NW) : std::min(160 * 1024 / T::SMEM, 12 / T::NW);
}
template <int WGM, int WGN>
inline DmaSched plan_fwd_dma(const GemmP& p, int nb, size_t ws_bytes, double* cost) {
  using T = DmaTile<WGM, WGN>;
  const int ntiles = ceil_div(p.M, T::BM) * ceil_div(p.Npad, T::BN);
  constexpr int wg = dma_wg_per_cu<WGM, WGN>();
  return plan_dma(ntiles * nb, ntiles, p.K / T::BK, 256 * wg, (size_t)T::BM * T::BN * 4, ws_bytes, cost, wg * T::NW / 12.0);
}
// schedule of a pre-cut ring launch: nb batch elements / phases of `ntiles` tiles of T, WGCU workgroups per CU
template <class T, int WGCU>
inline DmaSched plan_pc(int ntiles, int nb, int K, size_t ws_cap) {
  return plan_dma(ntiles * nb, ntiles, K / T::BK, 256 * WGCU, (size_t)T::BM * T::BN * 4, ws_cap, nullptr, WGCU * T::NW / 12.0);
}
// the 128 x 128 pre-cut configuration: two LDS stages, four workgroups per CU (3- and 4-stage rings measured the same within
// 0.4 %: rounds 3 / 4).  Named because conv_fwd_stat_chunk plans the launch that launch_fwd_pc will make.
constexpr int PC128_WGM = 4, PC128_NB = 4, PC128_NSTG = 2, PC128_WGCU = 4;

// ---- conv_direct.hip: tiles are BM x BN of the output (forward-type) / k-rows x columns (weight gradient)
enum FwdTile { FWD_128x192, FWD_256x128, FWD_128x128, FWD_128x64, FWD_128x32 };
enum WgradTile { WGRAD_256x128, WGRAD_128x128, WGRAD_128x64, WGRAD_128x32, WGRAD_256x4, WGRAD_256x8 };
void launch_fwd_direct(Stream& s, GemmP& p, FwdTile tile, bool fast, int batch);
void launch_fwd_narrow(Stream& s, GemmP& p, int ng, bool fast, int batch);        // ng column groups of 4: 1, 2, 4, 5, 6, 8
void launch_wgrad_direct(Stream& s, GemmP& p, WgradTile tile, int batch);
// out[b] = the sum of the `splits` slabs of n floats, fixed order
void slab_sum(Stream& s, const float* slab, float* out, size_t n, int splits, int batch, size_t slab_bs, size_t out_bs);

// ---- conv_ring.hip
enum RingTile { RING_128x128, RING_128x256, RING_256x64 };
void launch_fwd_dma(Stream& s, GemmP& p, RingTile tile, int nb);
// bn: the column tile the operand was cut for (64, 128, 192); planes: 1 or 2
void launch_fwd_pc(Stream& s, GemmP& p, int bn, int planes, int nb, const unsigned short* wpc, size_t wpc_bs, bool phases,
                   const float* x_amax, const int* x_pair_k);
// the last 2 KiB of a stream's scratch hold the partial maxima of the launch in flight (A operand) and of the operand a producer
// is cutting; the split-K slabs of the same launch stay below
constexpr size_t PC_WS_TAIL = 2048;
float* ws_amax(Stream& s, int which);
void amax_partials(Stream& s, const float* x, size_t rows, int C, size_t rs, int batch, size_t bs, float* out, int fold = 0,
                   float floor = 0.f);

// (RING_128x128: 128 k-rows x 128 columns, RING_256x64)
void launch_wgrad_dma(Stream& s, GemmP& p, RingTile tile, int nb, const ConvWgradArgs& a);

// ---- conv_tail.hip
void launch_tail_fwd4(Stream& s, GemmP& p);
void launch_tail_wgrad4(Stream& s, GemmP& p);
void launch_fwd_phase4(Stream& s, GemmP& p, int ng);                              // ng: 1, 2, 4, 5

}  // namespace swn
