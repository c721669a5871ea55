// swapnet_amd -- warp batch hand-over (ops.h warp_batch): every buffer a warp step reads from outside, written by ONE launch from the
// compact batch -- the decoded uint8 HWC body image, the uint8 input and target label maps, the per-channel map table of
// affine_gather -- bit-identical to the host chain of the reference's WarpDataset.__getitem__ (datasets/warp_dataset.py:139-183)
// with the augmentation of gpu_augment in it.
//
// Work units: a crop pixel has 1 + 2 Cq of them, Cq = round_up(C, 4) / 4.  Unit 0 reads the 2 x 2 bytes around the pixel's source
// position per colour and stores the bilinear sample of their normalised texels, one float4 into every body destination; unit
// 1 + q reads the pixel's target label and stores channels [4q, 4q + 4) of its one-hot vector; unit 1 + Cq + q walks the chains of
// the input cloth's channels [4q, 4q + 4) backwards through the map table and stores whether each ends on its own label.  Units
// are numbered pixel-major, so the lanes of a wave store the consecutive 16-byte groups of a pixel's cloth vectors.  The source
// bytes are read with byte loads; the 72-byte map rows of one (sample, channel) are read by every lane of that channel from the
// same addresses and stay in the vector cache (not staged in LDS: a block's lanes span all channels of ~23 pixels, so a stage
// would hold B-dependent rows of every channel for a pass that is bound by its stores).  The 19-channel float one-hot map of the
// host chain never exists.
#include <algorithm>

#include "chain_resample.h"
#include "hip_util.h"

namespace swn {
namespace {

struct WBp {
  const uint8_t* body; const uint8_t* in_labels; const uint8_t* tgt_labels; const double* maps;
  float* in_cloth; float* tgt_cloth; float* body_out[3];
  int in_cs, tgt_cs, body_cs[3], nbody;
  int B, H, W, Hb, Wb, Hl, Wl, C, Cq, nmaps, x_min, y_min;
  float mean[3], sd[3], lscale_y, lscale_x, bscale_y, bscale_x;
};

// torch's nearest rule (UpSample.h nearest_idx): min(int(floorf(dst * scale)), in - 1), scale = float(in) / out taken on the host
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
  return min((int)floorf(__fmul_rn((float)dst, scale)), in - 1);
}
// to_tensor (true divide by 255), Normalize (sub, then a true divide by std): three correctly rounded fp32 operations
__device__ __forceinline__ float texel(const uint8_t* px, int c, const WBp& p) {
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)px[c], 255.f), p.mean[c]), p.sd[c]);
}
// torch's bilinear source position (UpSample.h area_pixel_compute_source_index, align_corners False): the two taps and their weights
__device__ __forceinline__ void bilinear_src(int dst, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
  const float src = fmaxf(__fsub_rn(__fmul_rn(scale, (float)dst + 0.5f), 0.5f), 0.f);
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = __fsub_rn(src, (float)i0);
  l0 = __fsub_rn(1.f, l1);
}
// the chain of (sample, channel) bc walked backwards from (x, y) of the Hl x Wl map, as affine_gather_kernel (gather.hip) walks it:
// the source pixel's index in the map, or -1 where the walk leaves it
__device__ __forceinline__ int walk(const WBp& p, int bc, int x0, int y0) {
  long long x = x0, y = y0;
  for (int k = p.nmaps - 1; k >= 0; --k) {
    const double* m = p.maps + ((size_t)bc * p.nmaps + k) * 9;
    const int kind = (int)m[0];
    long long xin = x, yin = y;
    if (kind == 1) {
      xin = ((long long)m[3] + (long long)m[2] * y + (long long)m[1] * x) >> 16;
      yin = ((long long)m[6] + (long long)m[5] * y + (long long)m[4] * x) >> 16;
    } else if (kind == 2) {
      const double xc = (double)x + 0.5, yc = (double)y + 0.5;
      const double den = m[7] * xc + m[8] * yc + 1.0;
      const double fx = (m[1] * xc + m[2] * yc + m[3]) / den, fy = (m[4] * xc + m[5] * yc + m[6]) / den;
      xin = fx < 0.0 ? -1 : (long long)(int)fx;
      yin = fy < 0.0 ? -1 : (long long)(int)fy;
    }
    if (!(xin >= 0 && xin < p.Wl && yin >= 0 && yin < p.Hl)) return -1;
    x = xin; y = yin;
  }
  return (int)y * p.Wl + (int)x;
}

// BICUBIC = false: the table holds kinds 0 to 2, the work units above.  BICUBIC = true (WarpBatchArgs::bicubic): it may hold kind 3,
// and an input-cloth value is then a chain evaluated by chain_resample.h -- up to 16 taps through up to nmaps - 1 rows and two cubics in
// double, against one walk.  The four channels of a cloth unit would run that one after the other on one lane, while the body and
// target lanes of the wave wait and the chains of the wave's channels differ in kind.  So that instantiation splits the index space
// in two: first the 1 + Cq body and target units of every pixel, as above, padded to a whole number of blocks; then ONE LANE PER
// (pixel, channel), four consecutive lanes a 16-byte group.  A lane evaluates its channel's whole chain by itself -- the order of
// rounded operations per output is the rule's -- the four values of a group meet in its first lane through ds_bpermute (__shfl, width
// 4), and that lane stores the float4.  Both ranges start on a multiple of 256 and the grid stride is one, so a group never
// straddles a wave and its four lanes leave the loop together.  (The second launch bound holds <true> to four waves per SIMD: 123 VGPRs
// where the allocator would take 129; <false> keeps the allocation it always had, 56.)
template <bool BICUBIC>
__global__ __launch_bounds__(256, BICUBIC ? 4 : 1) void warp_batch_kernel(const WBp p) {
  const int Q = BICUBIC ? 1 + p.Cq : 1 + 2 * p.Cq;
  const size_t npix = (size_t)p.B * p.H * p.W;
  const size_t nlight = npix * Q, nlight_pad = BICUBIC ? (nlight + 255) / 256 * 256 : nlight;
  const size_t nunit = BICUBIC ? nlight_pad + npix * 4 * p.Cq : nlight, stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nunit; i += stride) {
    if constexpr (BICUBIC) {
      if (i >= nlight_pad) {                             // ---- one channel of the augmented input cloth
        const size_t e = i - nlight_pad;
        const int Cp = 4 * p.Cq;
        const size_t pix = e / Cp;
        const int c = (int)(e - pix * Cp);
        const int x = (int)(pix % p.W); const size_t t = pix / p.W;
        const int y = (int)(t % p.H); const int b = (int)(t / p.H);
        const int ly = nearest_src(p.y_min + y, p.lscale_y, p.Hl), lx = nearest_src(p.x_min + x, p.lscale_x, p.Wl);
        const uint8_t* lab = p.in_labels + (size_t)b * p.Hl * p.Wl;
        float v = 0.f;
        if (c != 0 && c < p.C) {
          auto hot = [&](int idx) { return lab[idx] == c ? 1.f : 0.f; };
          v = p.nmaps ? chain_value(p.maps + (size_t)(b * p.C + c) * p.nmaps * 9, p.nmaps, lx, ly, p.Wl, p.Hl, hot) : hot(ly * p.Wl + lx);
        }
        const float v1 = __shfl(v, 1, 4), v2 = __shfl(v, 2, 4), v3 = __shfl(v, 3, 4);
        if ((c & 3) == 0) *reinterpret_cast<float4*>(p.in_cloth + pix * p.in_cs + c) = make_float4(v, v1, v2, v3);
        continue;
      }
      if (i >= nlight) continue;                         // (the pad between the two ranges)
    }
    const size_t pix = i / Q;
    const int u = (int)(i - pix * Q);
    const int x = (int)(pix % p.W); const size_t t = pix / p.W;
    const int y = (int)(t % p.H); const int b = (int)(t / p.H);
    const int sy = p.y_min + y, sx = p.x_min + x;        // position in the Ls x Ls resized sample
    if (u == 0) {                                        // ---- the body texel
      int y0, y1, x0, x1; float h0, h1, w0, w1;
      bilinear_src(sy, p.bscale_y, p.Hb, y0, y1, h0, h1);
      bilinear_src(sx, p.bscale_x, p.Wb, x0, x1, w0, w1);
      const uint8_t* im = p.body + (size_t)b * p.Hb * p.Wb * 3;
      const uint8_t* pa = im + ((size_t)y0 * p.Wb + x0) * 3; const uint8_t* pb = im + ((size_t)y0 * p.Wb + x1) * 3;
      const uint8_t* pc = im + ((size_t)y1 * p.Wb + x0) * 3; const uint8_t* pd = im + ((size_t)y1 * p.Wb + x1) * 3;
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = __fadd_rn(__fmul_rn(w0, texel(pa, c, p)), __fmul_rn(w1, texel(pb, c, p)));
        const float bot = __fadd_rn(__fmul_rn(w0, texel(pc, c, p)), __fmul_rn(w1, texel(pd, c, p)));
        v[c] = __fadd_rn(__fmul_rn(h0, top), __fmul_rn(h1, bot));
      }
      const float4 o = make_float4(v[0], v[1], v[2], 0.f);
      for (int k = 0; k < p.nbody; ++k) *reinterpret_cast<float4*>(p.body_out[k] + pix * p.body_cs[k]) = o;
      continue;
    }
    const int ly = nearest_src(sy, p.lscale_y, p.Hl), lx = nearest_src(sx, p.lscale_x, p.Wl);
    const size_t lb = (size_t)b * p.Hl * p.Wl;
    if (u <= p.Cq) {                                     // ---- four channels of the target's one-hot vector
      if (!p.tgt_cloth) continue;
      const int l = p.tgt_labels[lb + (size_t)ly * p.Wl + lx];
      const int c0 = (u - 1) * 4;
      const int hot = (l != 0 && l < p.C) ? l - c0 : -1;       // label 0 -> the all-zero vector; pad channels stay zero
      *reinterpret_cast<float4*>(p.tgt_cloth + pix * p.tgt_cs + c0) =
          make_float4(hot == 0 ? 1.f : 0.f, hot == 1 ? 1.f : 0.f, hot == 2 ? 1.f : 0.f, hot == 3 ? 1.f : 0.f);
    } else if constexpr (!BICUBIC) {                     // ---- four channels of the augmented input cloth
      const int c0 = (u - 1 - p.Cq) * 4;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + j;
        v[j] = 0.f;
        if (c == 0 || c >= p.C) continue;                // channel 0 of the one-hot map is all zero, and so is every image of it
        const int src = walk(p, b * p.C + c, lx, ly);
        if (src >= 0 && p.in_labels[lb + src] == c) v[j] = 1.f;
      }
      *reinterpret_cast<float4*>(p.in_cloth + pix * p.in_cs + c0) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

}  // namespace

void warp_batch(Stream& s, const WarpBatchArgs& a) {
  warp_batch_check(a);
  WBp p{};
  p.body = a.body; p.in_labels = a.in_labels; p.tgt_labels = a.tgt_labels; p.maps = a.maps; p.nmaps = a.maps ? a.nmaps : 0;
  p.in_cloth = a.in_cloth.p; p.in_cs = a.in_cloth.cs; p.tgt_cloth = a.tgt_cloth.p; p.tgt_cs = a.tgt_cloth.cs;
  p.nbody = a.nbody;
  for (int k = 0; k < a.nbody; ++k) { p.body_out[k] = a.body_out[k].p; p.body_cs[k] = a.body_out[k].cs; }
  p.B = a.in_cloth.N; p.H = a.in_cloth.H; p.W = a.in_cloth.W; p.Hb = a.Hb; p.Wb = a.Wb; p.Hl = a.Hl; p.Wl = a.Wl;
  p.C = a.C; p.Cq = round_up(a.C, 4) / 4; p.x_min = a.x_min; p.y_min = a.y_min;
  for (int c = 0; c < 3; ++c) { p.mean[c] = a.mean[c]; p.sd[c] = a.std[c]; }
  p.lscale_y = (float)a.Hl / (float)a.Ls; p.lscale_x = (float)a.Wl / (float)a.Ls;
  p.bscale_y = (float)a.Hb / (float)a.Ls; p.bscale_x = (float)a.Wb / (float)a.Ls;
  const size_t npix = (size_t)p.B * p.H * p.W;
  if (a.bicubic) {                                        // (the kernel's two index ranges)
    const size_t total = (npix * (1 + p.Cq) + 255) / 256 * 256 + npix * 4 * p.Cq;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(warp_batch_kernel<true>, dim3(grid), dim3(256), 0, hs(s), p);
    check_launch("warp_batch (bicubic)");
    return;
  }
  const size_t total = npix * (1 + 2 * p.Cq);
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(warp_batch_kernel<false>, dim3(grid), dim3(256), 0, hs(s), p);
  check_launch("warp_batch");
}

}  // namespace swn
