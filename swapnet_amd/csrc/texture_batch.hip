// swapnet_amd -- texture batch hand-over (ops.h texture_batch): every model slot of a texture step written by ONE launch from the
// compact batch -- uint8 HWC images, uint8 label maps, the raw ROI table, five scalars per sample -- bit-identical to the host
// chain of the reference's TextureDataset.__getitem__ (datasets/texture_dataset.py:87-160, datasets/data_utils.py:169-295).
//
// Work units: a crop pixel has 1 + Cq of them, Cq = round_up(C, 4) / 4.  Unit 0 reads the pixel's three bytes (and those of its
// mirror image) and stores the normalised target and input texels, one float4 each; unit 1 + q reads the pixel's label byte and
// stores channels [4q, 4q + 4) of the one-hot vector into every cloth destination.  Units are numbered pixel-major, so the lanes
// of a wave store the consecutive 16-byte groups of consecutive pixels: whole 64-byte segments wherever a destination's slice is
// that wide.  The source bytes are read with byte loads (rows of 3 * Ws bytes have no alignment to speak of); a pixel's label is
// read by its Cq neighbouring lanes from one address.  The B * R ROI rows are a second, short loop of the same grid.  The pass moves a
// few MB and is bound by its stores; nothing here needs LDS.
#include <algorithm>

#include "hip_util.h"

namespace swn {
namespace {

struct TBp {
  const uint8_t* img; const uint8_t* labels; const float* rois_raw; const float* sample; float* rois_out;
  float* in_tex; float* tgt_tex; float* cloth[3];
  int in_cs, tgt_cs, cloth_cs[3], ncloth;
  int B, H, W, Hs, Ws, Hl, Wl, R, C, Cq, x_min, y_min, clamp_rois;
  float mean[3], sd[3], lscale_y, lscale_x;
};

// torch's nearest rule (UpSample.h nearest_idx): min(int(floorf(dst * scale)), in - 1), scale = float(in) / out taken on the host
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
  return min((int)floorf(__fmul_rn((float)dst, scale)), in - 1);
}
// to_tensor (true divide by 255), Normalize (sub, then a true divide by std): three correctly rounded fp32 operations
__device__ __forceinline__ float4 texel(const uint8_t* px, const TBp& p) {
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)px[c], 255.f), p.mean[c]), p.sd[c]);
  return make_float4(v[0], v[1], v[2], 0.f);
}
// flip_rois_: (values - center) * -1 + center
__device__ __forceinline__ float mirror(float v, float c) { return __fadd_rn(-__fsub_rn(v, c), c); }
// crop_rois: clamp(v, lo, hi) - lo with torch.clamp's min(max(v, lo), hi)
__device__ __forceinline__ float crop1(float v, float lo, float hi) { return __fsub_rn(fminf(fmaxf(v, lo), hi), lo); }

__global__ __launch_bounds__(256) void texture_batch_kernel(const TBp p) {
  const int Q = 1 + p.Cq;
  const size_t nunit = (size_t)p.B * p.H * p.W * Q, nroi = (size_t)p.B * p.R;
  const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t i = first; i < nunit; i += stride) {
    const size_t pix = i / Q;
    const int u = (int)(i - pix * Q);
    const int x = (int)(pix % p.W); const size_t t = pix / p.W;
    const int y = (int)(t % p.H); const int b = (int)(t / p.H);
    const int sy = p.y_min + y, sx = p.x_min + x;        // position in the Hs x Ws source
    if (u == 0) {                                        // ---- the two texels
      const uint8_t* im = p.img + (size_t)b * p.Hs * p.Ws * 3;
      const float* sp = p.sample + (size_t)b * 5;
      const int fy = sp[0] != 0.f ? p.Hs - 1 - sy : sy, fx = sp[1] != 0.f ? p.Ws - 1 - sx : sx;
      *reinterpret_cast<float4*>(p.in_tex + pix * p.in_cs) = texel(im + ((size_t)fy * p.Ws + fx) * 3, p);
      if (p.tgt_tex) *reinterpret_cast<float4*>(p.tgt_tex + pix * p.tgt_cs) = texel(im + ((size_t)sy * p.Ws + sx) * 3, p);
    } else {                                             // ---- four one-hot channels, every destination
      const int ly = nearest_src(sy, p.lscale_y, p.Hl), lx = nearest_src(sx, p.lscale_x, p.Wl);
      const int l = p.labels[((size_t)b * p.Hl + ly) * p.Wl + lx];
      const int c0 = (u - 1) * 4;
      const int hot = (l != 0 && l < p.C) ? l - c0 : -1;       // label 0 -> the all-zero vector; pad channels stay zero
      const float4 v = make_float4(hot == 0 ? 1.f : 0.f, hot == 1 ? 1.f : 0.f, hot == 2 ? 1.f : 0.f, hot == 3 ? 1.f : 0.f);
      for (int k = 0; k < p.ncloth; ++k) *reinterpret_cast<float4*>(p.cloth[k] + pix * p.cloth_cs[k] + c0) = v;
    }
  }
  // ---- the ROI rows: the first B * R threads of the grid, one row each (a loop of its own: sharing the loop above, the compiler
  // merges the tail of this store with the target texel's and both leave as a 4-byte and a 12-byte store)
  for (size_t k = first; k < nroi; k += stride) {
    const int b = (int)(k / p.R);
    const float* sp = p.sample + (size_t)b * 5;
    const float* raw = p.rois_raw + k * 4;
    const float sc = sp[2];
    float x1 = rintf(__fmul_rn(raw[0], sc)), y1 = rintf(__fmul_rn(raw[1], sc));
    float x2 = rintf(__fmul_rn(raw[2], sc)), y2 = rintf(__fmul_rn(raw[3], sc));
    if (sp[0] != 0.f) { const float lo = mirror(y2, sp[3]), hi = mirror(y1, sp[3]); y1 = lo; y2 = hi; }   // vertical first
    if (sp[1] != 0.f) { const float lo = mirror(x2, sp[4]), hi = mirror(x1, sp[4]); x1 = lo; x2 = hi; }
    if (p.clamp_rois) {
      const float xl = (float)p.x_min, xh = (float)(p.x_min + p.W - 1), yl = (float)p.y_min, yh = (float)(p.y_min + p.H - 1);
      x1 = crop1(x1, xl, xh); x2 = crop1(x2, xl, xh); y1 = crop1(y1, yl, yh); y2 = crop1(y2, yl, yh);
    }
    *reinterpret_cast<float4*>(p.rois_out + k * 4) = make_float4(x1, y1, x2, y2);
  }
}

}  // namespace

void texture_batch(Stream& s, const TextureBatchArgs& a) {
  texture_batch_check(a);
  TBp p{};
  p.img = a.img; p.labels = a.labels; p.rois_raw = a.rois_raw; p.sample = a.sample; p.rois_out = a.rois_out;
  p.in_tex = a.in_tex.p; p.in_cs = a.in_tex.cs; p.tgt_tex = a.tgt_tex.p; p.tgt_cs = a.tgt_tex.cs;
  p.ncloth = a.ncloth;
  for (int k = 0; k < a.ncloth; ++k) { p.cloth[k] = a.cloth[k].p; p.cloth_cs[k] = a.cloth[k].cs; }
  p.B = a.in_tex.N; p.H = a.in_tex.H; p.W = a.in_tex.W; p.Hs = a.Hs; p.Ws = a.Ws; p.Hl = a.Hl; p.Wl = a.Wl; p.R = a.R;
  p.C = a.C; p.Cq = round_up(a.C, 4) / 4; p.x_min = a.x_min; p.y_min = a.y_min;
  p.clamp_rois = !(a.x_min == 0 && a.y_min == 0 && p.H == a.Hs && p.W == a.Ws);
  for (int c = 0; c < 3; ++c) { p.mean[c] = a.mean[c]; p.sd[c] = a.std[c]; }
  p.lscale_y = (float)a.Hl / (float)a.Hs; p.lscale_x = (float)a.Wl / (float)a.Ws;
  const size_t total = std::max((size_t)p.B * p.H * p.W * (1 + p.Cq), (size_t)p.B * p.R);
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(texture_batch_kernel, dim3(grid), dim3(256), 0, hs(s), p);
  check_launch("texture_batch");
}

}  // namespace swn
