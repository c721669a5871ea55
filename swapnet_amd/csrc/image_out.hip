// swapnet_amd -- saved-image visuals (ops.h image_u8): what inference.py does on the host between a model's tensors and
// Image.fromarray -- unnormalize / scale_tensor(scale_each) (datasets/data_utils.py:41-90), decode_cloth_labels (util/decode_labels.py:
// 24-55), draw_rois_on_texture (util/draw_rois.py:16-47), util.tensor2im (util/util.py:9-32) -- as one pass from an NHWC view (or a label
// map) to interleaved (B,H,W,3) bytes.  The arithmetic is spelled out in ops.h; engine.cpp holds the same expressions as plain loops.
//
// Shape: the pass moves 16 bytes in and 3 bytes out per pixel and is bound by that traffic.  A workgroup belongs to ONE image, so the
// image's affine row, its min / max and its ROI table are wave-uniform; a thread owns four consecutive pixels: one 16-byte load each
// on 4-channel views, twelve output bytes leaving as three dword stores wherever the image's byte offset allows (H * W a multiple of 4,
// or image 0), byte stores at an image's tail and otherwise.  scale_each adds one launch in front: image_u8_chunks(H, W) <= 64
// workgroups per image leave (min, max) partials, and every wave of the conversion kernel folds them again for itself (64 lanes, one
// partial each) -- no atomics, no second pass over the image, nothing the host reads.  The ROI table of the image is truncated to
// integers once per workgroup into LDS; the per-pixel test is then compares on broadcast reads.
#include <algorithm>

#include "hip_util.h"

namespace swn {
namespace {

__constant__ uint8_t kImagePalette[LABEL_PALETTE_SIZE][3] = {SWN_LABEL_PALETTE};

struct IOp {
  const float* x; const int32_t* labels; const float* rows; const float* minmax; const float* rois; const uint8_t* colours;
  uint8_t* out;
  int cs, C, H, W, HW, source, range, scale_each, vec, chunks, R, width, bpi;
};

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// (min, max) over the logical channels of pixels [chunk * per, (chunk + 1) * per) of image b -> part[b][chunk][2].  Every (b, chunk)
// is written on every call, an empty chunk with (+inf, -inf).
__global__ __launch_bounds__(256) void image_minmax_kernel(const float* __restrict__ x, int cs, int C, int HW, int chunks, int vec,
                                                           float* __restrict__ part) {
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const int per = (HW + chunks - 1) / chunks;
  const int p0 = chunk * per, p1 = min(HW, p0 + per);
  const float* img = x + (size_t)b * HW * cs;
  float lo = INFINITY, hi = -INFINITY;
  for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
    const float* px = img + (size_t)p * cs;
    if (vec) {
      const float4 v = *reinterpret_cast<const float4*>(px);
      lo = fminf(lo, v.x); hi = fmaxf(hi, v.x);
      if (C == 3) { lo = fminf(lo, fminf(v.y, v.z)); hi = fmaxf(hi, fmaxf(v.y, v.z)); }
    } else {
      for (int c = 0; c < C; ++c) { const float v = px[c]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
    }
  }
  __shared__ float red[4][2];
  lo = wave_min(lo); hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = lo; red[threadIdx.x >> 6][1] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { lo = fminf(lo, red[w][0]); hi = fmaxf(hi, red[w][1]); }
    part[((size_t)b * chunks + chunk) * 2] = lo;
    part[((size_t)b * chunks + chunk) * 2 + 1] = hi;
  }
}

// tensor2im's byte: one rounded fp32 operation per step, saturated, truncated
__device__ __forceinline__ unsigned to_byte(float u, int range) {
  const float t = range == RANGE_SIGNED ? __fmul_rn(__fdiv_rn(__fadd_rn(u, 1.f), 2.f), 255.f) : __fmul_rn(u, 255.f);
  return (unsigned)(int)fminf(fmaxf(t, 0.f), 255.f);
}

__global__ __launch_bounds__(256) void image_u8_kernel(const IOp p) {
  const int b = blockIdx.x / p.bpi, blk = blockIdx.x - b * p.bpi;       // one image per workgroup: everything per image is uniform
  __shared__ int roi[IMAGE_MAX_ROIS][8];                               // x0, y0, x1, y1, first / last row of the side columns, colour
  if ((int)threadIdx.x < p.R) {
    const float* r = p.rois + ((size_t)b * p.R + threadIdx.x) * 4;
    int v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (int)fminf(fmaxf(r[j], -536870912.f), 536870912.f);    // (int): toward zero, as Pillow's cast
    const int a = v[1] + p.width, e = v[3] - p.width + 1;
    const uint8_t* col = p.colours + threadIdx.x * 3;
    int* d = roi[threadIdx.x];
    d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    d[4] = a <= e ? a : e + 1; d[5] = a <= e ? e - 1 : a;
    d[6] = (int)((unsigned)col[0] | ((unsigned)col[1] << 8) | ((unsigned)col[2] << 16));
  }
  float lo = 0.f, hi = 0.f, den = 1.f;
  if (p.scale_each) {                                                  // every wave folds the image's partials for itself
    const int lane = threadIdx.x & 63;
    float l = INFINITY, h = -INFINITY;
    if (lane < p.chunks) { l = p.minmax[((size_t)b * p.chunks + lane) * 2]; h = p.minmax[((size_t)b * p.chunks + lane) * 2 + 1]; }
    lo = wave_min(l); hi = wave_max(h);
    den = (float)((double)hi - (double)lo + 1e-5);
  }
  float sc[3] = {1.f, 1.f, 1.f}, sh[3] = {0.f, 0.f, 0.f};
  bool clamp01 = false;
  if (p.rows) {
    const float* r = p.rows + (size_t)b * (2 * p.C + 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) { const int cc = p.C == 1 ? 0 : c; sc[c] = r[cc]; sh[c] = r[p.C + cc]; }
    clamp01 = r[2 * p.C] != 0.f;
  }
  __syncthreads();

  const int q0 = (blk * 256 + (int)threadIdx.x) * 4;                   // first of this thread's four pixels within the image
  if (q0 >= p.HW) return;
  const int npx = min(4, p.HW - q0);
  int y = q0 / p.W, x = q0 - y * p.W;
  unsigned rgb[4] = {0u, 0u, 0u, 0u};
  for (int j = 0; j < npx; ++j) {
    const size_t pix = (size_t)b * p.HW + q0 + j;
    unsigned c3;
    if (p.source == SRC_FLOAT) {
      const float* px = p.x + pix * p.cs;
      float v[3];
      if (p.vec) { const float4 t = *reinterpret_cast<const float4*>(px); v[0] = t.x; v[1] = t.y; v[2] = t.z; }
      else { v[0] = px[0]; if (p.C == 3) { v[1] = px[1]; v[2] = px[2]; } }
      if (p.C == 1) v[1] = v[2] = v[0];
      c3 = 0u;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float u = v[c];
        if (p.rows) {
          u = __fadd_rn(__fmul_rn(u, sc[c]), sh[c]);
          if (clamp01) u = fminf(fmaxf(u, 0.f), 1.f);
        } else if (p.scale_each) {
          u = __fdiv_rn(__fadd_rn(fminf(fmaxf(u, lo), hi), -lo), den);
        }
        c3 |= to_byte(u, p.range) << (8 * c);
      }
    } else {
      int best;
      if (p.source == SRC_LABELS) {
        best = p.labels[pix];
      } else {
        const float* px = p.x + pix * p.cs;
        best = 0;
        float m = px[0];
        if (p.vec) {                                                   // whole 16-byte groups; channels at or above C are read and ignored
          for (int c0 = 0; c0 < p.C; c0 += 4) {
            const float4 t = *reinterpret_cast<const float4*>(px + c0);
            const float g[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (c0 + k < p.C && g[k] > m) { m = g[k]; best = c0 + k; }          // strict: the first maximum wins, as argmax
          }
        } else {
          for (int c = 1; c < p.C; ++c) { const float v = px[c]; if (v > m) { m = v; best = c; } }
        }
      }
      c3 = 0u;
      if (best >= 0 && best < LABEL_PALETTE_SIZE)
        c3 = (unsigned)kImagePalette[best][0] | ((unsigned)kImagePalette[best][1] << 8) | ((unsigned)kImagePalette[best][2] << 16);
    }
    for (int r = 0; r < p.R; ++r) {                                    // ascending, overwriting: the last outline that covers wins
      const int* d = roi[r];
      const int x0 = d[0], y0 = d[1], x1 = d[2], y1 = d[3], w = p.width;
      const bool rows_hit = x >= x0 && x <= x1 && ((y >= y0 && y <= y0 + w - 1) || (y >= y1 - w + 1 && y <= y1));
      const bool cols_hit = ((x >= x0 && x <= x0 + w - 1) || (x >= x1 - w + 1 && x <= x1)) && y >= d[4] && y <= d[5];
      if (rows_hit || cols_hit) c3 = (unsigned)d[6];
    }
    rgb[j] = c3;
    if (++x == p.W) { x = 0; ++y; }
  }
  uint8_t* dst = p.out + ((size_t)b * p.HW + q0) * 3;
  if (npx == 4 && ((uintptr_t)dst & 3) == 0) {                         // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
    d32[0] = rgb[0] | (rgb[1] << 24);
    d32[1] = (rgb[1] >> 8) | (rgb[2] << 16);
    d32[2] = (rgb[2] >> 16) | (rgb[3] << 8);
  } else {
    for (int j = 0; j < npx; ++j) {
      dst[3 * j] = (uint8_t)rgb[j]; dst[3 * j + 1] = (uint8_t)(rgb[j] >> 8); dst[3 * j + 2] = (uint8_t)(rgb[j] >> 16);
    }
  }
}

}  // namespace

void image_u8(Stream& s, const ImageU8Args& args) {
  const ImageU8Args a = image_u8_check(args);
  IOp p{};
  p.x = a.x.p; p.cs = a.x.cs; p.C = a.C; p.labels = a.labels; p.rows = a.rows; p.minmax = a.minmax; p.rois = a.rois; p.colours = a.colours;
  p.out = a.out; p.H = a.H; p.W = a.W; p.HW = a.H * a.W; p.source = a.source; p.range = a.range; p.scale_each = a.scale_each;
  p.R = a.R; p.width = a.width;
  // 16-byte loads where every pixel row of the view starts on a 16-byte boundary (what the models' views do); a float source then
  // reads one group, an argmax source ceil(C / 4) of them, which the pixel stride has to cover
  p.vec = a.source != SRC_LABELS && a.x.cs % 4 == 0 && !((uintptr_t)a.x.p & 15) && round_up(a.C, 4) <= a.x.cs;
  p.chunks = image_u8_chunks(a.H, a.W);
  p.bpi = (p.HW + 1023) / 1024;
  if ((size_t)a.B * p.bpi > 0x7fffffffull || (size_t)a.B * p.chunks > 0x7fffffffull) throw Error(1, "image_u8: batch too large for one launch");
  if (a.scale_each) {
    hipLaunchKernelGGL(image_minmax_kernel, dim3((unsigned)(a.B * p.chunks)), dim3(256), 0, hs(s), a.x.p, a.x.cs, a.C, p.HW, p.chunks,
                       p.vec, a.minmax);
    check_launch("image_u8 (min/max)");
  }
  hipLaunchKernelGGL(image_u8_kernel, dim3((unsigned)(a.B * p.bpi)), dim3(256), 0, hs(s), p);
  check_launch("image_u8");
}

}  // namespace swn
