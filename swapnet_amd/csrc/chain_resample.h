// swapnet_amd -- device side of ops.h chain_resample: one chain of {kind, c0..c7} rows evaluated at one output pixel, kinds 0 to 2 with
// PIL's NEAREST rule as affine_gather_kernel walks them, kind 3 with Pillow's mode-"F" BICUBIC perspective.  Shared by gather.hip
// (chain_resample_kernel: the taps read a float image) and warp_batch.hip (the taps are the indicators in_labels == c).  The host
// form with the same expressions in the same order is chain_value_host in engine.cpp.
#pragma once
#include "hip_util.h"

namespace swn {

// Pillow's FLOOR (Geometry.c): truncation for v >= 0, floor below
__device__ __forceinline__ int pil_floor(double v) { return v < 0.0 ? (int)floor(v) : (int)v; }

// the source position of a perspective row (kinds 2 and 3) for output pixel (x, y): affine_gather_kernel's expressions
__device__ __forceinline__ void perspective_src(const double* m, long long x, long long y, double& fx, double& fy) {
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  const double den = m[7] * xc + m[8] * yc + 1.0;
  fx = (m[1] * xc + m[2] * yc + m[3]) / den;
  fy = (m[4] * xc + m[5] * yc + m[6]) / den;
}

// one NEAREST step through row m, as in affine_gather_kernel; false where it leaves the W x H image.  (A kind-3 row met here -- a
// second one in a chain, which the callers rule out -- is resampled NEAREST like kind 2: nothing is read out of bounds.)
__device__ __forceinline__ bool nearest_step(const double* m, long long& x, long long& y, int W, int H) {
  const int kind = (int)m[0];
  long long xin = x, yin = y;
  if (kind == 1) {
    xin = ((long long)m[3] + (long long)m[2] * y + (long long)m[1] * x) >> 16;
    yin = ((long long)m[6] + (long long)m[5] * y + (long long)m[4] * x) >> 16;
  } else if (kind == 2 || kind == 3) {
    double fx, fy;
    perspective_src(m, x, y, fx, fy);
    xin = fx < 0.0 ? -1 : (long long)(int)fx;
    yin = fy < 0.0 ? -1 : (long long)(int)fy;
  }
  x = xin; y = yin;
  return xin >= 0 && xin < W && yin >= 0 && yin < H;
}

// Pillow's BICUBIC macro (Geometry.c).  Along a row of a mode-"F" image its arguments are the FLOAT32 texels themselves, so p2, p3 and
// p4 are float expressions, each operation rounded to fp32, and only the Horner form in d runs in double ...
__device__ __forceinline__ double cubic_taps(float v1, float v2, float v3, float v4, double d) {
  const double p1 = (double)v2;
  const double p2 = (double)__fadd_rn(-v1, v3);
  const double p3 = (double)__fsub_rn(__fadd_rn(__fmul_rn(2.f, __fsub_rn(v1, v2)), v3), v4);
  const double p4 = (double)__fadd_rn(__fsub_rn(__fadd_rn(-v1, v2), v3), v4);
  return __dadd_rn(p1, __dmul_rn(d, __dadd_rn(p2, __dmul_rn(d, __dadd_rn(p3, __dmul_rn(d, p4))))));
}
// ... and down the four row values, which are doubles, all of it does
__device__ __forceinline__ double cubic_rows(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = __dadd_rn(-v1, v3);
  const double p3 = __dsub_rn(__dadd_rn(__dmul_rn(2.0, __dsub_rn(v1, v2)), v3), v4);
  const double p4 = __dadd_rn(__dsub_rn(__dadd_rn(-v1, v2), v3), v4);
  return __dadd_rn(p1, __dmul_rn(d, __dadd_rn(p2, __dmul_rn(d, __dadd_rn(p3, __dmul_rn(d, p4))))));
}

// The chain `rows` (nmaps rows of 9 doubles) at output pixel (x0, y0) of a W x H image whose value at flat index y * W + x is src(index).
// Rows behind the kind-3 row are walked first from the output pixel; at the kind-3 row the 4 x 4 window is placed by Pillow's rule
// (ops.h chain_resample) and ALL sixteen tap positions go through the rows in front of it together, row by row -- a row's nine
// doubles are loaded and converted once for the sixteen, and a lane's branch on the row's kind is taken once per row, not per tap.  A
// tap that leaves the image on the way reads 0.  Everything is unrolled: positions, the inside mask and the texels stay in registers.
template <class Src>
__device__ __forceinline__ float chain_value(const double* rows, int nmaps, int x0, int y0, int W, int H, Src src) {
  long long x = x0, y = y0;
  int k = nmaps - 1;
  for (; k >= 0; --k) {
    const double* m = rows + (size_t)k * 9;
    if ((int)m[0] == 3) break;
    if (!nearest_step(m, x, y, W, H)) return 0.f;
  }
  if (k < 0) return src((int)y * W + (int)x);
  double fx, fy;
  perspective_src(rows + (size_t)k * 9, x, y, fx, fy);
  const int ix = pil_floor(fx), iy = pil_floor(fy);
  if (ix < 0 || ix >= W || iy < 0 || iy >= H) return 0.f;                       // Pillow's fill
  fx = __dsub_rn(fx, 0.5); fy = __dsub_rn(fy, 0.5);
  const int wx = pil_floor(fx), wy = pil_floor(fy);
  const double dx = __dsub_rn(fx, (double)wx), dy = __dsub_rn(fy, (double)wy);
  int tx[16], ty[16];
  unsigned live = 0;                                    // bit 4 j: window row j is evaluated (row 0 always, clipped)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yy = wy - 1 + j;
    if (j == 0 || (yy >= 0 && yy < H)) live |= 1u << (4 * j);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      tx[4 * j + i] = min(max(wx - 1 + i, 0), W - 1);
      ty[4 * j + i] = min(max(yy, 0), H - 1);           // (rows 1 to 3 outside the image are not evaluated; their taps stay in bounds)
    }
  }
  unsigned in = 0xffffu;                                // bit t: tap t is still inside the image
  for (int r = k - 1; r >= 0; --r) {
    const double* m = rows + (size_t)r * 9;
    const int kind = (int)m[0];
    if (kind == 1) {
      const long long a0 = (long long)m[1], a1 = (long long)m[2], a2 = (long long)m[3];
      const long long a3 = (long long)m[4], a4 = (long long)m[5], a5 = (long long)m[6];
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const long long px = tx[t], py = ty[t];
        const long long xin = (a2 + a1 * py + a0 * px) >> 16, yin = (a5 + a4 * py + a3 * px) >> 16;
        const bool ok = xin >= 0 && xin < W && yin >= 0 && yin < H;
        if (!ok) in &= ~(1u << t);
        tx[t] = ok ? (int)xin : 0; ty[t] = ok ? (int)yin : 0;
      }
    } else if (kind == 2 || kind == 3) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        double gx, gy;
        perspective_src(m, tx[t], ty[t], gx, gy);
        const long long xin = gx < 0.0 ? -1 : (long long)(int)gx, yin = gy < 0.0 ? -1 : (long long)(int)gy;
        const bool ok = xin >= 0 && xin < W && yin >= 0 && yin < H;
        if (!ok) in &= ~(1u << t);
        tx[t] = ok ? (int)xin : 0; ty[t] = ok ? (int)yin : 0;
      }
    }
  }
  double rv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = 4 * j + i;
      v[i] = (in >> t & 1u) ? src(ty[t] * W + tx[t]) : 0.f;
    }
    const double c = cubic_taps(v[0], v[1], v[2], v[3], dx);
    rv[j] = (j == 0 || (live >> (4 * j) & 1u)) ? c : rv[j > 0 ? j - 1 : 0];
  }
  return (float)cubic_rows(rv[0], rv[1], rv[2], rv[3], dy);
}

}  // namespace swn
