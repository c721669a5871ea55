// swapnet_amd -- SSIM and Charbonnier losses of modules.losses, fused with their gradients (ops.h ssim_loss / charbonnier_loss; the
// per-pixel arithmetic is ssim_math.h, shared with the host form in engine.cpp).
// Reference: modules/losses/__init__.py:14-27 (L1_Charbonnier_loss), :30-35 (gaussian), :128-259 (SSIM).
//
// SSIM forward: a 256-thread workgroup owns a 32 x 32 tile of one (b, c) plane.  It stages the tile plus a halo of P = window / 2
// pixels of x and y in LDS (zeros outside the image), runs the row pass of the five filters into LDS ((32 + 2P) rows x 32 columns
// each), then the column pass with four output rows per thread, forms S and the loss in registers, and leaves one fp64 partial.
// When a gradient is wanted it also writes the four coefficient maps (ssim_math.h) to the workspace; the backward launch stages
// those the same way, filters them separably and combines them with x and y.
#include "hip_util.h"

namespace swn {
namespace {

constexpr int T = SSIM_TILE;

// sum over a 256-thread block in a fixed order; result valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0;
  if (threadIdx.x == 0) r = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return r;
}

struct Tile { int plane, y0, x0; };
__device__ __forceinline__ Tile tile_of_block(int tiles_x, int tiles) {
  Tile t;
  t.plane = blockIdx.x / tiles;
  const int k = blockIdx.x - t.plane * tiles;
  t.y0 = (k / tiles_x) * T; t.x0 = (k % tiles_x) * T;
  return t;
}

template <int WS, bool COEF>
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int tiles_x,
                                                       int tiles, SsimWindow win, float C1, float C2, float* __restrict__ loss_map,
                                                       const float* __restrict__ gmap, float gscalar, float* __restrict__ coef,
                                                       size_t numel, double* __restrict__ partial) {
  constexpr int P = WS / 2, IN = T + 2 * P;
  __shared__ float sx[IN * IN], sy[IN * IN];      // tile + halo of both images
  __shared__ float r[5][IN * T];                   // row-filtered m1, m2, e11, e22, e12
  __shared__ double sh[4];
  const int tid = threadIdx.x;
  const Tile t = tile_of_block(tiles_x, tiles);
  const size_t base = (size_t)t.plane * H * W;
  for (int i = tid; i < IN * IN; i += 256) {
    const int ry = i / IN, rx = i - ry * IN;
    const int gy = t.y0 + ry - P, gx = t.x0 + rx - P;
    float a = 0.f, b = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const size_t o = base + (size_t)gy * W + gx;
      a = x[o]; b = y[o];
    }
    sx[i] = a; sy[i] = b;
  }
  __syncthreads();
  for (int i = tid; i < IN * T; i += 256) {
    const int ry = i / T, cx = i - ry * T;
    SsimMoments m = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < WS; ++k) ssim_tap(m, win.w[k], sx[ry * IN + cx + k], sy[ry * IN + cx + k]);
    r[0][i] = m.m1; r[1][i] = m.m2; r[2][i] = m.e11; r[3][i] = m.e22; r[4][i] = m.e12;
  }
  __syncthreads();
  const int cx = tid & (T - 1), ry0 = (tid / T) * 4;
  const int gx = t.x0 + cx;
  double acc = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int oy = ry0 + j, gy = t.y0 + oy;
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < WS; ++k)
#pragma unroll
      for (int q = 0; q < 5; ++q) v[q] += win.w[k] * r[q][(oy + k) * T + cx];
    if (gy < H && gx < W) {
      const size_t o = base + (size_t)gy * W + gx;
      const SsimMoments m = {v[0], v[1], v[2], v[3], v[4]};
      const SsimTerms st = ssim_terms(m, C1, C2);
      const float l = ssim_loss_of(st.S);
      acc += (double)l;
      if (loss_map) loss_map[o] = l;
      if (COEF) {
        const SsimCoefs c = ssim_coefs(m, st, gmap ? gmap[o] : gscalar);
        coef[o] = c.a1; coef[numel + o] = c.a2; coef[2 * numel + o] = c.b; coef[3 * numel + o] = c.c;
      }
    }
  }
  const double s = block_sum(acc, sh);
  if (tid == 0) partial[blockIdx.x] = s;
}

template <int WS>
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ coef,
                                                       size_t numel, int H, int W, int tiles_x, int tiles, SsimWindow win,
                                                       float* __restrict__ d1, float* __restrict__ d2) {
  constexpr int P = WS / 2, IN = T + 2 * P;
  __shared__ float sc[4][IN * IN];                 // tile + halo of a1, a2, b, c (zero outside the image: no output lives there)
  __shared__ float r[4][IN * T];
  const int tid = threadIdx.x;
  const Tile t = tile_of_block(tiles_x, tiles);
  const size_t base = (size_t)t.plane * H * W;
  for (int i = tid; i < IN * IN; i += 256) {
    const int ry = i / IN, rx = i - ry * IN;
    const int gy = t.y0 + ry - P, gx = t.x0 + rx - P;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const size_t o = base + (size_t)(in ? gy : 0) * W + (in ? gx : 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) sc[q][i] = in ? coef[q * numel + o] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < IN * T; i += 256) {
    const int ry = i / T, cx = i - ry * T;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < WS; ++k)
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += win.w[k] * sc[q][ry * IN + cx + k];
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q][i] = v[q];
  }
  __syncthreads();
  const int cx = tid & (T - 1), ry0 = (tid / T) * 4;
  const int gx = t.x0 + cx;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int oy = ry0 + j, gy = t.y0 + oy;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < WS; ++k)
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += win.w[k] * r[q][(oy + k) * T + cx];
    if (gy < H && gx < W) {
      const size_t o = base + (size_t)gy * W + gx;
      const float xv = x[o], yv = y[o];
      if (d1) d1[o] = v[0] + 2.f * xv * v[2] + yv * v[3];
      if (d2) d2[o] = v[1] + 2.f * yv * v[2] + xv * v[3];
    }
  }
}

__global__ __launch_bounds__(256) void charbonnier_kernel(const float* __restrict__ x, const float* __restrict__ y, size_t n, float eps,
                                                          float g, float* __restrict__ dx, float* __restrict__ dy,
                                                          double* __restrict__ partial) {
  __shared__ double sh[4];
  double acc = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float gr;
    acc += (double)charbonnier_term(x[i], y[i], eps, g, &gr);
    if (dx) dx[i] = gr;
    if (dy) dy[i] = -gr;
  }
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

struct SsimPlan {
  int tiles_x = 0, tiles = 0, blocks = 0;
  size_t numel = 0;
  double* partial = nullptr; float* coef = nullptr;
};

template <int WS>
void ssim_launch(Stream& s, const SsimArgs& a, const SsimPlan& p) {
  const SsimWindow win = ssim_window(WS);
  const float C1 = ssim_c1(a.max_val), C2 = ssim_c2(a.max_val);
  const bool grad = a.d1 || a.d2;
  if (grad)
    hipLaunchKernelGGL((ssim_fwd_kernel<WS, true>), dim3(p.blocks), dim3(256), 0, hs(s), a.img1, a.img2, a.H, a.W, p.tiles_x, p.tiles, win, C1,
                       C2, a.loss_map, a.gmap, a.gscalar, p.coef, p.numel, p.partial);
  else
    hipLaunchKernelGGL((ssim_fwd_kernel<WS, false>), dim3(p.blocks), dim3(256), 0, hs(s), a.img1, a.img2, a.H, a.W, p.tiles_x, p.tiles, win, C1,
                       C2, a.loss_map, (const float*)nullptr, 0.f, (float*)nullptr, p.numel, p.partial);
  finalize_sum(s, p.partial, p.blocks, 1.0, a.loss_sum);
  if (grad)
    hipLaunchKernelGGL((ssim_bwd_kernel<WS>), dim3(p.blocks), dim3(256), 0, hs(s), a.img1, a.img2, p.coef, p.numel, a.H, a.W, p.tiles_x, p.tiles,
                       win, a.d1, a.d2);
}

}  // namespace

void ssim_loss(Stream& s, const SsimArgs& a) {
  ssim_check(a);
  SsimPlan p;
  p.tiles_x = ceil_div(a.W, T);
  p.tiles = p.tiles_x * ceil_div(a.H, T);
  p.blocks = p.tiles * a.B * a.C;
  p.numel = (size_t)a.B * a.C * a.H * a.W;
  const size_t off_coef = ((size_t)p.blocks * sizeof(double) + 255) / 256 * 256;
  const size_t need = off_coef + ((a.d1 || a.d2) ? 4 * p.numel * sizeof(float) : 0);
  if (need > s.ws_bytes)
    throw Error(1, "ssim: needs " + std::to_string(need) + " bytes of workspace (block partials and, for a gradient, four coefficient maps), the context has " +
                       std::to_string(s.ws_bytes));
  p.partial = reinterpret_cast<double*>(s.ws);
  p.coef = reinterpret_cast<float*>(s.ws + off_coef);
  switch (a.window) {
    case 1: ssim_launch<1>(s, a, p); break;
    case 3: ssim_launch<3>(s, a, p); break;
    case 5: ssim_launch<5>(s, a, p); break;
    case 7: ssim_launch<7>(s, a, p); break;
    case 9: ssim_launch<9>(s, a, p); break;
    case 11: ssim_launch<11>(s, a, p); break;
    case 13: ssim_launch<13>(s, a, p); break;
    case 15: ssim_launch<15>(s, a, p); break;
    default: throw Error(1, "ssim: window " + std::to_string(a.window) + " has no kernel");        // (ssim_check admits none)
  }
  check_launch("ssim_loss");
}

void charbonnier_loss(Stream& s, const CharbonnierArgs& a) {
  if (!a.x || !a.y || !a.loss_sum) throw Error(1, "charbonnier: NULL argument");
  if (a.n < 1) throw Error(1, "charbonnier: empty input");
  const int grid = (int)std::min<size_t>((a.n + 255) / 256, 1024);
  if ((size_t)grid * sizeof(double) > s.ws_bytes) throw Error(1, "charbonnier: workspace too small");
  double* partial = reinterpret_cast<double*>(s.ws);
  hipLaunchKernelGGL(charbonnier_kernel, dim3(grid), dim3(256), 0, hs(s), a.x, a.y, a.n, a.eps, a.gscalar, a.dx, a.dy, partial);
  finalize_sum(s, partial, grid, 1.0, a.loss_sum);
  check_launch("charbonnier_loss");
}

}  // namespace swn
