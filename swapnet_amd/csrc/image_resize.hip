// swapnet_amd -- Pillow's bilinear resize of uint8 RGB images (ops.h resize_u8): Image.resize((Ws, Hs), Image.BILINEAR) of a batch of
// decoded images of different sizes in ONE launch, byte for byte (Pillow's Resample.c: 8-bit resample, double-precision windows
// normalised and rounded to 22 fractional bits, a horizontal pass that leaves rounded bytes, then a vertical pass on those).
//
// Lane mapping.  A workgroup of 256 threads owns a TH x TW = 8 x 32 pixel tile of one sample's output; the grid is (column tiles,
// row tiles, samples).  Four stages, a barrier between each:
//   1. coefficients: lanes 0..31 derive the windows {xmin, n, k[n]} of the tile's 32 columns, lanes 64..71 (another wave) those of
//      its 8 rows, in double, into LDS -- per workgroup, so nothing is uploaded, cached or allocated per geometry.  The window is
//      walked twice (once for the sum, once for the normalised taps) instead of holding 63 doubles per lane.
//   2. horizontal pass: the tile's rows need the intermediate rows [r0, r1) of the source; their 32 columns x 3 colours are spread
//      over the lanes colour-fastest (a lane's neighbours read the neighbouring source bytes), each element one window sum over
//      byte loads from global memory, rounded and stored to LDS as a byte.
//   3. vertical pass + store: a tile row is 96 consecutive bytes of the output; it is cut at the 4-byte boundaries of its global
//      address into at most 25 slots, one lane per slot (8 x 25 = 200 lanes).  A lane sums its slot's up to four columns from LDS and
//      stores them as one dword where the slot is whole, byte by byte at the ragged ends of the row.
// An axis that is not resampled gets the identity window (n = 1, k = 1 << 22), which returns the byte exactly: one code path.
// LDS is static: 8.25 KiB column windows, 2.1 KiB row windows, 27 KiB intermediate rows.  The bound of ops.h (in <= 31 * out)
// makes every window at most 63 taps and a tile's intermediate rows at most 7 * 31 + 63 = 280; the kernel clamps both to its stages
// as well, so that no geometry can index outside them.
#include <algorithm>

#include "hip_util.h"

namespace swn {
namespace {

constexpr int TH = 8, TW = 32, KMAX = 64, RMAX = 288, NB = 64;
static_assert(2 * RESIZE_MAX_FACTOR + 1 <= KMAX && (TH - 1) * RESIZE_MAX_FACTOR + 2 * RESIZE_MAX_FACTOR + 1 <= RMAX, "stages too small for the bound");

struct RZGeom { unsigned long long off; int H0, W0; };
struct RZp {
  const uint8_t* src; uint8_t* dst;
  int Hs, Ws;
  RZGeom g[NB];
};

__device__ __forceinline__ double tri(double a) {
  if (a < 0.0) a = -a;
  return a < 1.0 ? 1.0 - a : 0.0;
}

// the window of output index xx on an axis in -> out (Resample.c precompute_coeffs + normalize_coeffs_8bpc), taps into k[0 .. KMAX)
__device__ void window(int xx, int in, int out, int* kmin, int* kn, int* k) {
  if (in == out) { *kmin = xx; *kn = 1; k[0] = 1 << 22; return; }
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * fs;
  const double ss = 1.0 / fs;
  const double center = ((double)xx + 0.5) * scale;
  const double lo = center - support;
  const double hi = center + support;
  int xmin = (int)(lo + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(hi + 0.5);
  if (xmax > in) xmax = in;
  int n = xmax - xmin;
  if (n > KMAX) n = KMAX;                                // (never under the bound of ops.h: the stage's own guard)
  double ww = 0.0;
  for (int x = 0; x < n; ++x) {
    const double d = (double)(x + xmin) - center;
    const double e = d + 0.5;
    ww = ww + tri(e * ss);
  }
  for (int x = 0; x < n; ++x) {
    const double d = (double)(x + xmin) - center;
    const double e = d + 0.5;
    double w = tri(e * ss);
    if (ww != 0.0) w = w / ww;
    const double q = w * 4194304.0;
    k[x] = (int)(0.5 + q);
  }
  *kmin = xmin; *kn = n;
}

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void resize_u8_kernel(const RZp p) {
  __shared__ int hk[TW][KMAX + 1];                       // (+1: the 32 lanes of a column read walk different banks)
  __shared__ int hmin[TW], hn[TW];
  __shared__ int vk[TH][KMAX + 1];
  __shared__ int vmin[TH], vn[TH];
  __shared__ uint8_t inter[RMAX][TW * 3];

  const int b = blockIdx.z, t = threadIdx.x;
  const int H0 = p.g[b].H0, W0 = p.g[b].W0;
  const uint8_t* im = p.src + p.g[b].off;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int tw = min(TW, p.Ws - x0), th = min(TH, p.Hs - y0);

  // ---- 1. the windows of this tile's columns and rows
  if (t < tw) window(x0 + t, W0, p.Ws, &hmin[t], &hn[t], hk[t]);
  else if (t >= 64 && t - 64 < th) window(y0 + t - 64, H0, p.Hs, &vmin[t - 64], &vn[t - 64], vk[t - 64]);
  __syncthreads();

  // the intermediate rows the tile reads: windows move monotonically with the output index
  const int r0 = vmin[0];
  const int nrows = min(vmin[th - 1] + vn[th - 1] - r0, RMAX);

  // ---- 2. horizontal pass of those rows into LDS, as rounded bytes
  const int rowlen = tw * 3;
  for (int e = t; e < nrows * rowlen; e += 256) {
    const int row = e / rowlen, j = e - row * rowlen;
    const int col = j / 3, c = j - col * 3;
    const uint8_t* sp = im + ((size_t)(r0 + row) * W0 + hmin[col]) * 3 + c;
    const int n = hn[col];
    int acc = 1 << 21;
    for (int x = 0; x < n; ++x) acc += (int)sp[(size_t)x * 3] * hk[col][x];
    inter[row][j] = (uint8_t)clip8(acc);
  }
  __syncthreads();

  // ---- 3. vertical pass from LDS; a lane owns one 4-byte slot of one tile row of the output
  constexpr int SLOTS = (TW * 3 + 3) / 4 + 1;            // a 96-byte row that starts off a boundary touches 25 dwords
  const int y = t / SLOTS, slot = t - y * SLOTS;
  if (y >= th) return;
  uint8_t* drow = p.dst + (((size_t)b * p.Hs + y0 + y) * p.Ws + x0) * 3;
  const int lead = (int)((uintptr_t)drow & 3);           // bytes of the row's first dword that belong to the pixel before it
  const int j0 = slot * 4 - lead;                        // the slot's bytes are the row's [j0, j0 + 4)
  const int ja = max(j0, 0), jb = min(j0 + 4, rowlen);
  if (ja >= jb) return;
  const int n = vn[y], rbase = vmin[y] - r0;
  int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
  for (int x = 0; x < n; ++x) {
    const int kx = vk[y][x];
    const int r = min(rbase + x, RMAX - 1);              // (never clamps under the bound of ops.h)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (j0 + i >= ja && j0 + i < jb) acc[i] += (int)inter[r][j0 + i] * kx;
  }
  if (jb - ja == 4) {
    const unsigned v = (unsigned)clip8(acc[0]) | ((unsigned)clip8(acc[1]) << 8) | ((unsigned)clip8(acc[2]) << 16) | ((unsigned)clip8(acc[3]) << 24);
    *reinterpret_cast<unsigned*>(drow + j0) = v;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (j0 + i >= ja && j0 + i < jb) drow[j0 + i] = (uint8_t)clip8(acc[i]);
  }
}

}  // namespace

void resize_u8(Stream& s, const ResizeU8Args& a) {
  resize_u8_check(a);                                     // every sample, before the first launch
  const dim3 tiles((unsigned)((a.Ws + TW - 1) / TW), (unsigned)((a.Hs + TH - 1) / TH), 1);
  if (tiles.y > 65535u) throw Error(1, "resize_u8: output too high for one launch (" + std::to_string(a.Hs) + " rows)");
  for (int b0 = 0; b0 < a.B; b0 += NB) {                  // the geometry travels by value, 64 samples a launch
    const int nb = std::min(NB, a.B - b0);
    RZp p{};
    p.src = a.src; p.dst = a.dst + (size_t)b0 * a.Hs * a.Ws * 3; p.Hs = a.Hs; p.Ws = a.Ws;
    for (int b = 0; b < nb; ++b) {
      const int64_t* g = a.geom + 3 * (size_t)(b0 + b);
      p.g[b].off = (unsigned long long)g[0]; p.g[b].H0 = (int)g[1]; p.g[b].W0 = (int)g[2];
    }
    hipLaunchKernelGGL(resize_u8_kernel, dim3(tiles.x, tiles.y, (unsigned)nb), dim3(256), 0, hs(s), p);
    check_launch("resize_u8");
  }
}

}  // namespace swn
