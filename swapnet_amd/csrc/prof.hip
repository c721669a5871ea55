// swapnet_amd -- per-launch profiling of the implicit-GEMM launches (HIP events on the launch stream; conv_gemm.h ProfScope)
// and the MFMA throughput probe.
#include <array>
#include <cstdarg>
#include <map>
#include <vector>

#include "conv_gemm.h"

namespace swn {

static int g_prof = 0;
static std::vector<ProfRec> g_recs;

ProfScope::ProfScope(const Stream& s, const char* name, double flops) : st(hs(s)), on(g_prof != 0) {
  if (route_on()) route_note(name);
  if (!on) return;
  r.name = name; r.flops = flops;
  (void)hipEventCreate(&r.a); (void)hipEventCreate(&r.b);
  (void)hipEventRecord(r.a, st);
}
ProfScope::~ProfScope() {
  if (!on) return;
  (void)hipEventRecord(r.b, st);
  g_recs.push_back(r);
}

void prof_name(char (&buf)[128], const char* base, const char* detail, ...) {
  char fmt[128];
  snprintf(fmt, sizeof fmt, "%s%s", base, prof_detail() ? detail : "");
  va_list ap;
  va_start(ap, detail);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
}

void prof_enable(int on) { g_prof = on; }
void prof_reset() {
  for (auto& r : g_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  g_recs.clear();
}
int prof_report(char* buf, int len) {
  std::map<std::string, std::array<double, 3>> agg;
  for (auto& r : g_recs) {
    (void)hipEventSynchronize(r.b);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    auto& a = agg[r.name];
    a[0] += 1; a[1] += ms; a[2] += r.flops;
  }
  std::string out;
  for (auto& kv : agg) {
    char line[256];
    snprintf(line, sizeof line, "%s %.0f %.6f %.6e\n", kv.first.c_str(), kv.second[0], kv.second[1], kv.second[2]);
    out += line;
  }
  if (buf && len > 0) { strncpy(buf, out.c_str(), len - 1); buf[len - 1] = 0; }
  return (int)out.size();
}

// ---- swn_probe_mfma: what the matrix pipe sustains for the ring kernels' instruction mix, operands in registers ----------------
__global__ __launch_bounds__(256, 4) void mfma_probe_kernel(int iters, int zeros, unsigned long long* clk, float* sink) {
  unsigned long long c0 = 0, r0 = 0;
  const bool me = blockIdx.x % 61 == 0 && blockIdx.x / 61 < 16 && threadIdx.x == 0;
  if (me) { c0 = __builtin_readcyclecounter(); r0 = __builtin_amdgcn_s_memrealtime(); }
  // fp16 bit patterns from a per-lane hash: sign, exponents 2^-3 .. 2^0, random mantissas (finite, products stay far from overflow)
  unsigned h = (blockIdx.x * 256u + threadIdx.x) * 2654435761u + 12345u;
  auto word = [&]() {
    h = h * 1664525u + 1013904223u;
    const unsigned lo = (h >> 3) & 0x83ffu, hi = (h >> 17) & 0x83ffu;
    return zeros ? 0u : ((lo | 0x3000u | ((h & 3u) << 10)) | ((hi | 0x3000u | (((h >> 2) & 3u) << 10)) << 16));
  };
  u32x4 ah, al, bh[4], bl[4];
  for (int q = 0; q < 4; ++q) { ah[q] = word(); al[q] = word(); }
  for (int j = 0; j < 4; ++j) for (int q = 0; q < 4; ++q) { bh[j][q] = word(); bl[j][q] = word(); }
  f32x16 acc[4];
  for (int j = 0; j < 4; ++j) for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = mma_f16(al, bh[j], acc[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = mma_f16(ah, bl[j], acc[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = mma_f16(ah, bh[j], acc[j]);
    asm volatile("" ::: "memory");
  }
  float t = 0.f;
  for (int j = 0; j < 4; ++j) for (int e = 0; e < 16; ++e) t += acc[j][e];
  if (t == 12345.678f) sink[0] = t;                                  // (keeps the accumulators alive)
  if (me) { clk[2 * (blockIdx.x / 61)] = __builtin_readcyclecounter() - c0; clk[2 * (blockIdx.x / 61) + 1] = __builtin_amdgcn_s_memrealtime() - r0; }
}
void probe_mfma(Stream& s, int zeros, int iters, float* out4) {
  if (!s.ws || s.ws_bytes < 4096) throw Error(1, "probe_mfma: the stream scratch is missing");
  unsigned long long* clk = reinterpret_cast<unsigned long long*>(s.ws);
  float* sink = reinterpret_cast<float*>(s.ws + 512);
  const int blocks = 1024;
  hipEvent_t e0, e1;
  SWN_HIP_CHECK(hipEventCreate(&e0)); SWN_HIP_CHECK(hipEventCreate(&e1));
  // steady state, not a burst: the chip's power management settles over milliseconds (a single launch after an idle gap runs
  // 30-40 % faster than the same launch inside a train of them).  Twelve launches back to back; the last six are timed.
  constexpr int WARM = 6, TIMED = 6;
  SWN_HIP_CHECK(hipMemsetAsync(clk, 0, 256, hs(s)));
  for (int rep = 0; rep < WARM + TIMED; ++rep) {
    if (rep == WARM) SWN_HIP_CHECK(hipEventRecord(e0, hs(s)));
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(blocks), dim3(256), 0, hs(s), iters, zeros, clk, sink);
  }
  SWN_HIP_CHECK(hipEventRecord(e1, hs(s)));
  SWN_HIP_CHECK(hipEventSynchronize(e1));
  float best = 0.f; SWN_HIP_CHECK(hipEventElapsedTime(&best, e0, e1));
  best /= TIMED;
  SWN_HIP_CHECK(hipEventDestroy(e0)); SWN_HIP_CHECK(hipEventDestroy(e1));
  unsigned long long h[32];
  SWN_HIP_CHECK(hipMemcpy(h, clk, sizeof h, hipMemcpyDeviceToHost));
  int wall_khz = 0, dev = 0;
  SWN_HIP_CHECK(hipGetDevice(&dev));
  SWN_HIP_CHECK(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, dev));
  double cs = 0, rs = 0;
  for (int i = 0; i < 16; ++i) { cs += (double)h[2 * i]; rs += (double)h[2 * i + 1]; }
  const double ghz = rs > 0 ? cs / rs * wall_khz * 1e-6 : 0.0;
  const double mfmas = (double)blocks * 4 * iters * 12;               // per launch
  out4[0] = (float)(mfmas * 32768.0 / (best * 1e-3) * 1e-12);
  out4[1] = (float)ghz;
  out4[2] = best;
  out4[3] = ghz > 0 ? (float)(mfmas * 32.0 / 1024.0 / (best * 1e-3 * ghz * 1e9)) : 0.f;
}

}  // namespace swn
