// swapnet_amd -- the per-pixel arithmetic of the SSIM and Charbonnier losses (modules/losses/__init__.py:14-35,128-259), plain
// inline functions shared by the HIP kernels (ssim.hip) and the host form (engine.cpp): the same expressions in the same order.
//
// With f = the zero-padded depthwise Gaussian filter and the five filtered maps m1 = f(x), m2 = f(y), e11 = f(x^2), e22 = f(y^2),
// e12 = f(xy):
//   s1 = e11 - m1^2, s2 = e22 - m2^2, s12 = e12 - m1 m2
//   N1 = 2 m1 m2 + C1, N2 = 2 s12 + C2, D1 = m1^2 + m2^2 + C1, D2 = s1 + s2 + C2,  S = N1 N2 / (D1 D2)
//   loss = clamp(1 - S, 0, 1) / 2
// Gradient under an upstream g: g' = -g / 2 where 0 <= 1 - S <= 1 (torch's clamp passes the gradient at both ends), else 0;
//   dx = f(a1) + 2 x f(b) + y f(c),  dy = f(a2) + 2 y f(b) + x f(c)          (f is its own adjoint: symmetric, odd, zero padding)
//   b  = g' dS/de11 = g' dS/de22 = -g' S / D2                                 (D2 is symmetric in s1, s2)
//   c  = g' dS/de12 = 2 g' N1 / (D1 D2)
//   a1 = g' dS/dm1 with the m-dependence of s1 and s12 folded in = g' (2 m2 (N2 - N1) / (D1 D2) - 2 m1 S / D1 + 2 m1 S / D2)
//   a2 = the same with m1 and m2 exchanged.
#pragma once
#include <math.h>

#if defined(__HIP__)
#define SSIM_HD __host__ __device__ inline
#else
#define SSIM_HD inline
#endif

namespace swn {

constexpr int SSIM_MAX_WINDOW = 15;        // the largest window the kernels are instantiated for (odd sizes 1 .. 15)

// gaussian(window_size, 1.5) of the reference (:30-35) in float32: exp(-(i - ws / 2)^2 / 4.5), normalised by its float32 sum
struct SsimWindow { float w[SSIM_MAX_WINDOW]; };
inline SsimWindow ssim_window(int ws) {
  SsimWindow g;
  float sum = 0.f;
  for (int i = 0; i < SSIM_MAX_WINDOW; ++i) g.w[i] = 0.f;
  for (int i = 0; i < ws; ++i) {
    const float x = (float)(i - ws / 2);
    g.w[i] = expf(-(x * x) / 4.5f);
    sum += g.w[i];
  }
  for (int i = 0; i < ws; ++i) g.w[i] /= sum;
  return g;
}
// C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2: Python floats in the reference (:190-191), rounded to float32 where they meet the maps
inline float ssim_c1(float max_val) { const double v = 0.01 * (double)max_val; return (float)(v * v); }
inline float ssim_c2(float max_val) { const double v = 0.03 * (double)max_val; return (float)(v * v); }

struct SsimMoments { float m1, m2, e11, e22, e12; };
// one tap of the row pass: the five products of a pixel pair enter the filter
SSIM_HD void ssim_tap(SsimMoments& a, float w, float x, float y) {
  a.m1 += w * x; a.m2 += w * y; a.e11 += w * (x * x); a.e22 += w * (y * y); a.e12 += w * (x * y);
}
struct SsimTerms { float N1, N2, D1, D2, S; };
SSIM_HD SsimTerms ssim_terms(const SsimMoments& m, float C1, float C2) {
  const float m11 = m.m1 * m.m1, m22 = m.m2 * m.m2, m12 = m.m1 * m.m2;
  const float s1 = m.e11 - m11, s2 = m.e22 - m22, s12 = m.e12 - m12;
  SsimTerms t;
  t.N1 = 2.f * m12 + C1; t.N2 = 2.f * s12 + C2;
  t.D1 = m11 + m22 + C1; t.D2 = s1 + s2 + C2;
  t.S = (t.N1 * t.N2) / (t.D1 * t.D2);
  return t;
}
// clamp(1 - S, 0, 1) / 2; a NaN stays a NaN, as in torch.clamp
SSIM_HD float ssim_loss_of(float S) {
  const float d = 1.f - S;
  return (d < 0.f ? 0.f : (d > 1.f ? 1.f : d)) / 2.f;
}
struct SsimCoefs { float a1, a2, b, c; };
SSIM_HD SsimCoefs ssim_coefs(const SsimMoments& m, const SsimTerms& t, float g) {
  const float d = 1.f - t.S;
  SsimCoefs o = {0.f, 0.f, 0.f, 0.f};
  if (!(d >= 0.f && d <= 1.f)) return o;          // the clamped branches: exactly zero, whatever the quotients below would be
  const float gp = -0.5f * g;
  const float dd = t.D1 * t.D2;
  const float sd1 = t.S / t.D1, sd2 = t.S / t.D2;
  const float k = 2.f * (t.N2 - t.N1) / dd;
  o.b = gp * -sd2;
  o.c = gp * (2.f * t.N1 / dd);
  o.a1 = gp * (m.m2 * k - 2.f * m.m1 * sd1 + 2.f * m.m1 * sd2);
  o.a2 = gp * (m.m1 * k - 2.f * m.m2 * sd1 + 2.f * m.m2 * sd2);
  return o;
}

// Charbonnier (:14-27): sqrt(d^2 + eps) per element, d = x - y; d/dx = g d / sqrt(d^2 + eps), d/dy = -that
SSIM_HD float charbonnier_term(float x, float y, float eps, float g, float* grad) {
  const float d = x - y;
  const float e = sqrtf(d * d + eps);
  *grad = g * d / e;
  return e;
}

}  // namespace swn
