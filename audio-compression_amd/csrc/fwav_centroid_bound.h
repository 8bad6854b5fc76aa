// fwav_centroid_bound.h — the centroid pre-filter's threshold (fwav_topk.hip, CENT geometry), in plain
// C++17 so the kernel and a host test run the same code.
//
// Heads h = 0, 1 of 8 dimensions.  A centroid's fp16 vector is c (as fed to the MFMA), member m's fp16 high part q_m,
// e_m = q_m − c (exact in f32: a difference of two fp16 values).  n_h = ‖c_h‖, ĉ_h = c_h / n_h, N² = n_0² + n_1²,
// β_{m,h} = e_{m,h}·ĉ_h, ‖e⊥_{m,h}‖² = ‖e_{m,h}‖² − β_{m,h}², Γ = Σ_h max_m |β_{m,h}|, σ² = Σ_h max_m ‖e⊥_{m,h}‖².
// D = 1 + 2⁻⁹ bounds the norm of a head of the fp16 table: the f32 heads have norm ≤ 1, rounding to fp16 moves a
// normal component by at most 2⁻¹¹ of itself and a subnormal one by at most 2⁻²⁵, so a rounded head has norm
// ≤ 1 + 2⁻¹¹ + √8·2⁻²⁵ < D.
//
// For a table row d put a_h = ĉ_h·d_h (|a_h| ≤ D).  Then
//   q_m·d = c·d + Σ_h (β_{m,h} a_h + e⊥_{m,h}·d⊥_h) ≤ c·d + Γ·D + Σ_h σ_h √(D² − a_h²)
//         ≤ c·d + Γ·D + σ √(2D² − a_0² − a_1²)                         (Cauchy–Schwarz over the heads)
// and (c·d)² = (n_0 a_0 + n_1 a_1)² ≤ N² (a_0² + a_1²), so with s = s16(c, d)
//   s16(q_m, d) ≤ g(s) = s + Γ·D + σ √max(0, 2D² − s²/N²) + η.
// η = 1e-5 is the rounding allowance: the two MFMA accumulations (s16(c, d) and s16(q_m, d): 16 f32 roundings each of
// partial sums ≤ 2, ≤ 16 · 2⁻²⁴ · 2 · 2 < 3.9e-6) and the f32 evaluation of the threshold below (t, t/A and the root:
// a handful of roundings of values ≤ 2 and the device's 1-ulp 1/x and √x, < 1e-6; the constants themselves are
// rounded towards the safe side, see cent_bound).  g rises with s up to its maximum √2·D·N·√A (A = 1 + σ²/N²), so when g(0) < t_min every s below the
// smaller root s* of g(s) = t_min, negative s included, has g(s) < t_min:
//   s* = (t − √(σ²(2D²A − t²/N²))) / A,   t = t_min − Γ·D − η
// (the quadratic's (t − √(t² − A(t² − 2σ²D²))) / A with the radicand expanded: that form cancels in f32).  A radicand
// below zero means t_min is above g's maximum: no row can reach it and any threshold is valid; it counts as zero.
// The filter threshold is max(t_min − slack, s*), where slack = (ρ_0 + ρ_1)·D + η, ρ_h = max_m ‖e_{m,h}‖, is the
// worst case of Cauchy–Schwarz; it alone holds when g(0) ≥ t_min (cold or −∞ limits), when the centroid is all zero,
// and for a non-finite t_min.  A head with n_h = 0 has β = 0 and e⊥ = e (its a_h does not enter s).
#ifndef FWAV_CENTROID_BOUND_H
#define FWAV_CENTROID_BOUND_H

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FWAV_HD __host__ __device__
#else
#define FWAV_HD
#endif

namespace fwav {

constexpr float kCentD = 1.0f + 0x1p-9f;  // D: a head of the fp16 table has norm ≤ D
constexpr float kCentEta = 1e-5f;         // η: rounding allowance

// One head's terms of a centroid: n² = ‖c_h‖², ρ = max_m ‖e_{m,h}‖, β = max_m |β_{m,h}|, p² = max_m ‖e⊥_{m,h}‖².
struct CentHead {
  float n2, rho, beta, perp2;
};
// The lane's constants of the filter threshold: slack = (ρ_0 + ρ_1)·D + η, gd = Γ·D + η, k0 = 2σ²D², k2 = σ²/N²
// (gd = +∞: the centroid is all zero, only the slack holds).
struct CentBound {
  float slack, gd, k0, k2;
};

// 1/x and √x of the per-group threshold: on the device the hardware's one-instruction forms (1 ulp each; the
// correctly rounded ones cost ≈ 25 instructions per wave and group), part of η's evaluation share.
FWAV_HD inline float cent_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcpf(x);
#else
  return 1.0f / x;
#endif
}
FWAV_HD inline float cent_sqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sqrtf(x);
#else
  return sqrtf(x);
#endif
}

FWAV_HD inline void cent_head_begin(CentHead& t, const float (&c)[8]) {
  float n2 = 0.0f;
  for (int i = 0; i < 8; ++i) n2 += c[i] * c[i];
  t = CentHead{n2, 0.0f, 0.0f, 0.0f};
}
// Adds member q (one head: 8 fp16 values as floats) of the centroid c to the head's terms.  β and p² are rounded up
// by more than their f32 evaluation can lose: the dot products of 8 terms are off by < 2⁻²¹ of Σ|x_i y_i|, so β by
// < 2⁻²⁰·‖e‖ and e² − β² by < 2⁻¹⁸·e².
FWAV_HD inline void cent_head_member(CentHead& t, const float (&c)[8], const float (&q)[8]) {
  float e2 = 0.0f, ec = 0.0f;
  for (int i = 0; i < 8; ++i) {
    const float e = q[i] - c[i];  // exact: a difference of two fp16 values
    e2 += e * e;
    ec += e * c[i];
  }
  const float en = sqrtf(e2);
  t.rho = fmaxf(t.rho, en);
  float b2 = 0.0f;
  if (t.n2 > 0.0f) {
    b2 = fminf(ec * ec / t.n2, e2);
    t.beta = fmaxf(t.beta, sqrtf(b2) + 0x1p-20f * en);
  }
  t.perp2 = fmaxf(t.perp2, (e2 - b2) + 0x1p-18f * e2);
}
// Both heads' terms → the lane's constants.  σ² is rounded up and N² down by 2⁻²⁰ (the sums' own roundings are 2⁻²⁴).
FWAV_HD inline CentBound cent_bound(const CentHead& h0, const CentHead& h1) {
  CentBound b;
  b.slack = (h0.rho + h1.rho) * kCentD + kCentEta;  // (ρ_0 + ρ_1)(1 + 2⁻⁹) + 1e-5
  const float N2 = (h0.n2 + h1.n2) * (1.0f - 0x1p-20f);
  const float s2 = (h0.perp2 + h1.perp2) * (1.0f + 0x1p-20f);
  if (N2 > 0.0f) {
    b.gd = (h0.beta + h1.beta) * kCentD + kCentEta;
    b.k0 = 2.0f * s2 * (kCentD * kCentD);
    b.k2 = s2 / N2;
  } else {
    b.gd = INFINITY;
    b.k0 = b.k2 = 0.0f;
  }
  return b;
}
// The filter threshold for the smallest stream threshold t_min of the centroid's members: a row d with
// s16(c, d) ≤ the result has s16(q_m, d) ≤ t_min for every member (the stream tests pass on '>').  `tight` = false:
// the slack alone.
FWAV_HD inline float cent_threshold(const CentBound& b, float tmin, bool tight = true) {
  const float old = tmin - b.slack;
  const float t = tmin - b.gd;
  if (!tight || !(t > 0.0f) || !(t < INFINITY)) return old;
  const float A = 1.0f + b.k2;
  // the radicand σ²(2D²A − t²/N²), rounded up by 2⁻¹² of its first term (its evaluation loses < 2⁻²⁰ of it; near
  // zero the root would magnify that)
  const float rad = fmaxf(b.k0 * A * (1.0f + 0x1p-12f) - b.k2 * (t * t), 0.0f);
  const float s = (t - cent_sqrt(rad)) * cent_rcp(A);
  return s > 0.0f ? fmaxf(old, s) : old;  // s ≤ 0 ⟺ g(0) ≥ t_min
}

}  // namespace fwav

#endif  // FWAV_CENTROID_BOUND_H
