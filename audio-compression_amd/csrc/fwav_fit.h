// fwav_fit.h — the least-squares fit of one (range, tile orientation) pair and the order its winner is the minimum of:
// shared by fwav_affine.hip (K candidates per range) and fwav_affine_all.hip (every domain of the pool).
//
// The fit is stated once per operand form, and a change to it is made in these functions:
//   fit_any<FIT>                        one orientation, run-time length, operands in memory
//   orient_domain<RS> + orient_pair<RS, FIT>   one orientation, fixed length: the half that reads the tile alone
//                                       (d̄, d̃, Σd̃² + 1e-12) and the half that needs the range (Σd̃r̃, s, o, Σ(sD + o − R)²)
//   eval_orient<RS, FIT>                their composition, operands in registers
// (affine_one of fwav_affine.hip is the packed form of the benchmark's solve.)  Around them: gather_row (a tile into
// registers), FitOrder<FIT> (the tie-break key of a slot and the order the winner is the minimum of), wave_best /
// store_best (a wave's reduction and the five outputs).
#pragma once

#include <type_traits>

#include "fwav_common.h"

namespace fwav {

constexpr int kAffWaves = 4;
constexpr int kFitReference = 0, kFitClipped = 1;

struct Best {
  float err, s, o;
  int slot, dom;  // slot: the slot's FitOrder key
};

// (e1, k1) before (e2, k2) in the reference's argmin order: the first NaN error, else the smaller error, else the
// smaller key
template <class Key>
__device__ __forceinline__ bool first_min(float e1, Key k1, float e2, Key k2) {
  const bool n1 = e1 != e1, n2 = e2 != e2;
  if (n1 || n2) return (n1 && n2) ? k1 < k2 : n1;
  return e1 < e2 || (e1 == e2 && k1 < k2);
}

// The selection order of a fit mode.  kFitReference: the key is the slot (first minimum over [K | K mirrored]).
// kFitClipped: domain·2 + mirrored, compared as u32 (Best carries it in an int).
template <int FIT>
struct FitOrder {
  using Key = std::conditional_t<FIT == kFitClipped, uint32_t, int>;
  static constexpr int none = FIT == kFitClipped ? -1 : 0x7fffffff;  // the key no slot has: it loses every tie
  static __device__ __forceinline__ int key(int slot, int32_t dom, int mirrored) {
    if constexpr (FIT == kFitClipped) return (int)((uint32_t)dom * 2u + (uint32_t)mirrored);
    return slot;
  }
  static __device__ __forceinline__ bool better(float e1, int k1, float e2, int k2) {
    return first_min<Key>(e1, (Key)k1, e2, (Key)k2);
  }
  static __device__ __forceinline__ bool mirrored(int key, int K) {
    return FIT == kFitClipped ? (key & 1) != 0 : key >= K;
  }
};

// Tile `di` (a row index, already clamped to ≥ 0) of the pool into registers.
template <int RS>
__device__ __forceinline__ void gather_row(const float* __restrict__ pool, int64_t di, float (&D)[RS]) {
  if constexpr (RS % 4 == 0) {
    const float4* p = reinterpret_cast<const float4*>(pool + di * RS);
#pragma unroll
    for (int j = 0; j < RS / 4; ++j) {
      const float4 v = p[j];
      D[4 * j] = v.x; D[4 * j + 1] = v.y; D[4 * j + 2] = v.z; D[4 * j + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < RS; ++i) D[i] = pool[di * RS + i];
  }
}

// The half of the fit that reads one orientation X of a tile alone: dm = d̄, dc = d̃ = X − d̄, den = Σd̃² + 1e-12.
template <int RS>
__device__ __forceinline__ void orient_domain(const float (&X)[RS], float& dm, float (&dc)[RS], float& den) {
  auto fx = [&](int i) { return X[i]; };
  dm = pw_sum_n<RS>(fx) / (float)RS;
#pragma unroll
  for (int i = 0; i < RS; ++i) dc[i] = X[i] - dm;
  auto fd = [&](int i) { return dc[i] * dc[i]; };
  den = pw_sum_n<RS>(fd) + 1e-12f;
}

// ... and the half that needs the range R (rc = R − rm) too: s, o and the error's sum of squares `ss` (err = √ss) from
// orient_domain's values.  fx(i) = X[i] and fdc(i) = dc[i] read the tile from wherever it is; c = |s_clip|.
template <int RS, int FIT, class FX, class FDC>
__device__ __forceinline__ void orient_pair(const FX& fx, const FDC& fdc, float dm, float den, const float (&R)[RS],
                                            const float (&rc)[RS], float rm, float c, float& s, float& o, float& ss) {
  auto fn = [&](int i) { return fdc(i) * rc[i]; };
  const float num = pw_sum_n<RS>(fn);
  s = num / den;
  if constexpr (FIT == kFitClipped) s = clip_sym(s, c);
  o = rm - s * dm;
  auto fe = [&](int i) {
    const float df = (s * fx(i) + o) - R[i];
    return df * df;
  };
  ss = pw_sum_n<RS>(fe);
}

// The fit of one orientation X of a tile against range R (rc = R − rm), fixed length, operands in registers; c = |s_clip|.
template <int RS, int FIT = kFitReference>
__device__ __forceinline__ void eval_orient(const float (&X)[RS], const float (&R)[RS], const float (&rc)[RS], float rm,
                                            float& s, float& o, float& err, float c = 0.f) {
  float dm, den, ss, dc[RS];
  orient_domain<RS>(X, dm, dc, den);
  orient_pair<RS, FIT>([&](int i) { return X[i]; }, [&](int i) { return dc[i]; }, dm, den, R, rc, rm, c, s, o, ss);
  err = sqrtf(ss);
}

// The same fit at a run-time length n, operands read from memory: tile D as stored (orient 0) or mirrored (1) against
// range R of mean rm; c = |s_clip|.
template <int FIT>
__device__ __forceinline__ void fit_any(const float* __restrict__ D, int orient, const float* __restrict__ R, float rm,
                                        int n, float c, float& s_out, float& o_out, float& err) {
  auto X = [&](int i) { return orient ? D[n - 1 - i] : D[i]; };
  const float dm = pw_sum(X, n) / (float)n;
  auto fn = [&](int i) { return (X(i) - dm) * (R[i] - rm); };
  auto fd = [&](int i) {
    const float t = X(i) - dm;
    return t * t;
  };
  const float num = pw_sum(fn, n);
  const float den = pw_sum(fd, n) + 1e-12f;
  const float s = FIT == kFitClipped ? clip_sym(num / den, c) : num / den;
  const float o = rm - s * dm;
  auto fe = [&](int i) {
    const float df = (s * X(i) + o) - R[i];
    return df * df;
  };
  err = sqrtf(pw_sum(fe, n));
  s_out = s;
  o_out = o;
}

// The wave's best of every lane's: a 6-step xor-shuffle reduction in the mode's order; every lane ends with it.
template <int FIT>
__device__ __forceinline__ void wave_best(Best& b) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    Best o;
    o.err = __shfl_xor(b.err, m);
    o.s = __shfl_xor(b.s, m);
    o.o = __shfl_xor(b.o, m);
    o.slot = __shfl_xor(b.slot, m);
    o.dom = __shfl_xor(b.dom, m);
    if (FitOrder<FIT>::better(o.err, o.slot, b.err, b.slot)) b = o;
  }
}

template <int FIT>
__device__ __forceinline__ void store_best(const Best& b, int64_t r, int K, float sc, int32_t* __restrict__ out_idx,
                                           float* __restrict__ out_s, float* __restrict__ out_o,
                                           uint8_t* __restrict__ out_sym, float* __restrict__ out_err) {
  out_idx[r] = b.dom;
  out_s[r] = clip_sym(b.s, sc);  // (kFitClipped: already clipped; the clip is idempotent)
  out_o[r] = b.o;
  out_sym[r] = (uint8_t)FitOrder<FIT>::mirrored(b.slot, K);
  out_err[r] = b.err;
}

}  // namespace fwav
