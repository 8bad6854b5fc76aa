// fwav_pool_embed.hip — domain pool (mean-pooled sliding tiles) and the 16-d two-head DCT embedding.
//
// Replaces (reference /root/reference/fractal.py):
//   build_domains_memmap     :285-334  pool[d, k] = mean(signal[d·step + k·bl : … + bl]), bl = tile // rs
//   build_domain_embeddings  :238-280  → multi_head_embedding :166-175 → tile_embedding :178-208 (tonal head)
//                                        + transient_embedding :154-164
//
// Pool.  Each mean is numpy's pairwise float32 sum / bl (bit-exact).  When bl % step == 0 (every config in
// BASELINE.json), pool[d, k] = S[d + k·(bl/step)] with S[j] the mean of the bl samples starting at j·step,
// so only ≈ n/step block means are computed instead of nd·rs (8× less work at tile 2048): k_block_means.
// Otherwise k_domain_pool computes every (d, k) directly.
//
// Embedding (per domain, one thread), bit-exact with the reference for range sizes 4, 8 and 16 (every config in
// BASELINE.json and the goldens):
//   tonal[j]     = f32( f32-DCT(x)[j+1] · w[j+1] ), j < min(8, rs−1), zero-padded to 8; ‖·‖ as np.linalg.norm of a
//                  1-D float32 vector evaluates it (OpenBLAS sdot: f32 products summed in f64, rounded to f32, f32
//                  sqrt); / ‖·‖ in f32 if ‖·‖ > f32(1e-8)                                    (fractal.py:178-208)
//   transient[k] = f64-DCT(f64(x[n] − x[n−1]) · w[n])[k], k < min(8, rs); ‖·‖ as ddot (n < 16: a sequential f64 fma
//                  chain) then sqrt; / ‖·‖ if > 1e-8; → f32                                  (fractal.py:154-164)
// with the DCTs scipy's own pocketfft operation sequence in each precision (fwav_dct.h) and w = np.linspace(1, 2, rs)
// as numpy computes it (i·(1/(rs−1)) + 1, last = 2).  Other range sizes take the f64 matrix DCT and are NOT bit-exact:
// the tonal head is within 2⁻²² of the exactly rounded (f64) embedding, so its distance from the reference's is the
// reference's own f32 DCT error (a few 1e-6 at rs 19 and 32, growing with a row's DC/AC ratio; measured figures in
// DESIGN.md §4a); the transient head is f64 on both sides until one final rounding (within 2⁻²³).  The pool is
// bit-exact at every size.  fwav_embed_tables packs the matrices and pocketfft's constants for both precisions.
//
// Exact embedding at further range sizes (fwav_pool_embed_exact → k_embed_exact, one thread per domain as above): the
// same two heads with pocketfft's general plan for a runtime n (fwav_dct_plan.h: rfftp's factor order and the passes
// radb4, radb2, radb3, radb5 and the generic radbg), bit-exact with the reference at every n from 4 to 49 and at 50,
// 54, 56, 60, 63 and 64 — the lengths at which pocketfft runs that plan and not Bluestein's.  The host builds the plan
// (dct_plan_build, a kernel argument) and the constants (dct_plan_constants → fwav_embed_tables_exact); a thread's two
// work buffers are columns of an LDS array, the f32 head then the f64 head in the same storage.  An unsupported range
// size is an error, never the matrix path; 4, 8 and 16 route to k_embed's fixed plans.  The default entry point stays
// fwav_pool_embed: tests/test_gpu_generic_rs.py holds it within 2⁻²² of the f64 embedding, which the reference's own
// f32 DCT is not.
#include "fwav_common.h"
#include "fwav_dct.h"
#include "fwav_dct_plan.h"
#include "../../include/fwav.h"

#include <utility>
#include <vector>

namespace fwav {

constexpr int kPoolThreads = 256;

template <int BL>
__device__ __forceinline__ float block_mean_fixed(const float* __restrict__ x) {
  auto f = [&](int i) { return x[i]; };
  return pw_sum_n<BL>(f) / (float)BL;
}

// S[j] = pairwise_mean(sig[j*step : j*step + bl]),  j < ns.
template <int BL>
__global__ void k_block_means(const float* __restrict__ sig, int64_t ns, int step, int bl, float* __restrict__ S) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ns) return;
  const float* x = sig + j * step;
  if constexpr (BL > 0) {
    S[j] = block_mean_fixed<BL>(x);
  } else {
    auto f = [&](int i) { return x[i]; };
    S[j] = pw_sum(f, bl) / (float)bl;
  }
}

// General pool: one thread per (d, k).
__global__ void k_domain_pool(const float* __restrict__ sig, int64_t nd, int rs, int step, int bl,
                              float* __restrict__ pool) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nd * rs) return;
  int64_t d = t / rs;
  int k = (int)(t - d * rs);
  const float* x = sig + d * step + (int64_t)k * bl;
  auto f = [&](int i) { return x[i]; };
  pool[t] = pw_sum(f, bl) / (float)bl;
}

// Embedding of one domain row x[0..rs) read as src[d*a + k*b]; optionally writes the pool row.
//   tab layout (f64): tonal rows [8][rs] then transient rows [8][rs]; zero rows past take / tk.
// fp16 copies of embedding row d for the similarity search, tiled [chunk of 256][half h][256][8] (fwav_topk.hip): the
// high part x_hi = f16(x) (the stream's pre-filter), then, one table further on, the low part x_lo = f16(x − x_hi)
// (the replay's refined score x_hi·y_hi + x_hi·y_lo + x_lo·y_hi).  Both conversions round to nearest even and keep
// fp16 subnormals (the hi/lo error bound, DESIGN §3.1, counts on them).
__device__ __forceinline__ void store_emb16(_Float16* __restrict__ emb16, int64_t nd, int64_t d, const float (&out)[16]) {
  const int64_t c = d >> 8, j = d & 255;
  const int64_t n16 = ((nd + 255) >> 8) * 256 * 16;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    typedef _Float16 half8 __attribute__((ext_vector_type(8)));
    half8 vh, vl;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      vh[e] = (_Float16)out[8 * hh + e];
      vl[e] = (_Float16)(out[8 * hh + e] - (float)vh[e]);
    }
    *reinterpret_cast<half8*>(emb16 + ((c * 2 + hh) * 256 + j) * 8) = vh;
    *reinterpret_cast<half8*>(emb16 + n16 + ((c * 2 + hh) * 256 + j) * 8) = vl;
  }
}

// The fp16 table of the wide search (fwav_topk_wide.hip; emb_dim = 16·NS): row d's high parts only, tiled
// [chunk of 256][16-column step s][half h][256][8], so that a chunk is one contiguous block of 256·16·NS halfs and a
// lane's MFMA fragment of step s (columns 16s + 8h …) is one 16-byte read.  Rounds to nearest even, keeps subnormals.
template <int NS>
__device__ __forceinline__ void store_embh(_Float16* __restrict__ embh, int64_t d, const float (&out)[16 * NS]) {
  typedef _Float16 half8 __attribute__((ext_vector_type(8)));
  const int64_t c = d >> 8, j = d & 255;
#pragma unroll
  for (int sh = 0; sh < 2 * NS; ++sh) {
    half8 vh;
#pragma unroll
    for (int e = 0; e < 8; ++e) vh[e] = (_Float16)out[8 * sh + e];
    *reinterpret_cast<half8*>(embh + ((c * 2 * NS + sh) * 256 + j) * 8) = vh;
  }
}

// ddot of a vector with itself as numpy's f64 norm evaluates it (OpenBLAS ddot, Haswell/SkylakeX kernel) for n ≤ 16
// values v(0 … n−1): below 16 a sequential fma chain; at 16 four lanes l[i % 4] += v_i·v_i (product and add rounded
// separately), folded (l0 + l2) + (l1 + l3).  (From 32 values on the order is another one: emb_dim stops at 32.)
template <class V>
__host__ __device__ __forceinline__ double ddot_self(const V& v, int n) {
  if (n < 16) {
    double s2 = 0.0;
    for (int j = 0; j < n; ++j) s2 = __builtin_fma(v(j), v(j), s2);
    return s2;
  }
  double l[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 16; ++i) l[i & 3] = l[i & 3] + v(i) * v(i);
  return (l[0] + l[2]) + (l[1] + l[3]);
}

// H = coefficients per head: 8 (emb_dim 16; emb16 = the two-part table of fwav_topk.hip) or 16 (emb_dim 32; emb16 =
// the wide search's table, store_embh).  tab layout (f64): tonal rows [H][rs] then transient rows [H][rs].
template <int RS, int H = 8>
__global__ void k_embed(const float* __restrict__ src, int64_t nd, int rs, int64_t a, int64_t b,
                        const double* __restrict__ tab, float* __restrict__ pool_out, float* __restrict__ emb,
                        _Float16* __restrict__ emb16) {
  int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= nd) return;
  const int n = RS > 0 ? RS : rs;
  const float* xs = src + d * a;
  const int take = n - 1 < H ? n - 1 : H;
  const int tk = n < H ? n : H;
  const double* tt = tab;
  const double* td = tab + H * n;
  float e[H];
  double t[H];
  float tf[H];
  if constexpr (RS == 4 || RS == 8 || RS == 16) {
    // exact path: scipy's pocketfft DCTs and numpy's / OpenBLAS's norm orders (see the file header)
    DctK<float, RS> kf;
    DctK<double, RS> kd;
    dct_load(kf, tab + 2 * H * RS);
    dct_load(kd, tab + 2 * H * RS + dct_block(RS));
    float x[RS];
#pragma unroll
    for (int i = 0; i < RS; ++i) x[i] = xs[i * b];
    if (pool_out) {
#pragma unroll
      for (int i = 0; i < RS; ++i) pool_out[d * RS + i] = x[i];
    }
    float c[RS];
#pragma unroll
    for (int i = 0; i < RS; ++i) c[i] = x[i];
    dct2_ortho<float, RS>(c, kf);
#pragma unroll
    for (int j = 0; j < H; ++j) e[j] = j < take ? (float)((double)c[j + 1 < RS ? j + 1 : 0] * kd.w[j + 1 < RS ? j + 1 : 0]) : 0.0f;
    double acc = 0.0;  // sdot: f32 products, f64 sum in index order, f32 result
#pragma unroll
    for (int j = 0; j < H; ++j) acc = acc + (double)(e[j] * e[j]);
    const float nrm = sqrtf((float)acc);
    if (nrm > 1e-8f) {
#pragma unroll
      for (int j = 0; j < H; ++j) e[j] = e[j] / nrm;
    }
    double dv[RS];
#pragma unroll
    for (int i = 0; i < RS; ++i) dv[i] = (double)(i == 0 ? x[0] - x[0] : x[i] - x[i - 1]) * kd.w[i];
    dct2_ortho<double, RS>(dv, kd);
    double s2 = 0.0;  // ddot, n < 16: fma chain
    if constexpr (H == 16 && RS == 16) {
      s2 = ddot_self([&](int j) { return dv[j]; }, 16);
    } else {
#pragma unroll
      for (int j = 0; j < H; ++j)
        if (j < tk) s2 = __builtin_fma(dv[j < RS ? j : 0], dv[j < RS ? j : 0], s2);
    }
    const double nrmd = sqrt(s2);
#pragma unroll
    for (int j = 0; j < H; ++j) {
      double v = j < tk ? dv[j < RS ? j : 0] : 0.0;
      if (nrmd > 1e-8) v = v / nrmd;
      tf[j] = (float)v;
    }
  } else {
    if (pool_out) {
      for (int i = 0; i < n; ++i) pool_out[d * n + i] = xs[i * b];
    }
    for (int j = 0; j < H; ++j) {
      double acc = 0.0;
      for (int i = 0; i < n; ++i) acc += tt[j * n + i] * (double)xs[i * b];
      e[j] = j < take ? (float)acc : 0.0f;
    }
    for (int j = 0; j < H; ++j) t[j] = 0.0;
    for (int i = 0; i < n; ++i) {
      float xi = xs[i * b];
      float xp = i == 0 ? xi : xs[(i - 1) * b];
      double dd = (double)(xi - xp);
      for (int j = 0; j < H; ++j) t[j] += td[j * n + i] * dd;
    }
    double acc = 0.0;  // tonal norm in sdot order
    for (int j = 0; j < H; ++j) acc = acc + (double)(e[j] * e[j]);
    const float nrm = sqrtf((float)acc);
    if (nrm > 1e-8f) {
      for (int j = 0; j < H; ++j) e[j] = e[j] / nrm;
    }
    double s2d = 0.0;  // transient: ddot over the tk kept coefficients (an fma chain below 16 of them)
    if (H == 16 && tk == 16) {
      s2d = ddot_self([&](int j) { return t[j]; }, 16);
    } else {
      for (int j = 0; j < H; ++j)
        if (j < tk) s2d = __builtin_fma(t[j], t[j], s2d);
    }
    const double nd64 = sqrt(s2d);
    for (int j = 0; j < H; ++j) {
      double v = j < tk ? t[j] : 0.0;
      if (nd64 > 1e-8) v = v / nd64;
      tf[j] = (float)v;
    }
  }
  // concatenation [tonal H | transient tk] then zero pad to 2·H (multi_head_embedding :170-175)
  float out[2 * H];
#pragma unroll
  for (int j = 0; j < 2 * H; ++j) out[j] = 0.0f;
#pragma unroll
  for (int j = 0; j < H; ++j) out[j] = e[j];
#pragma unroll
  for (int j = 0; j < H; ++j)
    if (j < tk) out[H + j] = tf[j];
  float4* o4 = reinterpret_cast<float4*>(emb + d * 2 * H);
#pragma unroll
  for (int j = 0; j < H / 2; ++j) o4[j] = make_float4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
  if (emb16 != nullptr) {
    if constexpr (H == 8) store_emb16(emb16, nd, d, out);
    else store_embh<H / 8>(emb16, d, out);
  }
}

// Domain-embedding rows → the fp16 tables of the search (store_emb16), for embeddings produced elsewhere.
__global__ __launch_bounds__(kPoolThreads) void k_emb16(const float* __restrict__ emb, int64_t nd,
                                                        _Float16* __restrict__ emb16) {
  const int64_t d = (int64_t)blockIdx.x * kPoolThreads + threadIdx.x;
  if (d >= nd) return;
  float out[16];
  const float4* p = reinterpret_cast<const float4*>(emb + d * 16);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 v = p[j];
    out[4 * j] = v.x; out[4 * j + 1] = v.y; out[4 * j + 2] = v.z; out[4 * j + 3] = v.w;
  }
  store_emb16(emb16, nd, d, out);
}

template <int RS, int H = 8>
static void launch_embed(const float* src, int64_t nd, int rs, int64_t a, int64_t b, const double* tab,
                         float* pool_out, float* emb, _Float16* emb16, hipStream_t st) {
  k_embed<RS, H><<<cdiv(nd, kPoolThreads), kPoolThreads, 0, st>>>(src, nd, rs, a, b, tab, pool_out, emb, emb16);
}

// pocketfft's sincos_2pibyn<T>(n)[idx] (Thigh = double for float and double): a two-level table of octant-reduced
// cos/sin in double, entries multiplied in double — reproduced so that the twiddles are pocketfft's own values.
struct SinCos2PiByN {
  size_t n, shift, mask;
  std::vector<std::pair<double, double>> v1, v2;
  static std::pair<double, double> calc(size_t x, size_t n, double ang) {
    x <<= 3;
    if (x < 4 * n) {
      if (x < 2 * n) {
        if (x < n) return {std::cos(double(x) * ang), std::sin(double(x) * ang)};
        return {std::sin(double(2 * n - x) * ang), std::cos(double(2 * n - x) * ang)};
      }
      x -= 2 * n;
      if (x < n) return {-std::sin(double(x) * ang), std::cos(double(x) * ang)};
      return {-std::cos(double(2 * n - x) * ang), std::sin(double(2 * n - x) * ang)};
    }
    x = 8 * n - x;
    if (x < 2 * n) {
      if (x < n) return {std::cos(double(x) * ang), -std::sin(double(x) * ang)};
      return {std::sin(double(2 * n - x) * ang), -std::cos(double(2 * n - x) * ang)};
    }
    x -= 2 * n;
    if (x < n) return {-std::sin(double(x) * ang), -std::cos(double(x) * ang)};
    return {-std::cos(double(2 * n - x) * ang), -std::sin(double(2 * n - x) * ang)};
  }
  explicit SinCos2PiByN(size_t n_) : n(n_) {
    const long double pi = 3.141592653589793238462643383279502884197L;
    const double ang = (double)(0.25L * pi / (long double)n);
    const size_t nval = (n + 2) / 2;
    shift = 1;
    while (((size_t)1 << shift) * ((size_t)1 << shift) < nval) ++shift;
    mask = ((size_t)1 << shift) - 1;
    v1.resize(mask + 1);
    v1[0] = {1.0, 0.0};
    for (size_t i = 1; i < v1.size(); ++i) v1[i] = calc(i, n, ang);
    v2.resize((nval + mask) / (mask + 1));
    v2[0] = {1.0, 0.0};
    for (size_t i = 1; i < v2.size(); ++i) v2[i] = calc(i * (mask + 1), n, ang);
  }
  std::pair<double, double> operator[](size_t idx) const {
    if (2 * idx <= n) {
      const auto x1 = v1[idx & mask], x2 = v2[idx >> shift];
      return {x1.first * x2.first - x1.second * x2.second, x1.first * x2.second + x1.second * x2.first};
    }
    idx = n - idx;
    const auto x1 = v1[idx & mask], x2 = v2[idx >> shift];
    return {x1.first * x2.first - x1.second * x2.second, -(x1.first * x2.second + x1.second * x2.first)};
  }
};

// DctK<T, n> constants (T = double if dbl, else float, stored as doubles) exactly as pocketfft / numpy compute them:
// T_dcst23 twiddle[i] = T(sincos_2pibyn(4n)[i+1].r); the first rfftp factor's twiddles (comp_twiddle); fct =
// T(1/sqrt(long double(2n))); sqrt2 = T(1.414…L); w = np.linspace(1, 2, n) in double (arange · (1/(n−1)) + 1, last 2).
void dct_constants(int n, bool dbl, double* out) {
  auto r = [&](long double v) { return dbl ? (double)v : (double)(float)v; };
  for (int i = 0; i < 9; ++i) out[n + i] = 0.0;
  const SinCos2PiByN s4(4 * (size_t)n), s1((size_t)n);
  for (int i = 0; i < n; ++i) out[i] = r(s4[i + 1].first);
  if (n == 8) {  // radb2, l1 = 1, ido = 4
    out[n + 0] = r(s1[1].first);
    out[n + 1] = r(s1[1].second);
  } else if (n == 16) {  // radb4, l1 = 1, ido = 4
    for (int j = 1; j < 4; ++j) {
      out[n + (j - 1) * 3 + 0] = r(s1[j].first);
      out[n + (j - 1) * 3 + 1] = r(s1[j].second);
    }
  }
  const double step = 1.0 / (double)(n - 1);
  for (int i = 0; i < n; ++i) out[n + 9 + i] = i == n - 1 ? 2.0 : (double)i * step + 1.0;
  out[2 * n + 9] = r(1.0L / std::sqrt((long double)(2 * n)));
  out[2 * n + 10] = r(1.414213562373095048801688724209698L);
}


// ---------------------------------------------------------------------------------------------------------------
// Exact embedding at any supported range size: pocketfft's general plan (fwav_dct_plan.h) for a runtime n.

// pocketfft takes rfftp (never Bluestein) for n < 50 and wherever (largest prime factor)² ≤ n; up to 64 that is every
// n but 51, 52, 53, 55, 57, 58, 59, 61 and 62.
bool dct_plan_supported(int n) {
  if (n < 4 || n > kPlanMaxN) return false;
  if (n < 50) return true;
  int m = n, lpf = 1;
  for (int d = 2; d * d <= m; ++d)
    while (m % d == 0) {
      lpf = d;
      m /= d;
    }
  if (m > 1) lpf = m;
  return lpf * lpf <= n;
}

// The plan of length n as a kernel argument (uniform: it lives in scalar registers): rfftp::factorize's factor order
// and comp_twiddle's offsets into a precision block's twiddle memory; pb = doubles per precision block.
struct DctPlan {
  int n, nf, pb;
  int ip[kPlanMaxFact], tw[kPlanMaxFact], tws[kPlanMaxFact];
};

bool dct_plan_build(int n, DctPlan& p) {
  if (!dct_plan_supported(n)) return false;
  p.n = n;
  p.nf = 0;
  for (int k = 0; k < kPlanMaxFact; ++k) p.ip[k] = p.tw[k] = p.tws[k] = 0;
  int len = n;
  auto add = [&](int f) {
    if (p.nf < kPlanMaxFact) p.ip[p.nf] = f;
    ++p.nf;
  };
  while (len % 4 == 0) {
    add(4);
    len >>= 2;
  }
  if (len % 2 == 0) {
    len >>= 1;
    add(2);
    if (p.nf <= kPlanMaxFact) std::swap(p.ip[0], p.ip[p.nf - 1]);
  }
  for (int d = 3; d * d <= len; d += 2)
    while (len % d == 0) {
      add(d);
      len /= d;
    }
  if (len > 1) add(len);
  if (p.nf > kPlanMaxFact) return false;
  int ptr = 0;
  for (int k = 0, l1 = 1; k < p.nf; ++k) {
    const int ip = p.ip[k], ido = n / (l1 * ip);
    p.tw[k] = ptr;
    if (k < p.nf - 1) ptr += (ip - 1) * (ido - 1);  // the last factor needs no twiddles
    if (ip > 5) {
      p.tws[k] = ptr;
      ptr += 2 * ip;
    }
    l1 *= ip;
  }
  p.pb = kPlanConst + n + ptr;
  return p.pb <= plan_block_max(n);
}

// One precision block of the plan's constants (fwav_dct_plan.h's layout), T = double if dbl else float, exactly as
// pocketfft computes them: comp_twiddle's entries of sincos_2pibyn(n), T_dcst23's of sincos_2pibyn(4n), long-double
// literals rounded once to T.
void dct_plan_constants(const DctPlan& p, bool dbl, double* out) {
  auto r = [&](long double v) { return dbl ? (double)v : (double)(float)v; };
  const int n = p.n;
  out[0] = r(1.0L / std::sqrt((long double)(2 * n)));
  out[1] = r(1.414213562373095048801688724209698L);
  out[2] = r(0.8660254037844386467637231707529362L);
  out[3] = r(0.3090169943749474241022934171828191L);
  out[4] = r(0.9510565162951535721164393333793821L);
  out[5] = r(-0.8090169943749474241022934171828191L);
  out[6] = r(0.5877852522924731291687059546390728L);
  out[7] = 0.0;
  const SinCos2PiByN s4(4 * (size_t)n), s1((size_t)n);
  for (int i = 0; i < n; ++i) out[kPlanConst + i] = r(s4[i + 1].first);
  double* mem = out + kPlanConst + n;
  for (int i = kPlanConst + n; i < p.pb; ++i) out[i] = 0.0;  // an even ido leaves one slot per twiddle row unused
  for (int k = 0, l1 = 1; k < p.nf; ++k) {
    const int ip = p.ip[k], ido = n / (l1 * ip);
    if (k < p.nf - 1) {
      double* tw = mem + p.tw[k];
      for (int j = 1; j < ip; ++j)
        for (int i = 1; i <= (ido - 1) / 2; ++i) {
          tw[(j - 1) * (ido - 1) + 2 * i - 2] = r(s1[(size_t)j * l1 * i].first);
          tw[(j - 1) * (ido - 1) + 2 * i - 1] = r(s1[(size_t)j * l1 * i].second);
        }
    }
    if (ip > 5) {
      double* tws = mem + p.tws[k];
      tws[0] = 1.0;
      tws[1] = 0.0;
      for (int i = 2, ic = 2 * ip - 2; i <= ic; i += 2, ic -= 2) {
        const auto t = s1[(size_t)(i / 2) * (n / ip)];
        tws[i] = r(t.first);
        tws[i + 1] = r(t.second);
        tws[ic] = r(t.first);
        tws[ic + 1] = r(-t.second);
      }
    }
    l1 *= ip;
  }
}

template <class T>
FWAV_HD PlanK<T> plan_view(const DctPlan& p, const T* block) {
  PlanK<T> v;
  v.n = p.n;
  v.nf = p.nf;
  for (int k = 0; k < kPlanMaxFact; ++k) {
    v.ip[k] = p.ip[k];
    v.tw[k] = p.tw[k];
    v.tws[k] = p.tws[k];
  }
  v.k = block;
  return v;
}

constexpr int kExactThreads = 64;

// One thread per domain row, as k_embed's exact branch, for a runtime n ≤ NMAX.  The two DCT work buffers of a thread
// are columns of s_buf (element i of lane t at i·64 + t: conflict-free, nothing indexed at run time lives in
// registers or scratch); the f32 head and then the f64 head run in the same storage.  The plan arrives as a kernel
// argument, both precisions' constants and w are staged in LDS (uniform reads broadcast).  NMAX = 64 takes 68,640 B
// of LDS: two workgroups per CU.
template <int NMAX>
__global__ __launch_bounds__(kExactThreads) void k_embed_exact(const float* __restrict__ src, int64_t nd, int64_t a,
                                                               int64_t b, const double* __restrict__ tab,
                                                               const DctPlan plan, float* __restrict__ pool_out,
                                                               float* __restrict__ emb, _Float16* __restrict__ emb16) {
  __shared__ double s_buf[2 * NMAX * kExactThreads];
  __shared__ double s_kd[plan_block_max(NMAX)];
  __shared__ double s_w[NMAX];
  __shared__ float s_kf[plan_block_max(NMAX)];
  const int tid = threadIdx.x;
  const int n = plan.n;
  for (int i = tid; i < plan.pb; i += kExactThreads) {
    s_kf[i] = (float)tab[kPlanHead + n + i];
    s_kd[i] = tab[kPlanHead + n + plan.pb + i];
  }
  for (int i = tid; i < n; i += kExactThreads) s_w[i] = tab[kPlanHead + i];
  __syncthreads();
  const int64_t d = (int64_t)blockIdx.x * kExactThreads + tid;
  if (d >= nd) return;
  const float* xs = src + d * a;
  const int take = n - 1 < 8 ? n - 1 : 8;
  const int tk = n < 8 ? n : 8;
  float e[8], tf[8];
  {
    // tonal head: f32 pocketfft DCT, · w in f64 → f32, sdot-order norm, f32 divide
    float* fb = reinterpret_cast<float*>(s_buf);
    const Col<float, kExactThreads> c{fb + tid}, ch{fb + NMAX * kExactThreads + tid};
    for (int i = 0; i < n; ++i) {
      const float v = xs[i * b];
      if (pool_out) pool_out[d * n + i] = v;
      c[i] = v;
    }
    dct2_ortho_plan<float>(c, ch, plan_view<float>(plan, s_kf));
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = j + 1 < n ? j + 1 : 0;
      e[j] = j < take ? (float)((double)c[i] * s_w[i]) : 0.0f;
    }
    double acc = 0.0;  // sdot: f32 products, f64 sum in index order, f32 result
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = acc + (double)(e[j] * e[j]);
    const float nrm = sqrtf((float)acc);
    if (nrm > 1e-8f) {
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = e[j] / nrm;
    }
  }
  __atomic_signal_fence(__ATOMIC_SEQ_CST);  // the f64 head reuses the f32 head's storage: keep the compiler's order
  {
    // transient head: f64 pocketfft DCT of the weighted first difference, ddot fma-chain norm, divide, → f32
    const Col<double, kExactThreads> c{s_buf + tid}, ch{s_buf + NMAX * kExactThreads + tid};
    float xp = xs[0];
    for (int i = 0; i < n; ++i) {
      const float xi = xs[i * b];
      c[i] = (double)(i == 0 ? xi - xi : xi - xp) * s_w[i];
      xp = xi;
    }
    dct2_ortho_plan<double>(c, ch, plan_view<double>(plan, s_kd));
    double s2 = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < tk) s2 = __builtin_fma(c[j], c[j], s2);
    const double nrmd = sqrt(s2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      double v = j < tk ? c[j] : 0.0;
      if (nrmd > 1e-8) v = v / nrmd;
      tf[j] = (float)v;
    }
  }
  // concatenation [tonal 8 | transient tk] then zero pad to 16, as k_embed
  float out[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = e[j];
#pragma unroll
  for (int j = 0; j < 8; ++j) out[8 + j] = j < tk ? tf[j] : 0.0f;
  float4* o4 = reinterpret_cast<float4*>(emb + d * 16);
#pragma unroll
  for (int j = 0; j < 4; ++j) o4[j] = make_float4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
  if (emb16 != nullptr) store_emb16(emb16, nd, d, out);
}

template <int NMAX>
static void launch_embed_exact(const float* src, int64_t nd, int64_t a, int64_t b, const double* tab,
                               const DctPlan& plan, float* pool_out, float* emb, _Float16* emb16, hipStream_t st) {
  k_embed_exact<NMAX><<<cdiv(nd, kExactThreads), kExactThreads, 0, st>>>(src, nd, a, b, tab, plan, pool_out, emb,
                                                                         emb16);
}

// The pool stage of every fwav_pool_embed* entry point: block means (S in the workspace) when the block length is a
// multiple of the step, else every pool element on its own.  Returns where the embedding kernel reads row d, element k
// (src[d·a + k·b]) and whether it still has to write the pool rows.
struct PoolSrc {
  const float* src;
  int64_t a, b;
  float* pool_out;
};
static PoolSrc pool_stage(const float* sig, int64_t nd, int rs, int step, int bl, float* pool, float* S,
                          hipStream_t st) {
  if (bl % step == 0) {
    const int64_t m = bl / step;
    const int64_t ns = (nd - 1) + (int64_t)(rs - 1) * m + 1;
    const int64_t g = cdiv(ns, kPoolThreads);
    if (bl == 256) k_block_means<256><<<g, kPoolThreads, 0, st>>>(sig, ns, step, bl, S);
    else if (bl == 128) k_block_means<128><<<g, kPoolThreads, 0, st>>>(sig, ns, step, bl, S);
    else k_block_means<0><<<g, kPoolThreads, 0, st>>>(sig, ns, step, bl, S);
    return PoolSrc{S, 1, m, pool};
  }
  k_domain_pool<<<cdiv(nd * rs, kPoolThreads), kPoolThreads, 0, st>>>(sig, nd, rs, step, bl, pool);
  return PoolSrc{pool, rs, 1, nullptr};
}

// The embedding stage of fwav_pool_embed and fwav_embed_rows (emb_dim 16): the two-part fp16 table's padded tail
// zeroed, then k_embed on nd rows read as src[d·a + k·b] — pool rows from pool_stage, or a caller's rows (a = rs,
// b = 1, no pool_out).
static void zero_emb16_tail(_Float16* e16, int64_t nd, hipStream_t st) {
  if (e16 == nullptr || (nd & 255) == 0) return;
  // the padded tail of the last chunk (both halves of both tables)
  const int64_t c = nd >> 8, j0 = nd & 255;
  const int64_t n16 = ((nd + 255) >> 8) * 256 * 16;
  for (int tb = 0; tb < 2; ++tb)
    for (int hh = 0; hh < 2; ++hh)
      (void)hipMemsetAsync(e16 + tb * n16 + ((c * 2 + hh) * 256 + j0) * 8, 0,
                           (size_t)(256 - j0) * 8 * sizeof(_Float16), st);
}
static void embed_stage(const float* src, int64_t nd, int rs, int64_t a, int64_t b, const double* tab, float* pool_out,
                        float* emb, _Float16* e16, hipStream_t st) {
  zero_emb16_tail(e16, nd, st);
  switch (rs) {
    case 4: launch_embed<4>(src, nd, rs, a, b, tab, pool_out, emb, e16, st); break;
    case 8: launch_embed<8>(src, nd, rs, a, b, tab, pool_out, emb, e16, st); break;
    case 16: launch_embed<16>(src, nd, rs, a, b, tab, pool_out, emb, e16, st); break;
    default: launch_embed<0>(src, nd, rs, a, b, tab, pool_out, emb, e16, st); break;
  }
}
// ... and of fwav_pool_embed_exact and fwav_embed_rows_exact (k_embed_exact, range sizes with a pocketfft plan)
static void embed_stage_exact(const float* src, int64_t nd, int rs, int64_t a, int64_t b, const double* tab,
                              const DctPlan& plan, float* pool_out, float* emb, _Float16* e16, hipStream_t st) {
  zero_emb16_tail(e16, nd, st);
  if (rs <= 16) launch_embed_exact<16>(src, nd, a, b, tab, plan, pool_out, emb, e16, st);
  else if (rs <= 24) launch_embed_exact<24>(src, nd, a, b, tab, plan, pool_out, emb, e16, st);
  else if (rs <= 32) launch_embed_exact<32>(src, nd, a, b, tab, plan, pool_out, emb, e16, st);
  else if (rs <= 48) launch_embed_exact<48>(src, nd, a, b, tab, plan, pool_out, emb, e16, st);
  else launch_embed_exact<64>(src, nd, a, b, tab, plan, pool_out, emb, e16, st);
}

// Domain-embedding rows (emb_dim = 16·NS) → the wide search's fp16 table (store_embh).
template <int NS>
__global__ __launch_bounds__(kPoolThreads) void k_embh(const float* __restrict__ emb, int64_t nd,
                                                       _Float16* __restrict__ embh) {
  const int64_t d = (int64_t)blockIdx.x * kPoolThreads + threadIdx.x;
  if (d >= nd) return;
  float out[16 * NS];
  const float4* p = reinterpret_cast<const float4*>(emb + d * 16 * NS);
#pragma unroll
  for (int j = 0; j < 4 * NS; ++j) {
    const float4 v = p[j];
    out[4 * j] = v.x; out[4 * j + 1] = v.y; out[4 * j + 2] = v.z; out[4 * j + 3] = v.w;
  }
  store_embh<NS>(embh, d, out);
}

// Zeroes rows nd … of the last chunk of the wide search's table (every step and half), so that they score 0.
static void zero_embh_tail(_Float16* embh, int64_t nd, int dim, hipStream_t st) {
  if ((nd & 255) == 0) return;
  const int64_t c = nd >> 8, j0 = nd & 255;
  for (int sh = 0; sh < dim / 8; ++sh)
    (void)hipMemsetAsync(embh + ((c * (dim / 8) + sh) * 256 + j0) * 8, 0, (size_t)(256 - j0) * 8 * sizeof(_Float16), st);
}

// fwav_embed_tables' content for heads of H coefficients: the f64 matrices (tonal H rows, transient H rows of rs;
// zero rows past the coefficients a range size has) and, for rs = 4, 8, 16, pocketfft's constants in both precisions.
static void embed_tables_fill(int rs, int H, double* tab) {
  const double pi = 3.14159265358979323846;
  const int n = rs;
  auto w = [&](int i) { return n == 1 ? 1.0 : 1.0 + (double)i / (double)(n - 1); };  // np.linspace(1, 2, n)
  auto c = [&](int k, int i) {
    double f = k == 0 ? std::sqrt(1.0 / n) : std::sqrt(2.0 / n);
    return f * std::cos(pi * k * (2.0 * i + 1.0) / (2.0 * n));
  };
  const int take = n - 1 < H ? n - 1 : H;
  const int tk = n < H ? n : H;
  for (int j = 0; j < H; ++j)
    for (int i = 0; i < n; ++i) tab[j * n + i] = j < take ? c(j + 1, i) * w(j + 1) : 0.0;
  for (int j = 0; j < H; ++j)
    for (int i = 0; i < n; ++i) tab[H * n + j * n + i] = j < tk ? c(j, i) * w(i) : 0.0;
  if (rs == 4 || rs == 8 || rs == 16) {
    dct_constants(rs, false, tab + 2 * H * rs);
    dct_constants(rs, true, tab + 2 * H * rs + dct_block(rs));
  }
}

static bool exact_routes_fixed(int rs) { return rs == 4 || rs == 8 || rs == 16; }

}  // namespace fwav

using namespace fwav;

extern "C" {

size_t fwav_emb16_elems(int64_t nd) { return (size_t)(2 * ((nd + 255) / 256) * 256 * 16); }

// Host-side f64 tables for fwav_pool_embed: tab[fwav_embed_tables_size(rs)] = the matrices (tonal 8 rows, transient 8
// rows of rs) and, for rs = 4, 8, 16, pocketfft's constants in float32 then float64 (DctK layout, dct_constants).
size_t fwav_embed_tables_size(int rs) {
  return (size_t)16 * rs + ((rs == 4 || rs == 8 || rs == 16) ? 2 * (size_t)dct_block(rs) : 0);
}

int fwav_embed_tables(int rs, double* tab) {
  FWAV_CHECK_ARG(rs >= 1 && rs <= kMaxPairwise && tab, FWAV_ERR_ARG, "fwav_embed_tables: bad args");
  embed_tables_fill(rs, 8, tab);
  return FWAV_OK;
}

// Test hook (host): scipy.fftpack.dct(x, norm='ortho') of n = 4, 8, 16 doubles (dbl = 1) or floats (dbl = 0, passed
// and returned as doubles) through fwav_dct.h — the code the embedding kernel runs, instantiated on the host.
int fwav_debug_dct2(int n, int dbl, const double* x, double* out) {
  FWAV_CHECK_ARG((n == 4 || n == 8 || n == 16) && x && out, FWAV_ERR_ARG, "fwav_debug_dct2: n must be 4, 8 or 16");
  double tab[2 * (2 * 16 + 11)];
  dct_constants(n, dbl != 0, tab);
  auto run = [&](auto tag, auto nn) {
    using T = decltype(tag);
    constexpr int N = decltype(nn)::value;
    DctK<T, N> k;
    dct_load(k, tab);
    T c[N];
    for (int i = 0; i < N; ++i) c[i] = (T)x[i];
    dct2_ortho<T, N>(c, k);
    for (int i = 0; i < N; ++i) out[i] = (double)c[i];
  };
  using I4 = std::integral_constant<int, 4>;
  using I8 = std::integral_constant<int, 8>;
  using I16 = std::integral_constant<int, 16>;
  if (dbl) {
    if (n == 4) run(0.0, I4{}); else if (n == 8) run(0.0, I8{}); else run(0.0, I16{});
  } else {
    if (n == 4) run(0.0f, I4{}); else if (n == 8) run(0.0f, I8{}); else run(0.0f, I16{});
  }
  return FWAV_OK;
}

// ---- exact embedding (scipy's pocketfft DCTs at any supported range size)
int fwav_embed_exact_supported(int rs) { return exact_routes_fixed(rs) || dct_plan_supported(rs) ? 1 : 0; }

// Host-side table of fwav_pool_embed_exact: for rs = 4, 8, 16 fwav_embed_tables' own (those sizes run k_embed's fixed
// plans); otherwise the plan, w = np.linspace(1, 2, rs) and both precisions' constants (fwav_dct_plan.h's layout).
size_t fwav_embed_tables_exact_size(int rs) {
  if (exact_routes_fixed(rs)) return fwav_embed_tables_size(rs);
  DctPlan p;
  if (!dct_plan_build(rs, p)) return 0;
  return (size_t)kPlanHead + rs + 2 * (size_t)p.pb;
}

int fwav_embed_tables_exact(int rs, double* tab) {
  FWAV_CHECK_ARG(tab, FWAV_ERR_ARG, "fwav_embed_tables_exact: null table");
  if (exact_routes_fixed(rs)) return fwav_embed_tables(rs, tab);
  DctPlan p;
  FWAV_CHECK_ARG(dct_plan_build(rs, p), FWAV_ERR_ARG,
                 "fwav_embed_tables_exact: range size %d has no exact pocketfft plan (4 ... 49, 50, 54, 56, 60, 63, 64)",
                 rs);
  for (int i = 0; i < kPlanHead; ++i) tab[i] = 0.0;
  tab[0] = rs;
  tab[1] = p.nf;
  for (int k = 0; k < kPlanMaxFact; ++k) {
    tab[2 + 3 * k] = p.ip[k];
    tab[3 + 3 * k] = p.tw[k];
    tab[4 + 3 * k] = p.tws[k];
  }
  tab[14] = p.pb;
  const double step = 1.0 / (double)(rs - 1);
  for (int i = 0; i < rs; ++i) tab[kPlanHead + i] = i == rs - 1 ? 2.0 : (double)i * step + 1.0;
  dct_plan_constants(p, false, tab + kPlanHead + rs);
  dct_plan_constants(p, true, tab + kPlanHead + rs + p.pb);
  return FWAV_OK;
}

// Test hook (host): scipy.fftpack.dct(x, norm='ortho') of n doubles (dbl = 1) or floats (dbl = 0, passed and returned
// as doubles) through fwav_dct_plan.h — the code k_embed_exact runs, instantiated on the host with stride-1 buffers.
int fwav_debug_dct2_plan(int n, int dbl, const double* x, double* out) {
  FWAV_CHECK_ARG(x && out, FWAV_ERR_ARG, "fwav_debug_dct2_plan: null array");
  DctPlan p;
  FWAV_CHECK_ARG(dct_plan_build(n, p), FWAV_ERR_ARG, "fwav_debug_dct2_plan: n = %d has no exact pocketfft plan", n);
  double kd[plan_block_max(kPlanMaxN)];
  dct_plan_constants(p, dbl != 0, kd);
  auto run = [&](auto tag) {
    using T = decltype(tag);
    T k[plan_block_max(kPlanMaxN)], c[kPlanMaxN], ch[kPlanMaxN];
    for (int i = 0; i < p.pb; ++i) k[i] = (T)kd[i];
    for (int i = 0; i < n; ++i) c[i] = (T)x[i];
    dct2_ortho_plan<T>(Col<T, 1>{c}, Col<T, 1>{ch}, plan_view<T>(p, k));
    for (int i = 0; i < n; ++i) out[i] = (double)c[i];
  };
  if (dbl) run(0.0); else run(0.0f);
  return FWAV_OK;
}

size_t fwav_pool_workspace_size(int64_t n, int tile, int rs, int step) {
  const int bl = tile / rs;
  if (n < tile || bl % step != 0) return 0;
  const int64_t nd = (n - tile) / step + 1;
  const int64_t ns = (nd - 1) + (int64_t)(rs - 1) * (bl / step) + 1;
  return (size_t)ns * sizeof(float);
}

// Domain pool + embedding.  pool: f32[nd*rs], emb: f32[nd*16], tab: device copy of fwav_embed_tables(rs).
// emb16 (optional): fp16 high and low parts in the tiled layout the similarity search streams,
// f16[fwav_emb16_elems(nd)] = 2 tables of ceil(nd/256)*256*16; rows past nd are zeroed here.
// fp16 search tables (f16[fwav_emb16_elems(nd)]) of embedding rows emb f32[nd*16], as fwav_pool_embed writes them.
int fwav_emb16_from_emb(const float* emb, int64_t nd, void* emb16, void* stream) {
  FWAV_CHECK_ARG(emb && emb16 && nd > 0, FWAV_ERR_ARG, "fwav_emb16_from_emb: bad args");
  hipStream_t st = (hipStream_t)stream;
  _Float16* e16 = (_Float16*)emb16;
  zero_emb16_tail(e16, nd, st);
  k_emb16<<<cdiv(nd, kPoolThreads), kPoolThreads, 0, st>>>(emb, nd, e16);
  FWAV_LAUNCH_CHECK("fwav_emb16_from_emb");
  return FWAV_OK;
}

int fwav_pool_embed(const float* sig, int64_t n, int tile, int rs, int step, const double* tab, float* pool,
                    float* emb, void* emb16, void* workspace, size_t ws_bytes, void* stream) {
  FWAV_CHECK_ARG(sig && pool && emb && tab && tile > 0 && rs > 0 && step > 0, FWAV_ERR_ARG,
                 "fwav_pool_embed: bad args");
  FWAV_CHECK_ARG(n >= tile, FWAV_ERR_SHAPE, "fwav_pool_embed: n < tile");
  const int bl = tile / rs;
  FWAV_CHECK_ARG(bl >= 1 && bl <= kMaxPairwise && rs <= kMaxPairwise, FWAV_ERR_SHAPE,
                 "fwav_pool_embed: block length out of range");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nd = (n - tile) / step + 1;
  FWAV_CHECK_ARG(bl % step != 0 || (ws_bytes >= fwav_pool_workspace_size(n, tile, rs, step) && workspace),
                 FWAV_ERR_WORKSPACE, "fwav_pool_embed: workspace too small");
  const PoolSrc ps = pool_stage(sig, nd, rs, step, bl, pool, (float*)workspace, st);
  const float* src = ps.src;
  const int64_t a = ps.a, b = ps.b;
  float* pool_out = ps.pool_out;
  embed_stage(src, nd, rs, a, b, tab, pool_out, emb, (_Float16*)emb16, st);
  FWAV_LAUNCH_CHECK("fwav_pool_embed");
  return FWAV_OK;
}

// fwav_pool_embed with the exact embedding kernel: the same pool stage on both source layouts, then k_embed_exact.
// tab: device copy of fwav_embed_tables_exact(rs).  rs = 4, 8, 16: fwav_pool_embed itself (already exact).
int fwav_pool_embed_exact(const float* sig, int64_t n, int tile, int rs, int step, const double* tab, float* pool,
                          float* emb, void* emb16, void* workspace, size_t ws_bytes, void* stream) {
  if (exact_routes_fixed(rs))
    return fwav_pool_embed(sig, n, tile, rs, step, tab, pool, emb, emb16, workspace, ws_bytes, stream);
  FWAV_CHECK_ARG(sig && pool && emb && tab && tile > 0 && rs > 0 && step > 0, FWAV_ERR_ARG,
                 "fwav_pool_embed_exact: bad args");
  DctPlan plan;
  FWAV_CHECK_ARG(dct_plan_build(rs, plan), FWAV_ERR_ARG,
                 "fwav_pool_embed_exact: range size %d has no exact pocketfft plan (fwav_embed_exact_supported)", rs);
  FWAV_CHECK_ARG(n >= tile, FWAV_ERR_SHAPE, "fwav_pool_embed_exact: n < tile");
  const int bl = tile / rs;
  FWAV_CHECK_ARG(bl >= 1 && bl <= kMaxPairwise, FWAV_ERR_SHAPE, "fwav_pool_embed_exact: block length out of range");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nd = (n - tile) / step + 1;
  FWAV_CHECK_ARG(bl % step != 0 || (ws_bytes >= fwav_pool_workspace_size(n, tile, rs, step) && workspace),
                 FWAV_ERR_WORKSPACE, "fwav_pool_embed_exact: workspace too small");
  const PoolSrc ps = pool_stage(sig, nd, rs, step, bl, pool, (float*)workspace, st);
  const float* src = ps.src;
  const int64_t a = ps.a, b = ps.b;
  float* pool_out = ps.pool_out;
  embed_stage_exact(src, nd, rs, a, b, tab, plan, pool_out, emb, (_Float16*)emb16, st);
  FWAV_LAUNCH_CHECK("fwav_pool_embed_exact");
  return FWAV_OK;
}

// ---- embeddings of caller rows (compress_audio(query="range"): the ranges' own embeddings, fractal.py:337-351)
// fwav_pool_embed's embedding half on n rows of rs floats: the same kernel (k_embed) reading rows[d·rs + k].
int fwav_embed_rows(const float* rows, int64_t n, int rs, const double* tab, float* emb, void* emb16, void* stream) {
  FWAV_CHECK_ARG(rows && emb && tab && n >= 0 && rs >= 1, FWAV_ERR_ARG, "fwav_embed_rows: bad args");
  FWAV_CHECK_ARG(rs <= kMaxPairwise, FWAV_ERR_SHAPE, "fwav_embed_rows: range size out of range");
  if (n == 0) return FWAV_OK;
  embed_stage(rows, n, rs, rs, 1, tab, nullptr, emb, (_Float16*)emb16, (hipStream_t)stream);
  FWAV_LAUNCH_CHECK("fwav_embed_rows");
  return FWAV_OK;
}

// fwav_pool_embed_exact's embedding half on n rows of rs floats (k_embed_exact; rs = 4, 8, 16: fwav_embed_rows).
int fwav_embed_rows_exact(const float* rows, int64_t n, int rs, const double* tab, float* emb, void* emb16,
                          void* stream) {
  if (exact_routes_fixed(rs)) return fwav_embed_rows(rows, n, rs, tab, emb, emb16, stream);
  FWAV_CHECK_ARG(rows && emb && tab && n >= 0 && rs >= 1, FWAV_ERR_ARG, "fwav_embed_rows_exact: bad args");
  DctPlan plan;
  FWAV_CHECK_ARG(dct_plan_build(rs, plan), FWAV_ERR_ARG,
                 "fwav_embed_rows_exact: range size %d has no exact pocketfft plan (fwav_embed_exact_supported)", rs);
  if (n == 0) return FWAV_OK;
  embed_stage_exact(rows, n, rs, rs, 1, tab, plan, nullptr, emb, (_Float16*)emb16, (hipStream_t)stream);
  FWAV_LAUNCH_CHECK("fwav_embed_rows_exact");
  return FWAV_OK;
}

// ---- emb_dim = 32 (heads of 16 coefficients; the wide search's table, fwav_topk_wide.hip)
size_t fwav_embh_elems(int64_t nd, int emb_dim) {
  return emb_dim == 32 && nd > 0 ? (size_t)(((nd + 255) / 256) * 256 * emb_dim) : 0;
}

int fwav_embh_from_emb(const float* emb, int64_t nd, int emb_dim, void* embh, void* stream) {
  FWAV_CHECK_ARG(emb_dim == 32, FWAV_ERR_ARG, "fwav_embh_from_emb: emb_dim %d (only 32 is supported)", emb_dim);
  FWAV_CHECK_ARG(emb && embh && nd > 0, FWAV_ERR_ARG, "fwav_embh_from_emb: bad args");
  hipStream_t st = (hipStream_t)stream;
  zero_embh_tail((_Float16*)embh, nd, emb_dim, st);
  k_embh<2><<<cdiv(nd, kPoolThreads), kPoolThreads, 0, st>>>(emb, nd, (_Float16*)embh);
  FWAV_LAUNCH_CHECK("fwav_embh_from_emb");
  return FWAV_OK;
}

size_t fwav_embed_tables_dim_size(int rs, int emb_dim) {
  if (emb_dim != 32 || rs < 1) return 0;
  return (size_t)emb_dim * rs + (exact_routes_fixed(rs) ? 2 * (size_t)dct_block(rs) : 0);
}

int fwav_embed_tables_dim(int rs, int emb_dim, double* tab) {
  FWAV_CHECK_ARG(emb_dim == 32, FWAV_ERR_ARG, "fwav_embed_tables_dim: emb_dim %d (only 32 is supported)", emb_dim);
  FWAV_CHECK_ARG(rs >= 1 && rs <= kMaxPairwise && tab, FWAV_ERR_ARG, "fwav_embed_tables_dim: bad args");
  embed_tables_fill(rs, emb_dim / 2, tab);
  return FWAV_OK;
}

// fwav_pool_embed with rows of emb_dim = 32 columns: [tonal: min(16, rs − 1) values, zero-padded to 16][transient:
// min(16, rs) values][zeros to 32].  tab: device copy of fwav_embed_tables_dim(rs, 32); embh (optional):
// f16[fwav_embh_elems(nd, 32)], rows past nd zeroed here.
int fwav_pool_embed_dim(const float* sig, int64_t n, int tile, int rs, int step, int emb_dim, const double* tab,
                        float* pool, float* emb, void* embh, void* workspace, size_t ws_bytes, void* stream) {
  FWAV_CHECK_ARG(emb_dim == 32, FWAV_ERR_ARG, "fwav_pool_embed_dim: emb_dim %d (only 32 is supported)", emb_dim);
  FWAV_CHECK_ARG(sig && pool && emb && tab && tile > 0 && rs > 0 && step > 0, FWAV_ERR_ARG,
                 "fwav_pool_embed_dim: bad args");
  FWAV_CHECK_ARG(n >= tile, FWAV_ERR_SHAPE, "fwav_pool_embed_dim: n < tile");
  const int bl = tile / rs;
  FWAV_CHECK_ARG(bl >= 1 && bl <= kMaxPairwise && rs <= kMaxPairwise, FWAV_ERR_SHAPE,
                 "fwav_pool_embed_dim: block length out of range");
  FWAV_CHECK_ARG(bl % step != 0 || (ws_bytes >= fwav_pool_workspace_size(n, tile, rs, step) && workspace),
                 FWAV_ERR_WORKSPACE, "fwav_pool_embed_dim: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nd = (n - tile) / step + 1;
  const PoolSrc ps = pool_stage(sig, nd, rs, step, bl, pool, (float*)workspace, st);
  _Float16* eh = (_Float16*)embh;
  if (eh != nullptr) zero_embh_tail(eh, nd, emb_dim, st);
  switch (rs) {
    case 4: launch_embed<4, 16>(ps.src, nd, rs, ps.a, ps.b, tab, ps.pool_out, emb, eh, st); break;
    case 8: launch_embed<8, 16>(ps.src, nd, rs, ps.a, ps.b, tab, ps.pool_out, emb, eh, st); break;
    case 16: launch_embed<16, 16>(ps.src, nd, rs, ps.a, ps.b, tab, ps.pool_out, emb, eh, st); break;
    default: launch_embed<0, 16>(ps.src, nd, rs, ps.a, ps.b, tab, ps.pool_out, emb, eh, st); break;
  }
  FWAV_LAUNCH_CHECK("fwav_pool_embed_dim");
  return FWAV_OK;
}

}  // extern "C"
