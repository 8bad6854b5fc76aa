// fwav_topk_wide.hip — similarity top-K on embedding rows of 32 columns (compress_audio(emb_dim=32)).
//
// Same contract as fwav_sim_topk (fwav_topk.hip), for rows of D = 16·NS columns: per active query the K domains with
// the largest f32 score emb[d]·emb[q] in the reference's own sgemv order (fwav_common.h sgemv_dim), in (score desc,
// index asc) order, −1-padded when nd < K, exact ties listed in `ties`.  K > 64 goes to fwav_topk_large.hip's select
// on D-wide exact score rows; K ≤ 64 runs k_sim_topk_wide below.
//
// k_sim_topk_wide is k_sim_topk_f32 (fwav_topk.hip) with an fp16 MFMA pre-filter in front of its VALU scores.
// Workgroup = 4 waves × 32 queries.  The fp16 table (fwav_pool_embed.hip store_embh: high parts only, a 256-domain
// chunk is one contiguous 256·D·2-byte block) streams through LDS in increasing index order, one chunk per barrier
// pair, the next chunk prefetched into registers meanwhile.  Per 32-domain tile a wave chains NS
// v_mfma_f32_32x32x16_f16 (A = the tile's rows from LDS, B = its 32 queries' fp16 parts, in registers for the whole
// run): lane l gets the approximate scores a of query l & 31 against 16 of the tile's domains.  Each lane keeps the
// running threshold θ of its query (the K-th exact score of its buffer at the last compaction, −inf before).  Only
// pairs with a > θ − δ are scored exactly: sgemv_dim<D> on the f32 rows, the domain's row read from global memory
// (L2), the query's held in registers; a pair whose exact score beats θ is appended to the query's LDS key buffer,
// and a nearly full buffer is sorted, cut to its top K and θ raised (compact, fwav_topk_keys.h) exactly as the f32
// kernel does.  Domains arrive in index order, so a later domain whose exact score equals θ can never displace an
// earlier one: strict '>' is exact, and such a domain is only noted for the tie list.
//
// δ (kWideDelta) ≥ max |a − s| over unit-or-zero-norm heads, s the exact score (DESIGN.md §3.6 has the derivation):
//   fp16 rounding of both operands, f16(x) = x(1 + ε) + η with |ε| ≤ u = 2⁻¹¹ and |η| ≤ 2⁻²⁵ (subnormals are kept):
//     (2u + u²)·Σ|d_k q_k| + 2⁻²⁵(1 + u)(Σ|d_k| + Σ|q_k|) + 32·2⁻⁵⁰ ≤ 1.95361e-3 + 4.8e-7
//     (Σ|d_k q_k| ≤ 2(1 + 2⁻²¹): two heads of f32 norm ≤ 1 + 2⁻²²; Σ|d_k| ≤ 2·√16 per row);
//   the MFMAs' f32 accumulation of 32 exact products, any order, truncating or rounding: ≤ 32·2⁻²³·2.002 = 7.7e-6;
//   the exact score's own rounding, at most 11 roundings on the path of any term: ≤ 11·2⁻²⁴·2 = 1.4e-6.
// Sum 1.96311e-3; δ = 2.0e-3 leaves 1.9 %.  A pair with s ≥ θ therefore has a ≥ θ − 1.9632e-3 > θ − δ: the
// pre-filter drops no pair that the f32 kernel would keep or note.
#include <algorithm>

#include "fwav_common.h"
#include "fwav_topk_keys.h"
#include "../../include/fwav.h"

namespace fwav {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kWideWaves = 4;
constexpr int kWideQ = 32 * kWideWaves;  // queries per workgroup
constexpr int kWideChunk = 256;          // domains per LDS chunk
constexpr int kWideThreads = 64 * kWideWaves;
constexpr int kWideCap = 128;            // key-buffer entries per query (LDS): K ≤ 64 kept + 32 of slack + one tile
constexpr float kWideDelta = 2.0e-3f;

// fwav_topk_large.hip
size_t large_workspace_bytes(int64_t nd, int64_t max_q);
int launch_topk_large_dim(const float* emb, int64_t nd, int dim, const int32_t* active, const int32_t* n_active,
                          int64_t max_q, int64_t q_offset, int K, int32_t* cand, float* S, SgemvSplit sp,
                          int32_t* ties, hipStream_t st);
int launch_score_rows_dim(const float* emb, int64_t nd, int dim, const int32_t* rows, int64_t n_rows, int64_t q_offset,
                          SgemvSplit sp, float* S, hipStream_t st, const float* qemb);

template <int NS>
constexpr size_t wide_lds_bytes() {
  return (size_t)kWideQ * kWideCap * sizeof(uint64_t) + (size_t)kWideChunk * 16 * NS * sizeof(_Float16) +
         3 * kWideQ * sizeof(int);
}

template <int NS>
__global__ __launch_bounds__(kWideThreads) void k_sim_topk_wide(const _Float16* __restrict__ embh,
                                                                const float* __restrict__ emb, int64_t nd,
                                                                const int32_t* __restrict__ active,
                                                                const int32_t* __restrict__ n_active_p,
                                                                int64_t q_offset, int K, int32_t* __restrict__ cand,
                                                                SgemvSplit sp, int32_t* __restrict__ ties) {
  constexpr int D = 16 * NS;
  constexpr int C = kWideCap;
  constexpr int kVec = kWideChunk * D / 8;      // 16-byte vectors per chunk
  constexpr int kPer = kVec / kWideThreads;     // ... and per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* keys = (uint64_t*)smem;                  // [kWideQ][C]
  u32x4* lda = (u32x4*)(keys + (size_t)kWideQ * C);  // [2·NS column groups of 8][kWideChunk] fragments of 8 halfs
  int* cnt = (int*)(lda + kVec);                     // [kWideQ]
  float* theta = (float*)(cnt + kWideQ);             // [kWideQ]
  // [kWideQ] f2key of the largest θ that a domain of equal score was not kept at (0: none), as k_sim_topk_f32's
  uint32_t* tieb = (uint32_t*)(theta + kWideQ);

  const int n_active = *n_active_p;
  const int qbase = blockIdx.x * kWideQ;
  if (qbase >= n_active) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int col = lane & 31;
  const int h = lane >> 5;
  const int ql = wave * 32 + col;  // local query slot
  const int qi = qbase + ql;
  const int32_t q = qi < n_active ? active[qi] : -1;

  float qf[D];  // the whole query row (sgemv_dim) ...
#pragma unroll
  for (int j = 0; j < D / 4; ++j) {
    const float4 v = q >= 0 ? reinterpret_cast<const float4*>(emb + ((int64_t)q + q_offset) * D)[j]
                            : make_float4(0.f, 0.f, 0.f, 0.f);
    qf[4 * j] = v.x; qf[4 * j + 1] = v.y; qf[4 * j + 2] = v.z; qf[4 * j + 3] = v.w;
  }
  half8 qb[NS];  // ... and its fp16 parts as the MFMA's B fragments: step s, columns 16s + 8h …
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) qb[s][e] = (_Float16)(h ? qf[16 * s + 8 + e] : qf[16 * s + e]);
  float th = q >= 0 ? -INFINITY : INFINITY;  // invalid lanes never pass the filter
  if (tid < kWideQ) {
    cnt[tid] = 0;
    theta[tid] = -INFINITY;
    tieb[tid] = 0;
  }

  const int64_t nchunks = cdiv(nd, kWideChunk);
  u32x4 pf[kPer];  // the next chunk (the table is padded to whole chunks, rows past nd zero)
  auto load_chunk = [&](int64_t c) {
    const u32x4* g = reinterpret_cast<const u32x4*>(embh + c * (int64_t)(kWideChunk * D));
#pragma unroll
    for (int i = 0; i < kPer; ++i) pf[i] = g[i * kWideThreads + tid];
  };
  load_chunk(0);

  for (int64_t c = 0; c < nchunks; ++c) {
    __syncthreads();  // previous chunk fully consumed (and cnt/theta init visible)
#pragma unroll
    for (int i = 0; i < kPer; ++i) lda[i * kWideThreads + tid] = pf[i];
    __syncthreads();
    if (c + 1 < nchunks) load_chunk(c + 1);
    const int64_t dbase = c * kWideChunk;

    // a tile's approximate scores: acc[r] = query col · domain dbase + 32t + 4h + (r&3) + 8(r>>2); tile t + 1's
    // MFMAs are issued before tile t's scores are looked at
    auto tile_scores = [&](int t) {
      floatx16 a32 = floatx16{};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const half8 a = *reinterpret_cast<const half8*>(&lda[(2 * s + h) * kWideChunk + t * 32 + col]);
        a32 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qb[s], a32, 0, 0, 0);
      }
      return a32;
    };
    floatx16 nxt = tile_scores(0);
#pragma unroll 1
    for (int t = 0; t < kWideChunk / 32; ++t) {
      const floatx16 acc = nxt;
      if (t + 1 < kWideChunk / 32) nxt = tile_scores(t + 1);
      const float thd = th - kWideDelta;
      float mx = acc[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[r]);
      if (__ballot(mx > thd) == 0ull) continue;
      // the tile's sgemv kernels (fwav_common.h): all kind 0 unless it holds the tail of a BLAS thread chunk
      const uint32_t tf0 = (uint32_t)(dbase + t * 32);
      const uint32_t tl = (uint32_t)min<int64_t>(dbase + t * 32 + 31, nd - 1);
      const bool plain = sgemv_kind(tl, sp) == 0 && tf0 >= sgemv_chunk_start(tl, sp);
      const int64_t d0 = dbase + t * 32 + 4 * h;  // domain of acc[r] = d0 + (r&3) + 8*(r>>2)
      uint64_t* kq = keys + (size_t)ql * C;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t d = d0 + (r & 3) + 8 * (r >> 2);
        if (acc[r] > thd && d < nd) {
          float dv[D];
#pragma unroll
          for (int j = 0; j < D / 4; ++j) {
            const float4 v = reinterpret_cast<const float4*>(emb + d * D)[j];
            dv[4 * j] = v.x; dv[4 * j + 1] = v.y; dv[4 * j + 2] = v.z; dv[4 * j + 3] = v.w;
          }
          const float s = sgemv_dim<D>([&](int k) { return dv[k]; }, [&](int k) { return qf[k]; },
                                       plain ? 0 : sgemv_kind((uint32_t)d, sp));
          if (s > th) {
            const int slot = atomicAdd(&cnt[ql], 1);
            kq[slot] = make_key(s, (int32_t)d);
          } else if (s == th && th != -INFINITY) {
            atomicMax(&tieb[ql], f2key(th));  // equal to θ but later in index order: not kept
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      uint64_t need = __ballot(lane < 32 && cnt[ql] > C - 32);
      while (need != 0ull) {
        const int l = __builtin_ctzll(need);
        need &= need - 1;
        if ((compact<C>(keys, cnt, theta, wave * 32 + l, K) & 2) && lane == 0)
          atomicMax(&tieb[wave * 32 + l], f2key(theta[wave * 32 + l]));
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (q >= 0) th = theta[ql];
    }
  }

  // final: sort every query of this wave and write its top K
  for (int l = 0; l < 32; ++l) {
    const int qs = wave * 32 + l;
    const int qq = qbase + qs;
    if (qq >= n_active) break;
    const int32_t qid = active[qq];
    const int tf = compact<C>(keys, cnt, theta, qs, K);
    const uint32_t tv = tieb[qs];
    const uint64_t none[1] = {0ull};
    record_tie<1>(ties, qid, tf | (tv != 0u && cnt[qs] >= K && key2f(tv) == theta[qs] ? 2 : 0), none, 0, K);
    const int n = cnt[qs];
    int32_t* out = cand + (int64_t)qid * K;
    for (int e = lane; e < K; e += 64) out[e] = e < n ? key_idx(keys[(size_t)qs * C + e]) : -1;
  }
}

constexpr int kWideMaxDev = 64;

template <int NS>
static int launch_topk_wide(const float* emb, const _Float16* embh, int64_t nd, const int32_t* active,
                            const int32_t* n_active, int64_t max_q, int64_t q_offset, int K, int32_t* cand,
                            SgemvSplit sp, int32_t* ties, hipStream_t st) {
  constexpr size_t lds = wide_lds_bytes<NS>();
  static_assert(lds <= 160 * 1024, "one workgroup's buffers fit a CU's LDS");
  static bool attr[kWideMaxDev] = {false};  // a function attribute is set per device
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= kWideMaxDev) dev = 0;
  if (!attr[dev]) {
    (void)hipFuncSetAttribute((const void*)k_sim_topk_wide<NS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr[dev] = true;
  }
  k_sim_topk_wide<NS><<<cdiv(max_q, kWideQ), kWideThreads, lds, st>>>(embh, emb, nd, active, n_active, q_offset, K,
                                                                      cand, sp, ties);
  FWAV_LAUNCH_CHECK("fwav_sim_topk_dim");
  return FWAV_OK;
}

}  // namespace fwav

using namespace fwav;

extern "C" {

size_t fwav_sim_topk_dim_workspace_size(int64_t max_q, int64_t n_domains, int emb_dim, int k) {
  if (emb_dim != 32 || k <= 64) return 0;  // K ≤ 64: the key buffers live in LDS
  return large_workspace_bytes(n_domains, max_q > 0 ? max_q : 1);
}

int fwav_sim_topk_dim(const float* emb, const void* embh, int64_t nd, int emb_dim, const int32_t* active,
                      const int32_t* n_active, int64_t max_q, int64_t q_offset, int K, int blas_threads,
                      int32_t* cand, int32_t* ties, void* workspace, size_t ws_bytes, void* stream) {
  FWAV_CHECK_ARG(emb_dim == 32, FWAV_ERR_ARG, "fwav_sim_topk_dim: emb_dim %d (only 32 is supported)", emb_dim);
  FWAV_CHECK_ARG(emb && active && n_active && cand && nd > 0 && max_q >= 0 && q_offset >= 0, FWAV_ERR_ARG,
                 "fwav_sim_topk_dim: bad args");
  FWAV_CHECK_ARG(blas_threads >= 1 && blas_threads <= 4096, FWAV_ERR_ARG,
                 "fwav_sim_topk_dim: blas_threads outside [1, 4096]");
  FWAV_CHECK_ARG(K >= 1 && K <= fwav_topk_max_k(), FWAV_ERR_K, "fwav_sim_topk_dim: K=%d outside [1, %d]", K,
                 fwav_topk_max_k());
  FWAV_CHECK_ARG(nd < (int64_t)0x7fffffff, FWAV_ERR_SHAPE, "fwav_sim_topk_dim: nd too large");
  FWAV_CHECK_ARG(K > 64 || embh, FWAV_ERR_ARG, "fwav_sim_topk_dim: K <= 64 needs the fp16 table (fwav_embh_elems)");
  FWAV_CHECK_ARG(K <= 64 || (workspace && ws_bytes >= fwav_sim_topk_dim_workspace_size(max_q, nd, emb_dim, K)),
                 FWAV_ERR_WORKSPACE, "fwav_sim_topk_dim: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const SgemvSplit sp = make_sgemv_split_dim(nd, blas_threads, emb_dim);
  if (ties != nullptr) (void)hipMemsetAsync(ties, 0, sizeof(int32_t), st);
  if (max_q == 0) return FWAV_OK;
  if (K > 64)
    return launch_topk_large_dim(emb, nd, emb_dim, active, n_active, max_q, q_offset, K, cand, (float*)workspace, sp,
                                 ties, st);
  return launch_topk_wide<2>(emb, (const _Float16*)embh, nd, active, n_active, max_q, q_offset, K, cand, sp, ties, st);
}

int fwav_score_rows_dim(const float* emb, int64_t nd, int emb_dim, const int32_t* rows, int64_t n_rows,
                        int64_t q_offset, int blas_threads, float* scores, void* stream) {
  FWAV_CHECK_ARG(emb_dim == 32, FWAV_ERR_ARG, "fwav_score_rows_dim: emb_dim %d (only 32 is supported)", emb_dim);
  FWAV_CHECK_ARG(emb && rows && scores && nd > 0 && nd < (int64_t)0x7fffffff && n_rows >= 0, FWAV_ERR_ARG,
                 "fwav_score_rows_dim: bad args");
  FWAV_CHECK_ARG(blas_threads >= 1 && blas_threads <= 4096, FWAV_ERR_ARG,
                 "fwav_score_rows_dim: blas_threads outside [1, 4096]");
  if (n_rows == 0) return FWAV_OK;
  return launch_score_rows_dim(emb, nd, emb_dim, rows, n_rows, q_offset,
                               make_sgemv_split_dim(nd, blas_threads, emb_dim), scores, (hipStream_t)stream, nullptr);
}

// Test hook (host, no device): one (domain row, query row) pair of emb_dim = 32 floats through the search's own
// helpers, compiled for the host: out[0] = the exact score (sgemv_dim, kernel `kind` 0, 1 or 2), out[1] = the
// pre-filter's approximate score (fp16 parts rounded as store_embh rounds them, products exact in f32, summed in f32
// in index order), out[2] = δ, the bound on their difference that the pre-filter relies on.
int fwav_debug_score_dim(const float* d, const float* q, int emb_dim, int kind, float* out) {
  FWAV_CHECK_ARG(emb_dim == 32, FWAV_ERR_ARG, "fwav_debug_score_dim: emb_dim %d (only 32 is supported)", emb_dim);
  FWAV_CHECK_ARG(d && q && out && kind >= 0 && kind <= 2, FWAV_ERR_ARG, "fwav_debug_score_dim: bad args");
  out[0] = sgemv_dim<32>([&](int k) { return d[k]; }, [&](int k) { return q[k]; }, kind);
  float a = 0.0f;
  for (int k = 0; k < 32; ++k) a = a + (float)(_Float16)d[k] * (float)(_Float16)q[k];
  out[1] = a;
  out[2] = kWideDelta;
  return FWAV_OK;
}

}  // extern "C"
