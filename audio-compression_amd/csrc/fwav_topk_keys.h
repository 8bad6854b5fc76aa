// fwav_topk_keys.h — the (score, index) keys of the similarity searches and the wave-wide helpers on sorted key
// lists that fwav_topk.hip's kernels and fwav_topk_wide.hip share: the descending bitonic sort, the exact-tie flags,
// the tie-list records (fwav_sim_topk `ties`) and the f32 kernels' buffer compaction.
#pragma once

#include "fwav_common.h"

namespace fwav {

__device__ __forceinline__ uint64_t make_key(float s, int32_t idx) {
  return ((uint64_t)f2key(s) << 32) | (uint64_t)(~(uint32_t)idx);
}
__device__ __forceinline__ int32_t key_idx(uint64_t k) { return (int32_t)(~(uint32_t)(k & 0xffffffffu)); }
__device__ __forceinline__ float key_score(uint64_t k) { return key2f((uint32_t)(k >> 32)); }

// Descending bitonic sort of E*64 keys held as v[j] = element j*64 + lane.
template <int E>
__device__ __forceinline__ void wave_sort_desc(uint64_t (&v)[E]) {
  const int lane = threadIdx.x & 63;
  constexpr int N = E * 64;
#pragma unroll
  for (int size = 2; size <= N; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (stride >= 64) {
        const int js = stride >> 6;
#pragma unroll
        for (int j = 0; j < E; ++j) {
          if ((j & js) == 0) {
            const int jp = j | js;
            const int e = j * 64 + lane;
            const bool desc = (e & size) == 0;
            uint64_t a = v[j], b = v[jp];
            bool sw = desc ? (a < b) : (a > b);
            v[j] = sw ? b : a;
            v[jp] = sw ? a : b;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < E; ++j) {
          const int e = j * 64 + lane;
          uint64_t o = __shfl_xor(v[j], stride);
          const bool lower = (lane & stride) == 0;
          const bool desc = (e & size) == 0;
          uint64_t mx = v[j] > o ? v[j] : o;
          uint64_t mn = v[j] > o ? o : v[j];
          v[j] = (lower == desc) ? mx : mn;
        }
      }
    }
  }
}

// Exactly equal scores among the first K + 1 entries of a sorted key list (entry e = j·64 + lane, n valid entries):
// bit 0 — two equal scores inside the top K (numpy's argpartition/argsort decide their order), bit 1 — the K-th and
// (K+1)-th scores are equal (numpy decides the set).  Scores compare as floats (−0 == +0).  Whole wave; the result
// is wave-uniform.
template <int E>
__device__ __forceinline__ int tie_flags(const uint64_t (&v)[E], int n, int K) {
  const int lane = threadIdx.x & 63;
  bool in = false, bd = false;
#pragma unroll
  for (int j = 0; j < E; ++j) {
    uint64_t nx = __shfl_down(v[j], 1);
    const uint64_t first_next = __shfl(v[j + 1 < E ? j + 1 : j], 0);
    if (lane == 63) nx = j + 1 < E ? first_next : 0ull;
    const int e = j * 64 + lane;
    if (e + 1 < n && e + 1 <= K && key_score(nx) == key_score(v[j])) {
      if (e + 1 < K) in = true;
      else bd = true;
    }
  }
  return (__ballot(in) != 0ull ? 1 : 0) | (__ballot(bd) != 0ull ? 2 : 0);
}

// Lists query qid for the tie check (fwav_tie_check): ties[0] = count; record i = ties[1 + kTieRec·i ..]:
// [0] = 2·qid + (boundary tie), and for a boundary tie [1] = the number of domains outside the emitted K whose score
// equals the K-th (−1: not known), [2 ..] = those domains.  `v` (sorted, n valid entries) is the query's final band:
// when `group` is set it holds every domain scoring at least the K-th score, so the tie group is complete.  Whole
// wave (wave-uniform arguments).
template <int E>
__device__ __forceinline__ void record_tie(int32_t* ties, int32_t qid, int flags, const uint64_t (&v)[E], int n,
                                           int K, bool group) {
  if (ties == nullptr || flags == 0) return;
  const int lane = threadIdx.x & 63;
  int pos = 0;
  if (lane == 0) pos = atomicAdd(ties, 1);
  pos = __shfl(pos, 0);
  int32_t* rec = ties + 1 + (int64_t)kTieRec * pos;
  if (lane == 0) rec[0] = 2 * qid + ((flags >> 1) & 1);
  if (!(flags & 2)) return;
  int total = -1;
  if (group) {
    uint64_t kth = 0;
#pragma unroll
    for (int j = 0; j < E; ++j)
      if (j == ((K - 1) >> 6)) kth = __shfl(v[j], (K - 1) & 63);
    const float S = key_score(kth);
    total = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const int e = j * 64 + lane;
      const bool in = e >= K && e < n && key_score(v[j]) == S;  // sorted: positions K, K + 1, … of the group
      if (in && e - K < kTieRec - 2) rec[2 + e - K] = key_idx(v[j]);
      total += __popcll(__ballot(in));
    }
    if (total > kTieRec - 2) total = -1;
  }
  if (lane == 0) rec[1] = total;
}
template <int E>
__device__ __forceinline__ void record_tie(int32_t* ties, int32_t qid, int flags, const uint64_t (&v)[E], int n,
                                           int K) {
  record_tie<E>(ties, qid, flags, v, n, K, false);
}

// Sort query ql's buffer, keep the top K, update count and θ; returns tie_flags of the sorted buffer (a (K+1)-th
// entry equal to the K-th, about to be dropped, sets bit 1).  Whole wave, uniform ql.
template <int C>
__device__ __forceinline__ int compact(uint64_t* __restrict__ keys, int* __restrict__ cnt, float* __restrict__ theta,
                                       int ql, int K) {
  constexpr int E = C / 64;
  const int lane = threadIdx.x & 63;
  const int n = cnt[ql];
  uint64_t v[E];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = j * 64 + lane;
    v[j] = e < n ? keys[ql * C + e] : 0ull;
  }
  wave_sort_desc<E>(v);
  const int tf = tie_flags<E>(v, n, K);
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = j * 64 + lane;
    if (e < K && e < n) keys[ql * C + e] = v[j];
  }
  // K-th key (position K-1) lives in lane (K-1)&63, slot (K-1)>>6
  const int kl = (K - 1) & 63, kj = (K - 1) >> 6;
  uint64_t kth = 0;
#pragma unroll
  for (int j = 0; j < E; ++j)
    if (j == kj) kth = __shfl(v[j], kl);
  if (lane == 0) {
    cnt[ql] = n < K ? n : K;
    theta[ql] = n >= K ? key_score(kth) : -INFINITY;
  }
  return tf;
}

}  // namespace fwav
