// fwav_topk_f32.h — k_sim_topk_f32, the all-f32 search (emb16 == NULL).
// Part of fwav_topk.hip's translation unit: included there, inside namespace fwav, after the shared constants
// and the headers before it (the file map at the top of fwav_topk.hip); not a header for any other file.
#pragma once

template <int C>
__global__ __launch_bounds__(kTopkThreads) void k_sim_topk_f32(const float* __restrict__ emb, int64_t nd,
                                                               const int32_t* __restrict__ active,
                                                               const int32_t* __restrict__ n_active_p,
                                                               int64_t q_offset, int K, int32_t* __restrict__ cand,
                                                               SgemvSplit sp, int32_t* __restrict__ ties,
                                                               const float* __restrict__ qemb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* keys = (uint64_t*)smem;                            // [kTopkQ][C]
  float* lda = (float*)(keys + (size_t)kTopkQ * C);            // [kChunk][16] (row-major domain rows)
  int* cnt = (int*)(lda + 16 * kChunk);                        // [kTopkQ]
  float* theta = (float*)(cnt + kTopkQ);                       // [kTopkQ]
  // [kTopkQ] f2key of the largest θ that a domain of equal score was not kept at (0: none); the set among equal
  // scores is numpy's choice only if that θ is the final K-th score (θ rises, so earlier ones are superseded)
  uint32_t* tieb = (uint32_t*)(theta + kTopkQ);

  const int n_active = *n_active_p;
  const int qbase = blockIdx.x * kTopkQ;
  if (qbase >= n_active) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int col = lane & 31;
  const int h = lane >> 5;
  const int ql = wave * 32 + col;  // local query slot
  const int qi = qbase + ql;
  const int32_t q = qi < n_active ? active[qi] : -1;

  float qf[16];  // the whole query vector (sgemv16), a row of the query table (emb itself, or the _q entry point's)
#pragma unroll
  for (int k = 0; k < 16; ++k) qf[k] = q >= 0 ? qemb[((int64_t)q + q_offset) * 16 + k] : 0.0f;
  float th = q >= 0 ? -INFINITY : INFINITY;  // invalid lanes never append
  if (tid < kTopkQ) {
    cnt[tid] = 0;
    theta[tid] = -INFINITY;
    tieb[tid] = 0;
  }

  const int64_t nchunks = cdiv(nd, kChunk);
  // prefetch chunk 0: thread t holds the 16 floats of domain chunk*kChunk + t
  float4 pf[4];
  auto load_chunk = [&](int64_t c) {
    const int64_t d = c * kChunk + tid;
    if (d < nd) {
      const float4* p = reinterpret_cast<const float4*>(emb + d * 16);
#pragma unroll
      for (int j = 0; j < 4; ++j) pf[j] = p[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) pf[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  load_chunk(0);

  for (int64_t c = 0; c < nchunks; ++c) {
    __syncthreads();  // previous chunk fully consumed (and cnt/theta init visible)
#pragma unroll
    for (int j = 0; j < 4; ++j) reinterpret_cast<float4*>(lda)[tid * 4 + j] = pf[j];
    __syncthreads();
    if (c + 1 < nchunks) load_chunk(c + 1);
    const int64_t dbase = c * kChunk;

    for (int t = 0; t < kChunk / 32; ++t) {
      // the tile's sgemv kernels (fwav_common.h): all kind 0 unless it holds the tail of a BLAS thread chunk
      const uint32_t tf0 = (uint32_t)(dbase + t * 32);
      const uint32_t tl = (uint32_t)min<int64_t>(dbase + t * 32 + 31, nd - 1);
      const bool plain = sgemv_kind(tl, sp) == 0 && tf0 >= sgemv_chunk_start(tl, sp);
      // the lane's 16 rows of the tile (the row ↔ domain map of the MFMA tiles: d0 + (r&3) + 8*(r>>2))
      floatx16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float4* row = reinterpret_cast<const float4*>(lda) + (t * 32 + 4 * h + (r & 3) + 8 * (r >> 2)) * 4;
        float dv[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 v = row[j];
          dv[4 * j] = v.x; dv[4 * j + 1] = v.y; dv[4 * j + 2] = v.z; dv[4 * j + 3] = v.w;
        }
        const uint32_t dr = (uint32_t)(dbase + t * 32 + 4 * h + (r & 3) + 8 * (r >> 2));
        acc[r] = sgemv16([&](int k) { return dv[k]; }, [&](int k) { return qf[k]; },
                         plain || dr >= (uint32_t)nd ? 0 : sgemv_kind(dr, sp));
      }
      const int64_t d0 = dbase + t * 32 + 4 * h;  // domain of acc[r] = d0 + (r&3) + 8*(r>>2)
      // mask rows past nd
      if (dbase + t * 32 + 32 > nd) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (d0 + (r & 3) + 8 * (r >> 2) >= nd) acc[r] = -INFINITY;
      }
      float mx = acc[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[r]);
      if (__ballot(mx >= th) != 0ull) {
        uint64_t* kq = keys + (size_t)ql * C;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (acc[r] > th) {
            const int slot = atomicAdd(&cnt[ql], 1);
            kq[slot] = make_key(acc[r], (int32_t)(d0 + (r & 3) + 8 * (r >> 2)));
          } else if (acc[r] == th && th != -INFINITY) {
            atomicMax(&tieb[ql], f2key(th));  // equal to θ but later in index order: not kept
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
