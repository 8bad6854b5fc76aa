// fwav_topk_floor.h — the speculative floor's device side (FloorCtl, pilots) and the ordered active list.
// Part of fwav_topk.hip's translation unit: included there, inside namespace fwav, after the shared constants
// and the headers before it (the file map at the top of fwav_topk.hip); not a header for any other file.
#pragma once

// Speculative band floor of a first pass (launch_topk): *key = f2key of a filter floor f on the pass's own score scale
// (s16 or shl; 0 = no floor).  Every query's band limit starts at f, so the pass skips the rise of its limit from the
// seed; a query whose exact K-th score does not clear f + δ (δ ≥ |s16 − s32|, ≥ |shl − s32|: when it does, every exact
// top-K member had a filter score above f, and the result is exact) is listed in miss[0 .. *n_miss) for the
// floor-free second pass instead of being emitted.
// alt_rt / alt_p: the work plan when *key is 0 — the floor did not apply (fewer active queries on the device than the
// floor's minimum, or no finite pilot estimate): the launch then runs the plan of a floor-free pass (its grid covers
// both plans), not the floor's fewer, longer table pieces.
struct FloorCtl {
  const uint32_t* key;
  int32_t* miss;
  int32_t* n_miss;
  int alt_rt = -1, alt_p = 1;
  // the debug library's seed policy (fwav_debug_topk_seeds; read only where kSeedKnob is set: the product's kernels
  // hold the default, 0, as a constant)
  int seeds = 0;
};
// Whole wave: true (and the query listed for the second pass) when the floor may have cut a member of its top K:
// fewer than K band entries, or a K-th exact score (kth: key) not above f + δ.  Every domain whose filter score
// (s16, or shl in HL mode: within δ of s32) beats f was appended, and compactions drop only what the band rule drops;
// a member of the exact top K scores s32 ≥ the exact K-th ≥ the band's K-th > f + δ, so its filter score beat f.
// (Round 5 tested f + 2δ: 8,225 misses per cfg2 call instead of ≈ 2/3 of that.)
__device__ __forceinline__ bool floor_miss(uint32_t fkey, const FloorCtl& fl, int n, int K, uint64_t kth, int32_t qid) {
  if (fkey == 0u) return false;
  const bool miss = !(n >= K && key_score(kth) > key2f(fkey) + kF16Delta);
  if (miss && (threadIdx.x & 63) == 0) fl.miss[atomicAdd(fl.n_miss, 1)] = qid;
  return miss;
}
// Pilot count and floor rank: 256 pilots at rank 5 (the same ≈ 2 % quantile) against
// round 5's 512 at rank 10, same process, identical candidates (profiles/r06/ab_pilots256/): cfg2 14.03 → 14.01
// ms, 165,375 queries 7.83 → 7.87, 82,688 4.55 → 4.48, 41,344 2.85 → 2.80 — the pilots' half of the work (≈ 55 µs)
constexpr int kFloorPilots = 256;  // pilot queries (evenly spaced over the active list)
constexpr int kFloorJ = 8;  // the pilot's estimate: its j-th best score over every (K/j)-th domain ≈ its K-th
constexpr int kFloorRank = 5;  // the floor: the pilots' kFloorRank-th smallest estimate (≈ 2 % quantile)
static_assert(kFloorPilots % 64 == 0 && kFloorPilots <= 1024, "pilots: whole waves, one k_floor_reduce workgroup");
// The pilots' sampled scores: workgroup (g, s) = (blockIdx.x % kPilotGroups, blockIdx.x / kPilotGroups) scores the 64
// pilots g·64 + lane (pilot p at active position p·n/kFloorPilots) against slice s of the sampled domains m·stride
// (1/kFloorSlices of them; its rows staged in LDS 256 at a time, every 4th row to each of the 4 waves), keeps each
// pilot's kFloorJ best per wave, merges the 4 waves' lists in LDS and writes them to scratch[(p·kFloorSlices + s)·kFloorJ
// + i] (pilot-major: k_floor_est reads a pilot's entries contiguously).  The dot products in packed f32 FMAs (a guess
// only: no reference order needed).  Round 5 put 2 pilots on each thread of 1,024 one-dimensional slices and wrote
// 16 MB of pilot-major entries in 32-B pieces 32 KB apart: 136 µs, plus 47 µs in k_floor_est.
constexpr int kPilotGroups = kFloorPilots / 64, kFloorSlices = 128;
typedef float f32x2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void k_floor_pilot(const float* __restrict__ emb, int64_t nd,
                                                     const int32_t* __restrict__ active,
                                                     const int32_t* __restrict__ n_active_p, int64_t q_offset,
                                                     int stride, float* __restrict__ scratch,
                                                     const float* __restrict__ qemb) {
  __shared__ float4 rows[256][4];
  __shared__ float lists[4][64][kFloorJ + 1];
  const int na = *n_active_p;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x % kPilotGroups, sl = blockIdx.x / kPilotGroups;
  const int p = g * 64 + lane;
  const int64_t M = (nd + stride - 1) / stride;
  const int64_t m0 = M * sl / kFloorSlices, m1 = M * (sl + 1) / kFloorSlices;
  f32x2 q[8];
  {
    const int64_t pos = na > 0 ? (int64_t)p * na / kFloorPilots : 0;
    const int64_t row = na > 0 ? (int64_t)active[pos] + q_offset : 0;
    const float4* qp = reinterpret_cast<const float4*>(qemb + row * 16);  // (the query table: emb itself, or the _q one)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 v = qp[k];
      q[2 * k] = f32x2{v.x, v.y};
      q[2 * k + 1] = f32x2{v.z, v.w};
    }
  }
  float top[kFloorJ];
#pragma unroll
  for (int k = 0; k < kFloorJ; ++k) top[k] = -INFINITY;
  for (int64_t mb = m0; mb < m1; mb += 256) {
    const int nr = (int)min<int64_t>(256, m1 - mb);
    __syncthreads();
    if ((int)threadIdx.x < nr) {
      const float4* rp = reinterpret_cast<const float4*>(emb + (mb + threadIdx.x) * stride * 16);
#pragma unroll
      for (int k = 0; k < 4; ++k) rows[threadIdx.x][k] = rp[k];
    }
    __syncthreads();
    for (int r = wave; r < nr; r += 4) {
      f32x2 acc = f32x2{0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float4 d = rows[r][k];
        acc = __builtin_elementwise_fma(q[2 * k], f32x2{d.x, d.y}, acc);
        acc = __builtin_elementwise_fma(q[2 * k + 1], f32x2{d.z, d.w}, acc);
      }
      float x = acc.x + acc.y;
      // sorted insertion into the pilot's top kFloorJ (descending), only for a score that enters it
      if (x > top[kFloorJ - 1]) {
#pragma unroll
        for (int k = 0; k < kFloorJ; ++k) {
          const float hi = fmaxf(top[k], x);
          x = fminf(top[k], x);
          top[k] = hi;
        }
      }
    }
  }
  // the 4 waves' lists of each pilot merged by wave 0
#pragma unroll
  for (int k = 0; k < kFloorJ; ++k) lists[wave][lane][k] = top[k];
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w)
#pragma unroll
      for (int i = 0; i < kFloorJ; ++i) {
        float x = lists[w][lane][i];
        if (x > top[kFloorJ - 1]) {
#pragma unroll
          for (int k = 0; k < kFloorJ; ++k) {
            const float hi = fmaxf(top[k], x);
            x = fminf(top[k], x);
            top[k] = hi;
          }
        }
      }
    float4* out = reinterpret_cast<float4*>(scratch + ((int64_t)p * kFloorSlices + sl) * kFloorJ);
    static_assert(kFloorJ == 8, "two float4 per list");
    out[0] = make_float4(top[0], top[1], top[2], top[3]);
    out[1] = make_float4(top[4], top[5], top[6], top[7]);
  }
}

// One wave per pilot (block = pilot): its j-th best score over all nwg slices (its estimate of its K-th score), to
// est[pilot].  Each lane keeps the top kFloorJ of its slices' entries; then kFloorJ rounds take the wave's largest
// head (the lowest lane holding it pops it).
__global__ __launch_bounds__(64) void k_floor_est(const float* __restrict__ scratch, int nwg, int j,
                                                  float* __restrict__ est) {
  const int lane = threadIdx.x;
  const float* sp = scratch + (int64_t)blockIdx.x * nwg * kFloorJ;
  float top[kFloorJ];
#pragma unroll
  for (int k = 0; k < kFloorJ; ++k) top[k] = -INFINITY;
  for (int e = lane; e < nwg * kFloorJ; e += 64) {
    float x = sp[e];
    if (x > top[kFloorJ - 1]) {
#pragma unroll
      for (int k = 0; k < kFloorJ; ++k) {
        const float hi = fmaxf(top[k], x);
        x = fminf(top[k], x);
        top[k] = hi;
      }
    }
  }
  float got = -INFINITY;
  for (int r = 0; r < j; ++r) {
    float m = top[0];
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    const uint64_t who = __ballot(top[0] == m);
    if (lane == __builtin_ctzll(who)) {
#pragma unroll
      for (int k = 0; k + 1 < kFloorJ; ++k) top[k] = top[k + 1];
      top[kFloorJ - 1] = -INFINITY;
    }
    got = m;
  }
  if (lane == 0) est[blockIdx.x] = got;
}

// The floors from the pilots' estimates: the rank-th smallest (key in f2key order; 0 = no floor: fewer than min_q
// active queries, or no finite estimate) and the smallest − kFloor2Margin for the second pass.
__global__ __launch_bounds__(kFloorPilots) void k_floor_reduce(const float* __restrict__ est_g, int rank,
                                                               const int32_t* __restrict__ n_active_p, int min_q,
                                                               float margin2, uint32_t* __restrict__ floor_key) {
  __shared__ float est[kFloorPilots];
  const int p = threadIdx.x;
  // a NaN estimate ranks as +inf (after every number), so each place 0 … kFloorPilots − 1 has exactly one owner and
  // both keys are always written (a non-finite one as 0: no floor)
  const float e0 = est_g[p];
  const float e = e0 == e0 ? e0 : INFINITY;
  est[p] = e;
  __syncthreads();
  // every pilot's place in (estimate, pilot) order: the one at place rank − 1 is the floor, the one at place 0 the
  // second pass's floor (+ kFloor2Margin)
  int place = 0;
  // (unrolled: the LDS reads are independent — the rolled loop waited on each one, 15 µs for 512 pilots)
#pragma unroll 32
  for (int i = 0; i < kFloorPilots; ++i) {
    const float x = est[i];
    place += (x < e || (x == e && i < p)) ? 1 : 0;
  }
  const int na = *n_active_p;
  const bool ok = na >= min_q && na > 0 && e > -INFINITY && e < INFINITY;
  if (place == rank - 1) floor_key[0] = ok ? f2key(e) : 0u;
  if (place == 0) floor_key[1] = ok ? f2key(e - margin2) : 0u;
}

// ------------------------------------------------------------------------------------ the active list in order
// The search works on its own copy of the active list in ascending query order, whatever order the caller's list is
// in: fwav_prune appends each wave's ranges (ascending) at an atomic offset, so its list is runs of 64 ascending
// ranges in arbitrary run order, and with it the first pass ran 2.30 instead of 1.90 ms for 41,344 queries at the
// same floor (round 6, tools/diag/topk_reps.py AB_RUNS=1 against ascending ranges, profiles/r06/active_order.log;
// the counters of the two runs' work — appends, level-2 pairs — are equal, so it is how the work lands on the
// workgroups, not how much of it there is: with ascending ids the interleaved query groups of every block are spread
// evenly over the queries, with runs in random order each block draws its 16 groups at random and the slowest block
// sets the launch).  A bitmap of the listed ids (duplicates collapse), one count per 8,192 ids, then every block
// writes its ids at its prefix: three small kernels, no host synchronisation.  A list holding an id outside
// [0, max_q) (max_q bounds the list's length, not its ids: a slice of a longer list) is used as given.
constexpr int kOrderWords = 256;  // bitmap words (8,192 query ids) per block of k_order_sum / k_order_emit
__host__ __device__ inline int64_t order_words(int64_t max_q) { return cdiv(max_q > 0 ? max_q : 1, 32); }
// n_order[1] (zeroed with the bitmap): set when an id lies outside [0, max_q)
__global__ __launch_bounds__(256) void k_order_mark(const int32_t* __restrict__ active,
                                                    const int32_t* __restrict__ n_active_p, int64_t max_q,
                                                    uint32_t* __restrict__ bits, int32_t* __restrict__ n_order) {
  const int64_t n = *n_active_p;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int32_t v = active[i];
    if (v >= 0 && v < max_q) atomicOr(bits + (v >> 5), 1u << (v & 31));
    else n_order[1] = 1;
  }
}
// an id outside [0, max_q): the caller's list as given
__global__ __launch_bounds__(256) void k_order_copy(const int32_t* __restrict__ active,
                                                    const int32_t* __restrict__ n_active_p,
                                                    int32_t* __restrict__ order, int32_t* __restrict__ n_order) {
  if (n_order[1] == 0) return;
  const int64_t n = *n_active_p;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) order[i] = active[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) n_order[0] = (int32_t)n;
}
__device__ __forceinline__ int block_sum256(int c, int* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if (lane == 0) red[wave] = c;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void k_order_sum(const uint32_t* __restrict__ bits, int64_t nwords,
                                                   uint32_t* __restrict__ bsum) {
  __shared__ int red[4];
  const int64_t w = (int64_t)blockIdx.x * kOrderWords + threadIdx.x;
  const int t = block_sum256(w < nwords ? __popc(bits[w]) : 0, red);
  if (threadIdx.x == 0) bsum[blockIdx.x] = (uint32_t)t;
}
__global__ __launch_bounds__(256) void k_order_emit(const uint32_t* __restrict__ bits, int64_t nwords,
                                                    const uint32_t* __restrict__ bsum, int32_t* __restrict__ order,
                                                    int32_t* __restrict__ n_order) {
  __shared__ int red[4], wsum[4];
  if (n_order[1] != 0) return;  // k_order_copy writes the list
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int before = 0;  // ids in the blocks before this one
  for (int b = tid; b < (int)blockIdx.x; b += 256) before += (int)bsum[b];
  before = block_sum256(before, red);
  const int64_t w = (int64_t)blockIdx.x * kOrderWords + tid;
  const uint32_t word = w < nwords ? bits[w] : 0u;
  const int c = __popc(word);
  int inc = c;  // inclusive prefix over the wave's lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(inc, off);
    if (lane >= off) inc += y;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int pos = before + inc - c;
  for (int k = 0; k < wave; ++k) pos += wsum[k];
  for (uint32_t m = word; m != 0u; m &= m - 1u) order[pos++] = (int32_t)(w * 32 + __builtin_ctz(m));
  if (blockIdx.x == gridDim.x - 1 && tid == 255) *n_order = pos;
}
// the caller's active list → order[0 .. *n_order), ascending (workspace regions of TopkLayout)
static void order_active(const int32_t* active, const int32_t* n_active, int64_t max_q, uint32_t* bits, uint32_t* bsum,
                         int32_t* order, int32_t* n_order, hipStream_t st) {
  const int64_t nw = order_words(max_q);
  const int64_t nb = cdiv(nw, kOrderWords);
  (void)hipMemsetAsync(bits, 0, (size_t)nw * sizeof(uint32_t), st);
  (void)hipMemsetAsync(n_order + 1, 0, sizeof(int32_t), st);
  const int64_t gm = std::min<int64_t>(cdiv(max_q > 0 ? max_q : 1, 256), 2048);
  k_order_mark<<<gm, 256, 0, st>>>(active, n_active, max_q, bits, n_order);
  k_order_sum<<<nb, 256, 0, st>>>(bits, nw, bsum);
  k_order_emit<<<nb, 256, 0, st>>>(bits, nw, bsum, order, n_order);
  k_order_copy<<<gm, 256, 0, st>>>(active, n_active, order, n_order);
}
