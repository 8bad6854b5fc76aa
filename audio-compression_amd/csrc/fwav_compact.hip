// fwav_compact.hip — fwav_compact_domains: keep only the domain rows that some match names, renumber the matches.
//
// The decoder reads domains[idx[i]] and nothing else (fractal.py:1414), and a .fwav carries its own n_domains
// (save_compressed / load_compressed, fractal.py:1278-1322), so the pool restricted to the referenced rows, with the
// indices renumbered by rank, is the same codec input.  Six launches on the caller's stream, none of which waits on
// another workgroup:
//   k_compact_zero    bitmap words (one bit per domain) and counts ← 0
//   k_compact_mark    bitmap[v >> 6] |= 1 << (v & 63) for every idx entry v in [0, n_domains) (vector atomic OR);
//                     entries >= n_domains counted (one integer atomic per wave), never marked
//   k_compact_count   per scan block of kScanWords words: prefix[w] = set bits in the block's words before w,
//                     block_sum[b] = set bits in block b
//   k_compact_scan    one workgroup: block_sum ← its exclusive scan, counts[0] = m (and the all-negative rule: row 0)
//   k_compact_gather  one wave per bitmap word: kept[j] = d and pool_out[j] = pool[d] for the word's set bits, whose
//                     ranks j are consecutive from block_sum[w / kScanWords] + prefix[w]
//   k_compact_renumber idx_out[i] = block_sum[..] + prefix[v >> 6] + popcount(word & bits below v), O(1) per entry
// Integer atomics only, so the result is deterministic.  Workspace: [bitmap u64 × W][prefix u32 × W][block_sum u32 × B].
#include "fwav_common.h"
#include "../../include/fwav.h"
#ifdef FWAV_DEBUG_API
#include "../../include/fwav_debug.h"
#endif

namespace fwav {
namespace {

constexpr int kScanThreads = 256;
constexpr int kScanPerThread = 4;
constexpr int kScanWords = kScanThreads * kScanPerThread;  // 1024 bitmap words = 65,536 domains per scan block
constexpr int kGatherWaves = 4;                            // waves (= bitmap words in flight) per gather workgroup
constexpr int kGatherWords = 16;                           // bitmap words per gather workgroup

struct CompactLayout {
  int64_t words, blocks;
  size_t prefix_off, bsum_off, total;
};

__host__ inline size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

__host__ inline CompactLayout compact_layout(int64_t nd) {
  CompactLayout L;
  L.words = nd > 0 ? cdiv(nd, 64) : 1;
  L.blocks = cdiv(L.words, kScanWords);
  L.prefix_off = (size_t)L.words * 8;
  L.bsum_off = L.prefix_off + align8((size_t)L.words * 4);
  L.total = L.bsum_off + align8((size_t)L.blocks * 4);
  return L;
}

__global__ void k_compact_zero(unsigned long long* __restrict__ bitmap, int64_t words, int64_t* __restrict__ counts) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < words) bitmap[w] = 0ull;
  if (w < 2) counts[w] = 0;
}

__global__ void k_compact_mark(const int32_t* __restrict__ idx, int64_t nr, int64_t nd,
                               unsigned long long* __restrict__ bitmap, int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool over = false;
  if (i < nr) {
    const int64_t v = idx[i];
    if (v >= nd)
      over = true;
    else if (v >= 0)
      atomicOr(&bitmap[v >> 6], 1ull << (v & 63));
  }
  const unsigned long long b = __ballot(over);
  if (b != 0ull && (threadIdx.x & (kWave - 1)) == 0)
    atomicAdd((unsigned long long*)&counts[1], (unsigned long long)__popcll(b));
}

// Exclusive scan of one value per thread over a workgroup of kScanThreads; *total = the workgroup's sum.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t s_wave[kScanThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d, kWave);
    if (lane >= d) inc += t;
  }
  __syncthreads();  // s_wave may still be read by a previous call
  if (lane == kWave - 1) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kScanThreads / kWave; ++k) {
    const uint32_t t = s_wave[k];
    if (k < wave) before += t;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(kScanThreads) void k_compact_count(const unsigned long long* __restrict__ bitmap,
                                                                 int64_t words, uint32_t* __restrict__ prefix,
                                                                 uint32_t* __restrict__ bsum) {
  const int64_t w0 = (int64_t)blockIdx.x * kScanWords + (int64_t)threadIdx.x * kScanPerThread;
  uint32_t c[kScanPerThread];
  uint32_t mine = 0;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) {
    c[k] = (w0 + k < words) ? (uint32_t)__popcll(bitmap[w0 + k]) : 0u;
    mine += c[k];
  }
  uint32_t total;
  uint32_t run = block_exclusive_scan(mine, &total);
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) {
    if (w0 + k < words) prefix[w0 + k] = run;
    run += c[k];
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanThreads) void k_compact_scan(uint32_t* __restrict__ bsum, int64_t blocks,
                                                                unsigned long long* __restrict__ bitmap, int64_t nr,
                                                                int64_t* __restrict__ counts) {
  uint32_t carry = 0;
  for (int64_t b0 = 0; b0 < blocks; b0 += kScanThreads) {  // uniform trip count: the scan synchronises
    const int64_t b = b0 + threadIdx.x;
    const uint32_t v = b < blocks ? bsum[b] : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(v, &total);
    if (b < blocks) bsum[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    if (carry == 0 && nr > 0) {  // every entry negative: row 0 stays (the decoder indexes it, a file needs a row)
      bitmap[0] = 1ull;
      carry = 1;
    }
    counts[0] = (int64_t)carry;
  }
}

__global__ __launch_bounds__(kGatherWaves * kWave) void k_compact_gather(
    const unsigned long long* __restrict__ bitmap, int64_t words, const uint32_t* __restrict__ prefix,
    const uint32_t* __restrict__ bsum, const float* __restrict__ pool, int rs, float* __restrict__ pool_out,
    int32_t* __restrict__ kept) {
  __shared__ uint8_t s_bit[2][kGatherWaves][kWave];  // [parity][wave][rank] = the word's rank-th set bit
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t wb = (int64_t)blockIdx.x * kGatherWords;
  int par = 0;
  for (int it = 0; it < kGatherWords / kGatherWaves; ++it, par ^= 1) {  // uniform trip count: one barrier each
    const int64_t w = wb + (int64_t)it * kGatherWaves + wave;
    const unsigned long long word = w < words ? bitmap[w] : 0ull;
    const int cnt = __popcll(word);
    const int rank = __popcll(word & ((1ull << lane) - 1ull));
    const bool set = (word >> lane) & 1ull;
    if (set) s_bit[par][wave][rank] = (uint8_t)lane;
    __syncthreads();  // the parity buffer of two iterations ago was read before the previous barrier
    if (cnt == 0) continue;
    const int64_t base = (int64_t)bsum[w / kScanWords] + (int64_t)prefix[w];
    if (set && kept) kept[base + rank] = (int32_t)(w * 64 + lane);
    const int n = cnt * rs;
    float* __restrict__ dst = pool_out + base * (int64_t)rs;
    for (int e = lane; e < n; e += kWave) {
      const int r = e / rs, c = e - r * rs;
      const int64_t d = w * 64 + (int64_t)s_bit[par][wave][r];
      dst[e] = pool[d * (int64_t)rs + c];
    }
  }
}

__global__ void k_compact_renumber(const int32_t* idx, int64_t nr, int64_t nd,
                                   const unsigned long long* __restrict__ bitmap, const uint32_t* __restrict__ prefix,
                                   const uint32_t* __restrict__ bsum, int32_t* idx_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nr) return;
  const int32_t v = idx[i];  // idx_out may alias idx: each thread reads and writes its own entry only
  int32_t out = v;
  if (v >= 0 && (int64_t)v < nd) {
    const int64_t w = v >> 6;
    const unsigned long long below = bitmap[w] & ((1ull << (v & 63)) - 1ull);
    out = (int32_t)(bsum[w / kScanWords] + prefix[w] + (uint32_t)__popcll(below));
  }
  idx_out[i] = out;
}

[[maybe_unused]] constexpr int kCompactLaunches = 6;

// The argument checks and the six launches of fwav_compact_domains.  ev (NULL in the product entry point): kCompactLaunches
// + 1 events, recorded before the first launch and after each one (fwav_debug_compact_stage_ms).
static int compact_launch(const int32_t* idx, int64_t nr, const float* pool, int64_t nd, int rs, int32_t* idx_out,
                          float* pool_out, int32_t* kept, int64_t* counts, void* ws, size_t ws_bytes, hipStream_t st,
                          hipEvent_t* ev) {
  FWAV_CHECK_ARG(counts, FWAV_ERR_ARG, "fwav_compact_domains: null pointer (counts)");
  FWAV_CHECK_ARG(nr >= 0 && nd >= 0, FWAV_ERR_SHAPE, "fwav_compact_domains: negative count");
  FWAV_CHECK_ARG(rs >= 1 && rs <= 64, FWAV_ERR_SHAPE, "fwav_compact_domains: range_size %d outside 1..64", rs);
  FWAV_CHECK_ARG(nr == 0 || (idx && pool && idx_out && pool_out), FWAV_ERR_ARG, "fwav_compact_domains: null pointer");
  FWAV_CHECK_ARG(nr == 0 || nd >= 1, FWAV_ERR_SHAPE, "fwav_compact_domains: matches but no domain row");
  FWAV_CHECK_ARG(nd <= (int64_t)INT32_MAX, FWAV_ERR_SHAPE, "fwav_compact_domains: n_domains beyond int32 indices");
  const CompactLayout L = compact_layout(nd);
  FWAV_CHECK_ARG(ws && ws_bytes >= L.total, FWAV_ERR_WORKSPACE,
                 "fwav_compact_domains: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, L.total);
  FWAV_CHECK_ARG(((uintptr_t)ws & 7u) == 0, FWAV_ERR_ARG, "fwav_compact_domains: workspace not 8-byte aligned");
  auto* bitmap = (unsigned long long*)ws;
  auto* prefix = (uint32_t*)((char*)ws + L.prefix_off);
  auto* bsum = (uint32_t*)((char*)ws + L.bsum_off);
  int stage = 0;
  auto stamp = [&]() {
    if (ev) (void)hipEventRecord(ev[stage++], st);
  };
  stamp();
  k_compact_zero<<<cdiv(L.words, 256), 256, 0, st>>>(bitmap, L.words, counts);
  FWAV_LAUNCH_CHECK("fwav_compact_domains (zero)");
  stamp();
  if (nr == 0) return FWAV_OK;  // counts = {0, 0}
  k_compact_mark<<<cdiv(nr, 256), 256, 0, st>>>(idx, nr, nd, bitmap, counts);
  FWAV_LAUNCH_CHECK("fwav_compact_domains (mark)");
  stamp();
  k_compact_count<<<L.blocks, kScanThreads, 0, st>>>(bitmap, L.words, prefix, bsum);
  FWAV_LAUNCH_CHECK("fwav_compact_domains (count)");
  stamp();
  k_compact_scan<<<1, kScanThreads, 0, st>>>(bsum, L.blocks, bitmap, nr, counts);
  FWAV_LAUNCH_CHECK("fwav_compact_domains (scan)");
  stamp();
  k_compact_gather<<<cdiv(L.words, kGatherWords), kGatherWaves * kWave, 0, st>>>(bitmap, L.words, prefix, bsum, pool,
                                                                                rs, pool_out, kept);
  FWAV_LAUNCH_CHECK("fwav_compact_domains (gather)");
  stamp();
  k_compact_renumber<<<cdiv(nr, 256), 256, 0, st>>>(idx, nr, nd, bitmap, prefix, bsum, idx_out);
  FWAV_LAUNCH_CHECK("fwav_compact_domains (renumber)");
  stamp();
  return FWAV_OK;
}

}  // namespace
}  // namespace fwav

using namespace fwav;

extern "C" {

size_t fwav_compact_workspace_size(int64_t n_domains, int64_t n_ranges) {
  (void)n_ranges;  // the bitmap and its prefixes depend on the domain count alone
  return compact_layout(n_domains).total;
}

int fwav_compact_domains(const int32_t* idx, int64_t nr, const float* pool, int64_t nd, int rs, int32_t* idx_out,
                         float* pool_out, int32_t* kept, int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  return compact_launch(idx, nr, pool, nd, rs, idx_out, pool_out, kept, counts, ws, ws_bytes, (hipStream_t)stream,
                        nullptr);
}

#ifdef FWAV_DEBUG_API
// Diagnostic (libfwav_debug.so only): fwav_compact_domains with a HIP event between its launches; synchronises.
int fwav_debug_compact_stage_ms(const int32_t* idx, int64_t nr, const float* pool, int64_t nd, int rs,
                                int32_t* idx_out, float* pool_out, int32_t* kept, int64_t* counts, void* ws,
                                size_t ws_bytes, void* stream, float* ms) {
  FWAV_CHECK_ARG(ms && nr > 0, FWAV_ERR_ARG, "fwav_debug_compact_stage_ms: null ms or no ranges");
  hipEvent_t ev[kCompactLaunches + 1];
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) {
      set_error("fwav_debug_compact_stage_ms: hipEventCreate failed");
      return FWAV_ERR_HIP;
    }
  int rc = compact_launch(idx, nr, pool, nd, rs, idx_out, pool_out, kept, counts, ws, ws_bytes, (hipStream_t)stream, ev);
  if (rc == FWAV_OK && hipEventSynchronize(ev[kCompactLaunches]) != hipSuccess) {
    set_error("fwav_debug_compact_stage_ms: hipEventSynchronize failed");
    rc = FWAV_ERR_HIP;
  }
  for (int k = 0; k < kCompactLaunches && rc == FWAV_OK; ++k)
    if (hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]) != hipSuccess) {
      set_error("fwav_debug_compact_stage_ms: hipEventElapsedTime failed");
      rc = FWAV_ERR_HIP;
    }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}
#endif

}  // extern "C"
