// fwav_affine_all.hip — the affine solve over every domain of the pool (compress_audio(candidates="all")).
//
// No counterpart in the reference (opt-in).  For every listed range the five outputs are what fwav_affine_fit writes
// for the candidate row 0, 1, …, n_domains − 1 (K = n_domains) in the same fit mode: the best match any domain gives
// the range, the ceiling that top_k, query and emb_dim approach.  Nothing is gathered: the pool streams past the ranges.
//
// Range sizes 4, 8 and 16 (k_all).  A workgroup of 256 threads owns 256 listed ranges, one per thread: the range (R,
// rc = R − r̄, r̄) and the running best of either orientation stay in registers.  The pool passes through LDS in tiles
// of kAllTile rows.  Per tile the workgroup first computes, one (row, orientation) per thread, the half of the fit that
// does not depend on the range — d̄, d̃ = D − d̄ and Σd̃² + 1e-12 of the row and of its mirror, each with its own
// pairwise sums (orient_domain) — into LDS beside the row; then every thread walks the tile, all lanes reading the
// same LDS address (a broadcast read), and per (range, orientation) does only Σd̃r̃, the divide, the clip, o and the
// error's sum of squares (orient_pair).  The fit is the one of fwav_fit.h; every op is a separately rounded f32 op
// in numpy's pairwise order, so the results are fwav_affine_fit's bit for bit.
//   Selection.  A thread meets the slots of one orientation in ascending key order (FitOrder: fit 1 domain·2 +
// mirrored, fit 0 mirrored·n_domains + domain), so a later slot replaces the running best only with a strictly
// smaller error or as the first NaN.  √ is monotone, so a slot whose sum of squares exceeds the best's cannot have a
// smaller error: its √ is skipped.  Two sums can round to one √, so a sum that is not larger is only a candidate: the
// decision is FitOrder::better on the rooted value and the key.  The two orientations' bests merge in the same order.
//   Few ranges.  When the listed ranges alone cannot fill the device the domain axis is cut into
// fwav_affine_all_slices slices of whole tiles, one workgroup column each (blockIdx.y); every column writes its partial
// best to the workspace and k_all_merge takes their minimum in FitOrder's order — a total order whose keys are
// distinct across slices, so the result does not depend on the split.  With one slice the kernel writes the outputs
// itself and the workspace is not used.
//   Any other range size (k_all_any): one wave per (range, slice), lanes striding over the slice's domains with
// fit_any, then wave_best — k_affine_any with the candidate index replaced by the loop counter.  Exact, not tuned.
// Cost: n_listed · n_domains pairs, two orientations each; DESIGN §3.10 has the instruction count and the roofline.
#include "fwav_fit.h"
#include "../../include/fwav.h"

namespace fwav {

constexpr int kAllThreads = 256;  // k_all: ranges per workgroup (one per thread)
constexpr int kAllTile = 128;     // pool rows per LDS tile: 2·kAllTile (row, orientation) pairs = one per thread
constexpr int kAllAnyRows = 64;   // k_all_any: the wave's stride over the domains
constexpr int kAllBlocks = 1024;  // workgroups that fill the device (256 CUs × 4)
constexpr int kAllMinTiles = 4;   // a slice holds at least this many tiles
static_assert(2 * kAllTile == kAllThreads, "one (row, orientation) per thread in the tile's domain half");

__host__ __device__ inline bool all_fixed(int rs) { return rs == 4 || rs == 8 || rs == 16; }

// The launch geometry: `slices` domain slices of `rows` pool rows each (whole tiles; the last one may be short).
struct AllPlan {
  int slices;
  int64_t rows;
};
__host__ inline AllPlan all_plan(int64_t max_q, int64_t nd, int rs) {
  const int tile = all_fixed(rs) ? kAllTile : kAllAnyRows;
  const int64_t per_block = all_fixed(rs) ? kAllThreads : kAffWaves;
  const int64_t blocks = cdiv(max_q > 0 ? max_q : 1, per_block);
  int64_t want = cdiv(kAllBlocks, blocks);                   // columns that fill the device
  const int64_t most = cdiv(nd > 0 ? nd : 1, (int64_t)tile * kAllMinTiles);  // … of at least kAllMinTiles tiles
  if (want > most) want = most;
  if (want < 1) want = 1;
  const int64_t rows = cdiv(cdiv(nd > 0 ? nd : 1, want), tile) * tile;
  return AllPlan{(int)cdiv(nd > 0 ? nd : 1, rows), rows};   // (no empty slice)
}

// Partial bests of `slices` columns for P list positions, SoA: err, s, o f32[slices·P], slot, dom i32[slices·P].
struct AllPartials {
  float *err, *s, *o;
  int *slot, *dom;
  int64_t P;
  __device__ __forceinline__ void put(int64_t y, int64_t p, const Best& b) const {
    const int64_t j = y * P + p;
    err[j] = b.err; s[j] = b.s; o[j] = b.o; slot[j] = b.slot; dom[j] = b.dom;
  }
  __device__ __forceinline__ Best get(int64_t y, int64_t p) const {
    const int64_t j = y * P + p;
    return Best{err[j], s[j], o[j], slot[j], dom[j]};
  }
};
__host__ inline size_t all_partial_bytes(int64_t P, int slices) { return (size_t)slices * (size_t)P * 20; }

// The row of list position p (−1: not listed, or an entry outside [0, nr))
__device__ __forceinline__ int64_t all_row(const int32_t* __restrict__ active, int64_t p, int64_t n, int64_t nr) {
  if (p >= n) return -1;
  const int64_t r = active ? (int64_t)active[p] : p;
  return (r < 0 || r >= nr) ? -1 : r;
}
__device__ __forceinline__ int64_t all_listed(const int32_t* active, const int32_t* n_active, int64_t max_q,
                                              int64_t nr) {
  if (!active) return nr;
  const int64_t n = *n_active;
  return n < max_q ? n : max_q;
}

// One tile row in LDS: the row, then of either orientation d̃, d̄ and Σd̃² + 1e-12 (16-B aligned: 3·RS + 4 floats)
template <int RS>
struct alignas(16) AllRow {
  float x[RS];
  float dc[2][RS];
  float dm[2], den[2];
};

template <int RS, int FIT>
__global__ __launch_bounds__(kAllThreads) void k_all(const float* __restrict__ ranges, int64_t nr,
                                                     const int32_t* __restrict__ active,
                                                     const int32_t* __restrict__ n_active, int64_t max_q,
                                                     const float* __restrict__ pool, int64_t nd, int64_t slice_rows,
                                                     float s_clip, int32_t* __restrict__ out_idx,
                                                     float* __restrict__ out_s, float* __restrict__ out_o,
                                                     uint8_t* __restrict__ out_sym, float* __restrict__ out_err,
                                                     AllPartials part) {
  using Ord = FitOrder<FIT>;
  __shared__ AllRow<RS> tile[kAllTile];
  const int64_t n = all_listed(active, n_active, max_q, nr);
  const int64_t p = (int64_t)blockIdx.x * kAllThreads + threadIdx.x;
  if ((int64_t)blockIdx.x * kAllThreads >= n) return;  // (the whole workgroup: no barrier is left waiting)
  const int64_t r = all_row(active, p, n, nr);
  float R[RS], rc[RS];
  float rm = 0.f;
  if (r >= 0) {
#pragma unroll
    for (int i = 0; i < RS; ++i) R[i] = ranges[r * RS + i];
    auto fr = [&](int i) { return R[i]; };
    rm = pw_sum_n<RS>(fr) / (float)RS;
  } else {
#pragma unroll
    for (int i = 0; i < RS; ++i) R[i] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < RS; ++i) rc[i] = R[i] - rm;
  const float sc = fabsf(s_clip);

  const int64_t d0 = (int64_t)blockIdx.y * slice_rows;
  const int64_t d1 = d0 + slice_rows < nd ? d0 + slice_rows : nd;
  // the running best of either orientation, and its error's sum of squares (+inf before the first slot)
  Best best[2] = {{INFINITY, 0.f, 0.f, Ord::none, 0}, {INFINITY, 0.f, 0.f, Ord::none, 0}};
  float bss[2] = {INFINITY, INFINITY};
  const int trow = threadIdx.x & (kAllTile - 1), torient = threadIdx.x / kAllTile;  // (orientation: wave-uniform)
  for (int64_t base = d0; base < d1; base += kAllTile) {
    const int nt = d1 - base < kAllTile ? (int)(d1 - base) : kAllTile;
    __syncthreads();  // the previous tile has been read
    if (trow < nt) {
      float D[RS], X[RS], dc[RS], dm, den;
      gather_row<RS>(pool, base + trow, D);
#pragma unroll
      for (int i = 0; i < RS; ++i) X[i] = torient ? D[RS - 1 - i] : D[i];
      orient_domain<RS>(X, dm, dc, den);
      AllRow<RS>& t = tile[trow];
      if (torient == 0) {
#pragma unroll
        for (int i = 0; i < RS; ++i) t.x[i] = D[i];
      }
#pragma unroll
      for (int i = 0; i < RS; ++i) t.dc[torient][i] = dc[i];
      t.dm[torient] = dm;
      t.den[torient] = den;
    }
    __syncthreads();
    if (r < 0) continue;
    for (int j = 0; j < nt; ++j) {
      const AllRow<RS>& t = tile[j];
      const int dom = (int)(base + j);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        float s, o, ss;
        orient_pair<RS, FIT>([&](int i) { return t.x[m ? RS - 1 - i : i]; }, [&](int i) { return t.dc[m][i]; },
                             t.dm[m], t.den[m], R, rc, rm, sc, s, o, ss);
        if (!(ss > bss[m])) {  // not larger, or a NaN on either side: a candidate
          const float e = sqrtf(ss);
          const int key = Ord::key(m ? (int)nd + dom : dom, dom, m);
          if (Ord::better(e, key, best[m].err, best[m].slot)) {
            best[m] = Best{e, s, o, key, dom};
            bss[m] = ss;
          }
        }
      }
    }
  }
  if (r < 0) return;
  const Best b = Ord::better(best[1].err, best[1].slot, best[0].err, best[0].slot) ? best[1] : best[0];
  if (gridDim.y == 1)
    store_best<FIT>(b, r, (int)nd, sc, out_idx, out_s, out_o, out_sym, out_err);
  else
    part.put(blockIdx.y, p, b);
}

// Any other range size: one wave per (listed range, slice), lanes striding over the slice's domains.
template <int FIT>
__global__ __launch_bounds__(64 * kAffWaves) void k_all_any(const float* __restrict__ ranges, int64_t nr, int rs,
                                                            const int32_t* __restrict__ active,
                                                            const int32_t* __restrict__ n_active, int64_t max_q,
                                                            const float* __restrict__ pool, int64_t nd,
                                                            int64_t slice_rows, float s_clip,
                                                            int32_t* __restrict__ out_idx, float* __restrict__ out_s,
                                                            float* __restrict__ out_o, uint8_t* __restrict__ out_sym,
                                                            float* __restrict__ out_err, AllPartials part) {
  using Ord = FitOrder<FIT>;
  const int lane = threadIdx.x & 63;
  const int64_t n = all_listed(active, n_active, max_q, nr);
  const int64_t p = (int64_t)blockIdx.x * kAffWaves + (threadIdx.x >> 6);
  const int64_t r = all_row(active, p, n, nr);
  if (r < 0) return;
  const float* R = ranges + r * rs;
  auto fr = [&](int i) { return R[i]; };
  const float rm = pw_sum(fr, rs) / (float)rs;
  const float sc = fabsf(s_clip);
  const int64_t d0 = (int64_t)blockIdx.y * slice_rows;
  const int64_t d1 = d0 + slice_rows < nd ? d0 + slice_rows : nd;
  Best b{INFINITY, 0.f, 0.f, Ord::none, 0};
  bool have = false;
  for (int64_t d = d0 + lane; d < d1; d += kAllAnyRows) {
    const float* D = pool + d * rs;
    for (int orient = 0; orient < 2; ++orient) {
      float s, o, e;
      fit_any<FIT>(D, orient, R, rm, rs, sc, s, o, e);
      const int key = Ord::key(orient * (int)nd + (int)d, (int)d, orient);
      if (!have || Ord::better(e, key, b.err, b.slot)) { b = Best{e, s, o, key, (int)d}; have = true; }
    }
  }
  wave_best<FIT>(b);
  if (lane != 0) return;
  if (gridDim.y == 1)
    store_best<FIT>(b, r, (int)nd, sc, out_idx, out_s, out_o, out_sym, out_err);
  else
    part.put(blockIdx.y, p, b);
}

// The minimum of the slices' partial bests in FitOrder's order, one thread per list position.
template <int FIT>
__global__ __launch_bounds__(256) void k_all_merge(int64_t nr, const int32_t* __restrict__ active,
                                                   const int32_t* __restrict__ n_active, int64_t max_q, int slices,
                                                   int64_t nd, float s_clip, int32_t* __restrict__ out_idx,
                                                   float* __restrict__ out_s, float* __restrict__ out_o,
                                                   uint8_t* __restrict__ out_sym, float* __restrict__ out_err,
                                                   AllPartials part) {
  const int64_t n = all_listed(active, n_active, max_q, nr);
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = all_row(active, p, n, nr);
  if (r < 0) return;
  Best b = part.get(0, p);
  for (int y = 1; y < slices; ++y) {
    const Best o = part.get(y, p);
    if (FitOrder<FIT>::better(o.err, o.slot, b.err, b.slot)) b = o;
  }
  store_best<FIT>(b, r, (int)nd, fabsf(s_clip), out_idx, out_s, out_o, out_sym, out_err);
}

}  // namespace fwav

using namespace fwav;

template <int FIT>
static void all_launch(const float* ranges, int64_t nr, int rs, const int32_t* active, const int32_t* n_active,
                       int64_t max_q, const float* pool, int64_t nd, float s_clip, int32_t* out_idx, float* out_s,
                       float* out_o, uint8_t* out_sym, float* out_err, void* workspace, hipStream_t st) {
  const AllPlan pl = all_plan(max_q, nd, rs);
  AllPartials part{};
  part.P = max_q;
  if (pl.slices > 1) {
    const int64_t cnt = (int64_t)pl.slices * max_q;
    part.err = (float*)workspace;
    part.s = part.err + cnt;
    part.o = part.s + cnt;
    part.slot = (int*)(part.o + cnt);
    part.dom = part.slot + cnt;
  }
  auto fixed = [&](auto kern) {
    kern<<<dim3((unsigned)cdiv(max_q, kAllThreads), (unsigned)pl.slices), kAllThreads, 0, st>>>(
        ranges, nr, active, n_active, max_q, pool, nd, pl.rows, s_clip, out_idx, out_s, out_o, out_sym, out_err, part);
  };
  switch (rs) {
    case 4: fixed(k_all<4, FIT>); break;
    case 8: fixed(k_all<8, FIT>); break;
    case 16: fixed(k_all<16, FIT>); break;
    default:
      k_all_any<FIT><<<dim3((unsigned)cdiv(max_q, kAffWaves), (unsigned)pl.slices), 64 * kAffWaves, 0, st>>>(
          ranges, nr, rs, active, n_active, max_q, pool, nd, pl.rows, s_clip, out_idx, out_s, out_o, out_sym, out_err,
          part);
  }
  if (pl.slices > 1)
    k_all_merge<FIT><<<cdiv(max_q, 256), 256, 0, st>>>(nr, active, n_active, max_q, pl.slices, nd, s_clip, out_idx,
                                                       out_s, out_o, out_sym, out_err, part);
}

extern "C" {

int fwav_affine_all_tile_rows(int range_size) { return all_fixed(range_size) ? kAllTile : kAllAnyRows; }

int fwav_affine_all_slices(int64_t max_q, int64_t n_domains, int range_size) {
  return all_plan(max_q, n_domains, range_size).slices;
}

size_t fwav_affine_all_workspace_size(int64_t max_q, int64_t n_domains, int range_size) {
  const AllPlan pl = all_plan(max_q, n_domains, range_size);
  return pl.slices > 1 ? all_partial_bytes(max_q > 0 ? max_q : 0, pl.slices) : 0;
}

int fwav_affine_all(const float* ranges, int64_t n_ranges, int range_size, const int32_t* active,
                    const int32_t* n_active, int64_t max_q, const float* pool, int64_t n_domains, float s_clip,
                    int32_t* out_idx, float* out_s, float* out_o, uint8_t* out_sym, float* out_err, int fit,
                    void* workspace, size_t ws_bytes, void* stream) {
  FWAV_CHECK_ARG(fit == kFitReference || fit == kFitClipped, FWAV_ERR_ARG,
                 "fwav_affine_all: fit %d (0: reference, 1: clipped)", fit);
  FWAV_CHECK_ARG(ranges && pool && out_idx && out_s && out_o && out_sym && out_err && (!active || n_active),
                 FWAV_ERR_ARG, "fwav_affine_all: null pointer");
  FWAV_CHECK_ARG(n_ranges >= 0 && range_size >= 1 && n_domains >= 1 && max_q >= 0, FWAV_ERR_SHAPE,
                 "fwav_affine_all: bad shape");
  FWAV_CHECK_ARG(range_size <= kMaxPairwise, FWAV_ERR_SHAPE, "fwav_affine_all: rs > %d", kMaxPairwise);
  // keys are mirrored·n_domains + domain or domain·2 + mirrored in 32 bits; list positions index int32 lists
  FWAV_CHECK_ARG(n_domains < (1LL << 30) && n_ranges < (1LL << 31) && max_q < (1LL << 31), FWAV_ERR_SHAPE,
                 "fwav_affine_all: more than 2^30 domains or 2^31 ranges");
  FWAV_CHECK_ARG(active || max_q >= n_ranges, FWAV_ERR_SHAPE,
                 "fwav_affine_all: max_q < n_ranges with every row listed (active == NULL)");
  const size_t need = fwav_affine_all_workspace_size(max_q, n_domains, range_size);
  FWAV_CHECK_ARG(need == 0 || (workspace && ws_bytes >= need), FWAV_ERR_WORKSPACE,
                 "fwav_affine_all: workspace too small");
  if (n_ranges == 0 || max_q == 0) return FWAV_OK;
  FWAV_CHECK_ARG(!all_fixed(range_size) || ((uintptr_t)pool & 15) == 0, FWAV_ERR_ARG,
                 "fwav_affine_all: pool must be 16-B aligned");
  hipStream_t st = (hipStream_t)stream;
  if (fit == kFitReference)
    all_launch<kFitReference>(ranges, n_ranges, range_size, active, n_active, max_q, pool, n_domains, s_clip, out_idx,
                              out_s, out_o, out_sym, out_err, workspace, st);
  else
    all_launch<kFitClipped>(ranges, n_ranges, range_size, active, n_active, max_q, pool, n_domains, s_clip, out_idx,
                            out_s, out_o, out_sym, out_err, workspace, st);
  FWAV_LAUNCH_CHECK("fwav_affine_all");
  return FWAV_OK;
}

}  // extern "C"
