// fwav_topk_first.h — k_sim_topk_f16, the fp16 first pass and its relaunch modes.
// Part of fwav_topk.hip's translation unit: included there, inside namespace fwav, after the shared constants
// and the headers before it (the file map at the top of fwav_topk.hip); not a header for any other file.
#pragma once

// ------------------------------------------------------------------ fp16 pre-filter + exact f32 rescoring
// Same contract and results as k_sim_topk_f32 (the production K ≤ 64 search).
//
// Exactness.  Three scores per (query, domain): s32 the exact f32 score (sgemv16), s16 = ONE
// v_mfma_f32_32x32x16_f16 of the fp16 high parts (x_hi = f16(x)), shl = s16 + MFMA(d_hi, q_lo) + MFMA(d_lo, q_hi)
// (x_lo = f16(x − x_hi), f32 accumulation).  |s16 − s32| ≤ (2u + u²)·Σ|q_k d_k| + f32 accumulation ≤ 1.9584e-3
// (u = 2^-11; Σ|q_k d_k| ≤ ‖q‖‖d‖ ≤ 2, the tonal and transient heads each having norm ≤ 1) < δ = 2.0e-3;
// |shl − s32| ≤ 3u²·2 + fp16-subnormal low parts (≈ 3e-7) + three MFMAs' f32 accumulation (≤ 48 roundings of ≤ 2,
// 5.7e-6) + s32's own rounding (≈ 1e-6) < δ' = 1e-5 (measured max 6e-7: tools/micro/hilo_err.hip).
// The stream scores every tile with s16 only and fires a tile when some s16 > lim − δ − 2δ'; the replay of a fired
// tile adds the two low-part MFMAs and appends (shl, index) keys with shl > lim to the query's buffer.  A
// compaction takes S = its K-th largest shl and keeps the band shl > lim = S − 2δ' (K domains have s32 ≥ S − δ', so
// every exact top-K member has shl ≥ S − 2δ').  The final pass rescores the band in exact f32 (sgemv16), sorts
// (score desc, index asc) and emits K — identical to the all-f32 kernel whatever the processing order.  A band that
// would not leave 64 free slots (≥ 192 domains within 2δ' of the K-th: runs of identical tiles, periodic signals)
// flags the query for the exact-mode relaunch.
//
// Geometry.  8 waves × 32 queries per workgroup, two workgroups per CU (4 waves per SIMD).  Lane l owns query
// l & 31 (the MFMA's B column, in registers for the whole run) and 16 domain rows of each tile.  The fp16
// table streams through LDS in groups of 4 chunks (256 domains = 8 KB each) with one barrier per group: group
// g+1 goes global → LDS by LDS-DMA (global_load_lds_dwordx4, 8 wave-instructions per chunk) into the other
// half while group g is consumed.  Per chunk a wave issues 8 ds_read_b128 + 8 MFMAs and folds each tile's 16
// outputs into its own integer-max chain (8 × v_max3 per tile), then takes ballots against its integer filter.
// Chunks with a firing chain are recorded (chunk, chain mask) and replayed at the window end (every 32 groups;
// every group during the first 32 chunks) from L2/MALL in batches of 8 tiles: recompute the tile's three MFMAs,
// append survivors to the query's two-ended global key buffer (C = 256 entries), compact a buffer inline when
// it is nearly full.
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
// Native 16-byte vector for the chunk stream (a uint4 struct copy lowers to memcpy, which keeps the prefetch
// array out of registers).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// Launch bounds: the waves per SIMD the register allocation must allow — base and wide, centroid, exact mode (2
// avoids exact mode's register spills but halves the workgroups per CU: 856 vs 785 ms)
constexpr int kWavesPerSimd = 4, kCentWavesPerSimd = 4, kExactWavesPerSimd = 4;
// Wave priorities (s_setprio): centroid level 2 and its appends run at priority 1 (the part of a group whose length
// varies from wave to wave: the group barrier waits for it), and so do the base geometry's window-end replays.
// Same-box A/B, identical outputs (profiles/r05/ab_prio.log): cfg2 17.46 → 17.24 / 17.27 ms with level 2 raised
// (compactions at priority 2 instead: 17.33 / 17.38, both: 17.39 / 17.44, the second-dispatched half of the waves at
// priority 1: +0.5 %, that and the compactions: +2.5 %), 165,375 queries 9.77 → 9.61; the replays as well: cfg3
// 179.8 → 178.3 ms, one rank's eighth and quarter within ±0.5 %
// Exact mode (overflow relaunch) compacts every kExactGrow appends, so its K-th exact key — the store filter —
// and band limit rise sooner (cfg3 at δ = 2.5e-3: 32 / 64 / 96 / 128 / full buffer 859 / 861 / 870 / 887 / 898 ms;
// at δ = 2.0e-3: 16 / 24 / 32 / 64 / 128 → 690 / 702 / 695–704 / 711–725 / 727 ms)
constexpr int kExactGrow = 32;
// (A/B: triggers at 128 / 160 entries, cfg2 18.85 / 18.18 vs 17.50 ms, profiles/r04/ab_trig_*.log)
constexpr int kTrig = k16Cap - 32;  // early compaction: buffer size ...
constexpr int kGrow = 64;           // ... and growth since the last compaction
// Diagnostic counters (fwav_debug_sim_topk only; stays nullptr in production launches), summed over waves:
//   [0] replayed chunks  [1] firing tiles  [2] appends  [3] streaming compactions
//   [4] ticks in window replays (incl. their compactions)  [5] ticks in streaming compactions
//   [6] ticks per wave (whole kernel)  [7] ticks waiting at the group barrier  [8] ticks in the final pass
//   [9] ticks streaming (MFMA + filter, between barrier and window end)   (s_memrealtime ticks, 100 MHz)
// `stats` inside the kernel is the wave's own LDS counter row (lane 0 adds; flushed once per wave at the end),
// so the instrumentation adds no global atomics to the measured loop.
// [12] ticks waiting for the group's own chunk DMA (vmcnt at the group top; [7] is then the barrier alone),
//   [13] centroid level-1 ticks, [14] centroid level-2 (tile, set) pairs
// The prologue's counters live in slots of their own, [16 .. kStatsX), which only the STATS kernels' LDS rows have and
// which reach the caller's array only on request (dbg 64: callers that pass u64[16] are never written past it):
//   [16] ticks in the prologue (kernel start to the first group's DMA)  [17] ticks in its seed phase
//   [18] (query set, item) pairs that ran the seeds' full bit search
constexpr int kStats = 16;
constexpr int kStatsX = 20;
__device__ __forceinline__ void stat_add_p(unsigned long long* stats, int i, unsigned long long v) {
  if (stats != nullptr && (threadIdx.x & 63) == 0) stats[i] += v;
}
extern "C" __device__ uint32_t __ockl_wfred_add_u32(uint32_t);
#define stat_add(i, v) stat_add_p(stats, (i), (v))
// Window schedule (A/B at cfg2 with 8 chains: 16 groups / 64 warm chunks 21.17 ms, 32 / 64 20.92, 16 / 32 20.85,
// 32 / 32 20.67, 32 / 16 20.70; 8 groups 20.68 vs 20.26 on a faster box)
constexpr int kWindowGroups = 32;  // after the warm-up, fired chunks are replayed every 32 groups (128 chunks)
// fired-chunk FIFO per query group (a ring; power of two).  Measured and rejected (cfg2 A/B, identical outputs):
// replaying B ≤ 4 pending tiles per group with prefetched fragments instead of whole windows (27–32 ms vs 22.9:
// the band limit then rises too late), and windows at doubling stream lengths (28.0 vs 21.7 ms).
constexpr int kFifo = kWindowGroups * 4;
static_assert((kFifo & (kFifo - 1)) == 0, "the fired-chunk ring needs a power-of-two size");
constexpr int kWarmChunks = 32;   // ... and after every group during the first 32 chunks

// Component c (a compile-time constant after unrolling) of a float4.
__device__ __forceinline__ float f4c(const float4& v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }

// Max of the 16 scores of a lane as an int over the float bits (v_max3_i32; a float max would be preceded
// by canonicalising v_max_f32 x,x on every MFMA output).  For a threshold t >= 0, (int)x > (int)t ⟺ x > t
// for every non-NaN x (negative floats are negative ints); callers use it only in that regime.
__device__ __forceinline__ int imax16(const floatx16& a) {
  auto I = [&](int i) { return __float_as_int(a[i]); };
  auto mx = [](int x, int y) { return x > y ? x : y; };
  const int m0 = mx(mx(I(0), I(1)), I(2));
  const int m1 = mx(mx(I(3), I(4)), I(5));
  const int m2 = mx(mx(I(6), I(7)), I(8));
  const int m3 = mx(mx(I(9), I(10)), I(11));
  const int m4 = mx(mx(I(12), I(13)), I(14));
  return mx(mx(mx(m0, m1), mx(m2, m3)), mx(m4, I(15)));
}

// Does any score in this lane's imax beat the filter thf?  Exact for thf >= 0; always true for thf < 0
// (then the exact per-score test in the slow path decides).
__device__ __forceinline__ bool may_pass(int imx, float thf) {
  return thf < 0.0f || imx > __float_as_int(thf);
}

// NG = query groups of 32 per workgroup (W waves × QS sets).  Kept small: two workgroups (2 × 64 KB of chunk
// slots + this) must fit one CU's 160 KB of LDS.
template <int NG, bool STATS, bool FIFO = true, int NW = NG>
struct Topk16SmemT {
  int cnt[32 * NG];   // final pass: entries at the front of the query's buffer (its h = 0 lane's appends)
  int cnt1[32 * NG];  // ... and at the back (its h = 1 lane's)
  int ovf[32 * NG];  // band overflowed the buffer (f2key of its band limit, else 0): recompute in exact mode
  // exact mode: f2key of the largest K-th score that a domain of equal score was not kept at (0: none) — a boundary
  // tie (tie_flags bit 1) only if it is the final K-th score
  uint32_t tie[32 * NG];
  int64_t qrow[32 * NG];
  int32_t qpos[32 * NG];  // position of the slot's query in the active list (index of its shared band limit)
  uint32_t fired[FIFO ? NG : 1][kFifo];            // deferred work: ring of fired chunk entries (not in CENT)
  unsigned long long wstat[STATS ? NW : 1][STATS ? kStatsX : kStats];  // STATS builds only (one row per wave)
};
// The per-query rows of the centroid geometry with 4 query sets per wave (1,024 queries per workgroup: S16 / HL
// passes only): 14 B per query instead of 28, so that two workgroups' 2 × G chunk slots still fit a CU's LDS.  The
// buffer counts are 16-bit and live here for the whole pass (a set's counts and `kept` are in registers only while
// its level-2 pairs are scored: they are cold during level 1); the query's table row is rebuilt from the active list
// where the final pass needs it; `tie` is exact mode's and reads as 0.
template <int NG, bool STATS, int NW>
struct Topk16SmemColdT {
  struct ZeroRow {
    __device__ uint32_t operator[](int) const { return 0u; }
  };
  union {
    struct {
      uint16_t cnt[32 * NG];   // entries at the front of the query's buffer (its h = 0 lane's appends)
      uint16_t cnt1[32 * NG];  // ... and at the back (its h = 1 lane's)
    };
    uint16_t cnt01[2 * 32 * NG];  // both, by lane: h · 32·NG + slot
  };
  uint16_t kept[32 * NG];  // the buffer's size after its last compaction
  int ovf[32 * NG];
  int32_t qpos[32 * NG];
  ZeroRow tie;
  unsigned long long wstat[STATS ? NW : 1][STATS ? kStatsX : kStats];
};

// Streaming compaction on shl keys (no f32 rescoring, no table loads, no sort): S = the K-th largest shl in the
// buffer; every exact top-K member has shl ≥ S − 2δ' (K domains have s32 ≥ S − δ'), so keep the band shl > S − 2.5δ'
// (unsorted; the final pass rescores and sorts) and filter new domains with it.  A greedy bitwise radix select over
// the 32 key bits finds key(S) with ballots and scalar popcounts (no sort).  If the band would not leave 64 free
// slots the query is flagged (ovf) and searched again in exact mode.
// Key-buffer reads: L2-served (sc1), never a possibly stale L1 copy of a line this wave loaded before its later
// appends to it.
__device__ __forceinline__ uint64_t ld_key(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Entry e of a two-ended buffer holding n0 entries at the front and n1 at the back (append_tile).
template <int C>
__device__ __forceinline__ int two_end_slot(int e, int n0) {
  return e < n0 ? e : C - 1 - (e - n0);
}

template <int C, bool HL, class SM>
__device__ __forceinline__ void compact16_s16(uint64_t* __restrict__ kq, int n0, int n1, SM& sm, int ql, int K,
                                              unsigned long long* stats, int& m_out, float& lim_out) {
  constexpr int E = C / 64;
  const unsigned long long t_start = stats ? __builtin_amdgcn_s_memrealtime() : 0;
  const int lane = threadIdx.x & 63;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int n = min(n0 + n1, C);
  uint64_t v[E];
  uint32_t hi[E];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = j * 64 + lane;
    v[j] = e < n ? ld_key(kq + two_end_slot<C>(e, n0)) : 0ull;
    hi[j] = (uint32_t)(v[j] >> 32);  // 0 for empty slots; f2key of any real score is > 0
  }
  float lim = -INFINITY;
  if (n >= K) {
    uint32_t T = 0;
    // HL: full precision; S16: the top 20 key bits (S16 is needed only as a lower bound at ≈ 2^-11 resolution)
    for (int bit = 31; bit >= (HL ? 0 : 12); --bit) {
      const uint32_t Tc = T | (1u << bit);
      int c = 0;
#pragma unroll
      for (int j = 0; j < E; ++j) c += __popcll(__ballot(hi[j] >= Tc));
      if (c >= K) T = Tc;
    }
    lim = HL ? key2f(T) - 2.5f * kHLDelta : key2f(T) - 2.0f * kF16Delta;
  }
  // keep: every real entry with shl > lim, written densely in (j, lane) order
  int m = 0;
  int ovf = 0;
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const bool keep = hi[j] != 0u && key_score(v[j]) > lim;
    const uint64_t bm = __ballot(keep);
    const int pos = m + __popcll(bm & ((1ull << lane) - 1ull));
    if (keep && pos < C - 64) kq[pos] = v[j];
    m += __popcll(bm);
  }
  if (m > C - 64) {
    m = C - 64;
    ovf = 1;
  }
  // the flag carries the band limit at overflow (f2key, never 0): a valid lower bound on the s16 of every domain of
  // the query's exact top K, so it seeds the exact-mode relaunch
  if (lane == 0 && ovf) sm.ovf[ql] = (int)f2key(lim);
  m_out = m;
  lim_out = lim;
  if (stats) {
    stat_add(3, 1);
    stat_add(5, __builtin_amdgcn_s_memrealtime() - t_start);
  }
}

// Final pass of query ql (a whole-table item): rescore its two-ended buffer (sm.cnt entries at the front, sm.cnt1 at
// the back) in exact f32 (sgemv16), sort, emit the top K to `out`; qrow = the query's row of the query table qemb
// (the domain table itself unless the search was given another, QueryTab).  Whole wave.  Every
// per-query buffer and counter is owned by one wave, so no cross-wave fences are needed; the wave's own appended
// stores are drained once (vmcnt(0)), then all key loads and all row loads are issued together (two memory round
// trips in total).
template <int C, int E, class SM>
__device__ __forceinline__ void compact16_e(uint64_t* __restrict__ kq, SM& sm, int ql, int K,
                                            const float* __restrict__ emb, int32_t* __restrict__ out,
                                            const SgemvSplit& sp, int32_t* __restrict__ ties, int32_t qid,
                                            uint32_t fkey, const FloorCtl& fl, const float* __restrict__ qemb,
                                            int64_t qrow) {
  const int lane = threadIdx.x & 63;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int n0 = sm.cnt[ql];
  const int n = min(n0 + sm.cnt1[ql], C);
  const float4* qp = reinterpret_cast<const float4*>(qemb + qrow * 16);
  uint64_t v[E];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = j * 64 + lane;
    v[j] = e < n ? ld_key(kq + two_end_slot<C>(e, n0)) : 0ull;
  }
  float qv[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 w = qp[i];
    qv[4 * i] = w.x; qv[4 * i + 1] = w.y; qv[4 * i + 2] = w.z; qv[4 * i + 3] = w.w;
  }
  // rescore the entries two slots at a time (8 row loads in flight per lane)
#pragma unroll
  for (int j0 = 0; j0 < E; j0 += 2) {
    float4 row[2][4];
    int32_t dd[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = j0 + jj;
      const int e = j * 64 + lane;
      dd[jj] = (j < E && e < n) ? key_idx(v[j < E ? j : 0]) : 0;
      const float4* p = reinterpret_cast<const float4*>(emb + (int64_t)dd[jj] * 16);
#pragma unroll
      for (int i = 0; i < 4; ++i) row[jj][i] = p[i];
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = j0 + jj;
      const int e = j * 64 + lane;
      if (j < E && e < n) {
        const float acc = sgemv16([&](int k) { return f4c(row[jj][k >> 2], k & 3); }, [&](int k) { return qv[k]; },
                                  sgemv_kind((uint32_t)dd[jj], sp));
        v[j] = make_key(acc, dd[jj]);
      }
    }
  }
  wave_sort_desc<E>(v);
  // exactly tied scores at the top: listed for fwav_tie_check (not for a query about to be searched again)
  uint64_t kth = 0;
#pragma unroll
  for (int j = 0; j < E; ++j)
    if (j == ((K - 1) >> 6)) kth = __shfl(v[j], (K - 1) & 63);
  // a speculative floor that may have cut a member: the query goes to the second pass, nothing is emitted here
  if (sm.ovf[ql] == 0 && floor_miss(fkey, fl, n, K, kth, qid)) return;
  const uint32_t tv = sm.tie[ql];
  const int tf = tie_flags<E>(v, n, K) | (tv != 0u && n >= K && key2f(tv) == key_score(kth) ? 2 : 0);
  // the band of the S16 / HL modes holds every domain within the band margin of the K-th score, so the K-th's whole
  // tie group; exact mode keeps only the top K (a tied domain seen later was dropped: tv)
  if (sm.ovf[ql] == 0) record_tie<E>(ties, qid, tf, v, n, K, tv == 0u);
  // Emit straight from registers (never read back what was just stored: a load issued right behind the stores
  // of the same addresses can return the old contents): the K candidate indices, −1-padded.
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = j * 64 + lane;
    if (e < K) out[e] = e < n ? key_idx(v[j]) : -1;
  }
}

// A buffer of at most 128 entries (the usual case: the band kept by the last compaction plus the few appends after
// it) is rescored two entries per lane and sorted as 128 keys; a fuller one as C.  Same outputs either way.
template <int C, class SM>
__device__ __forceinline__ void compact16(uint64_t* __restrict__ kq, SM& sm, int ql, int K,
                                          const float* __restrict__ emb, int32_t* __restrict__ out,
                                          const SgemvSplit& sp, int32_t* __restrict__ ties, int32_t qid,
                                          uint32_t fkey, const FloorCtl& fl, const float* __restrict__ qemb,
                                          int64_t qrow) {
  const int n = __builtin_amdgcn_readfirstlane(sm.cnt[ql] + sm.cnt1[ql]);
  if (C > 128 && n <= 128)
    compact16_e<C, 2, SM>(kq, sm, ql, K, emb, out, sp, ties, qid, fkey, fl, qemb, qrow);
  else
    compact16_e<C, C / 64, SM>(kq, sm, ql, K, emb, out, sp, ties, qid, fkey, fl, qemb, qrow);
}

// End of a table piece (split block): no rescoring and no sort here — the piece keeps the entries of its band whose
// key beats the query's shared limit (Lk, the f2key of the largest band limit any piece of the query has published;
// every exact top-K member's key is above it), written densely at the front of its buffer, and a header in the last
// slot: (overflow key << 32) | count.  k_merge_pieces rescores and sorts the union of the pieces' bands once per
// query.  A band that would not leave 64 slots is flagged as overflowed (the query goes to the exact-mode relaunch).
// The band's keys of query ql (n = its entries, 0 past them), loaded by piece_band_load — for kBandBatch queries at
// once, so that the final loop of a table piece pays one memory round trip per batch instead of two per query
// (round 6, same process, identical candidates, profiles/r06/ab_band_batch.log: 330,750 / 165,375 / 82,688 / 41,344
// queries 14.49 → 14.38 / 8.07 → 7.86 / 4.48 → 4.37 / 2.82 → 2.72 ms)
constexpr int kBandBatch = 4;
template <int C, class SM>
__device__ __forceinline__ int piece_band_load(const uint64_t* __restrict__ kq, SM& sm, int ql,
                                               uint64_t (&v)[C / 64]) {
  constexpr int E = C / 64;
  const int lane = threadIdx.x & 63;
  const int n0 = sm.cnt[ql];
  const int n = min(n0 + sm.cnt1[ql], C);
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = j * 64 + lane;
    v[j] = e < n ? ld_key(kq + two_end_slot<C>(e, n0)) : 0ull;
  }
  return n;
}
// sh0: the query's shared limit read with its keys (any earlier value is a valid, smaller lower bound)
template <int C, bool HL, class SM>
__device__ __forceinline__ void piece_band(uint64_t* __restrict__ kq, SM& sm, int ql, int K,
                                           uint32_t* __restrict__ share_q, uint64_t (&v)[C / 64], int n,
                                           uint32_t sh0) {
  constexpr int E = C / 64;
  const int lane = threadIdx.x & 63;
  // the piece's own limit now (a last compaction's select over its whole buffer), published before the filter so
  // that the pieces still streaming and k_merge_pieces see it
  uint32_t Lk = 0u;
  if (n >= K) {
    uint32_t T = 0;
    for (int bit = 31; bit >= (HL ? 0 : 12); --bit) {
      const uint32_t Tc = T | (1u << bit);
      int c = 0;
#pragma unroll
      for (int j = 0; j < E; ++j) c += __popcll(__ballot((uint32_t)(v[j] >> 32) >= Tc));
      if (c >= K) T = Tc;
    }
    Lk = f2key(HL ? key2f(T) - 2.5f * kHLDelta : key2f(T) - 2.0f * kF16Delta);
    if (lane == 0) atomicMax(share_q, Lk);
  }
  Lk = max(Lk, sh0);
  int m = 0;
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const bool keep = v[j] != 0ull && (uint32_t)(v[j] >> 32) > Lk;
    const uint64_t bm = __ballot(keep);
    const int pos = m + __popcll(bm & ((1ull << lane) - 1ull));
    if (keep && pos < C - 64) kq[pos] = v[j];
    m += __popcll(bm);
  }
  uint32_t ovf = (uint32_t)sm.ovf[ql];
  if (m > C - 64) {
    m = C - 64;
    if (ovf == 0u) ovf = Lk != 0u ? Lk : 1u;  // any nonzero flag; the limit (if any) is a valid relaunch seed
  }
  if (lane == 0) kq[C - 1] = ((uint64_t)ovf << 32) | (uint32_t)m;
}

// Integer filter threshold for the fold-max test: (int)x > thi ⟺ x > thf for non-NaN x when thf >= 0;
// for thf < 0 every tile goes to the exact per-score test.
__device__ __forceinline__ int int_threshold(float thf) {
  return thf < 0.0f ? (int)0x80000000 : __float_as_int(thf);
}

__device__ __forceinline__ int fold16(int r, const floatx16& a) {
  auto I = [&](int i) { return __float_as_int(a[i]); };
  auto m3 = [](int x, int y, int z) { return max(max(x, y), z); };
  r = m3(r, I(0), I(1));
  r = m3(r, I(2), I(3));
  r = m3(r, I(4), I(5));
  r = m3(r, I(6), I(7));
  r = m3(r, I(8), I(9));
  r = m3(r, I(10), I(11));
  r = m3(r, I(12), I(13));
  return m3(r, I(14), I(15));
}

// One recomputed tile of a replay (acc = the tile's fp16 MFMA scores, domains dt .. dt+31): append the
// survivors (s16 keys) to the wave-owned global key buffers — one LDS atomic per lane reserves the slots,
// the stores are fire-and-forget — and compact a buffer inline only when it is about to overflow.
// Exact-mode compaction (the overflow relaunch, EX): the buffer holds exact f32 keys, so it keeps exactly its top K
// (a sort of the ≤ C keys; entries are distinct (score, index) keys, so no tie group can overflow), written sorted at
// the front.  New domains can only matter with s32 > S32_K (a later domain of equal score has a larger index), i.e.
// s16 > S32_K − δ: that is the returned filter limit.
template <int C>
__device__ __forceinline__ void compact_exact(uint64_t* __restrict__ kq, int n0, int n1, int K, int& m_out,
                                              float& lim_out, uint64_t& kth_out, uint32_t* __restrict__ tie_slot) {
  constexpr int E = C / 64;
  const int lane = threadIdx.x & 63;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int n = min(n0 + n1, C);
  uint64_t v[E];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = j * 64 + lane;
    v[j] = e < n ? ld_key(kq + two_end_slot<C>(e, n0)) : 0ull;
  }
  wave_sort_desc<E>(v);
  const int kl = (K - 1) & 63, kj = (K - 1) >> 6;
  uint64_t kth = 0;
#pragma unroll
  for (int j = 0; j < E; ++j)
    if (j == kj) kth = __shfl(v[j], kl);
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = j * 64 + lane;
    if (e < K && e < n) kq[e] = v[j];
  }
  // a dropped (K+1)-th entry with the K-th's score: the set among the equal scores is numpy's choice
  const int kl1 = K & 63, kj1 = K >> 6;
  uint32_t kh = 0u, k1h = 0u;
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int hj = (int)(uint32_t)(v[j] >> 32);
    const int a = __shfl(hj, kl), b = __shfl(hj, kl1);
    if (j == kj) kh = (uint32_t)a;
    if (j == kj1) k1h = (uint32_t)b;
  }
  if (lane == 0 && n > K && key2f(k1h) == key2f(kh)) atomicMax(tie_slot, kh);
  m_out = n < K ? n : K;
  lim_out = n >= K ? key_score(kth) - kF16Delta : -INFINITY;
  kth_out = n >= K ? kth : 0ull;
}

template <int C, bool STATS, class SM, int MODE>
__device__ __forceinline__ float append_tile(const floatx16& acc, float thf, int& qcnt, int& kept, int64_t dt, int64_t nd,
                                             uint64_t* __restrict__ gkeys, SM& sm, int qg, int K, int upd,
                                             unsigned long long* stats, const SgemvSplit& sp,
                                             const float* __restrict__ emb = nullptr,
                                             const float* qv = nullptr, uint64_t* kthp = nullptr,
                                             uint32_t* __restrict__ share = nullptr) {
  constexpr bool EX = MODE == kModeEX;
  const int lane = threadIdx.x & 63;
  const int col = lane & 31;
  const int h = lane >> 5;
  const int ql = qg * 32 + col;  // qg: the wave-uniform query group (32 queries) of this tile
  if (__ballot(fold16((int)0x80000000, acc) > int_threshold(thf)) == 0ull) return thf;
  if (STATS) stat_add(1, 1);
  const unsigned long long t_a0 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
  // Two-ended buffer: the h = 0 lane of a query appends at the front (slots 0, 1, …), the h = 1 lane at the back
  // (C−1, C−2, …), so a lane stores each survivor at its own running slot as soon as its compare passes: one
  // compare, the key and one exec-masked store per row, and no per-tile exchange of counts before the stores.
  // Byte offsets from the item's key region stay 32-bit (≤ 32·NG·C·8 B).
  const uint32_t nd0 = ~(uint32_t)(dt + 4 * h);  // key low word of row r: ~(domain index) = nd0 − offset(r)
  floatx16 a = acc;
  if (dt + 32 > nd) {  // wave-uniform: the table's last tile; rows past the end never pass
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (dt + 4 * h + (r & 3) + 8 * (r >> 2) >= nd) a[r] = -INFINITY;
  }
  const int before = qcnt;
  int slot = h ? C - 1 - qcnt : qcnt;
  const int step = h ? -1 : 1;
  char* kbase = reinterpret_cast<char*>(gkeys);
  if constexpr (EX) {
    // EX: exact f32 keys (sgemv16, the final pass's score) of the rows whose s16 passes the filter — typically one
    // or none per lane and tile, so they are computed on the VALU from the rows' f32 embeddings, two rows per lane
    // and memory round trip, in increasing row order (the order of the stores below)
    uint32_t pm = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) pm |= (a[r] > thf ? 1u : 0u) << r;
    while (__ballot(pm != 0u) != 0ull) {
      int rr[2];
      bool on[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        on[u] = pm != 0u;
        rr[u] = on[u] ? __builtin_ctz(pm) : 0;
        if (on[u]) pm &= pm - 1u;
      }
      float4 row[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int64_t d = dt + 4 * h + (rr[u] & 3) + 8 * (rr[u] >> 2);
        const float4* p = reinterpret_cast<const float4*>(emb + (on[u] ? d : dt) * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) row[u][i] = p[i];
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (on[u]) {
          const int r = rr[u];
          const int64_t dr = dt + 4 * h + (r & 3) + 8 * (r >> 2);
          const float sc = sgemv16([&](int k) { return f4c(row[u][k >> 2], k & 3); }, [&](int k) { return qv[k]; },
                                   sgemv_kind((uint32_t)dr, sp));
          const uint32_t uu = __float_as_uint(sc);
          const uint32_t key = uu ^ ((uint32_t)((int32_t)uu >> 31) | 0x80000000u);
          const uint64_t k64 = ((uint64_t)key << 32) | (uint64_t)(nd0 - (uint32_t)((r & 3) + 8 * (r >> 2)));
          // a domain that does not beat the query's current K-th exact key can never enter its top K (groups of
          // equal scores — repeated or silent tiles — are decided here, without stores or compactions)
          if (k64 > *kthp) {
            *reinterpret_cast<uint64_t*>(kbase + (uint32_t)((ql * C + slot) * 8)) = k64;
            slot += step;
          } else if (key_score(k64) == key_score(*kthp)) {
            // equal to the K-th exact score, later in index order: numpy decides whether it is in
            atomicMax(&sm.tie[ql], (uint32_t)(*kthp >> 32));
          }
        }
      }
    }
  } else {
    // a running byte offset (one add per stored row, the store's own VGPR offset) and the key's low word as one
    // subtraction from an opaque nd0 (the compiler otherwise derives it from dt's known low bits in two ops)
    uint32_t off = (uint32_t)((ql * C + slot) * 8);
    const uint32_t dstep = h ? (uint32_t)-8 : 8u;
    uint32_t nd0o = nd0;
    asm volatile("" : "+v"(nd0o));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (a[r] > thf) {
        // f2key of the score, branch-free: negative → ~u, else u | sign
        const uint32_t u = __float_as_uint(a[r]);
        const uint32_t key = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
        const uint64_t k64 = ((uint64_t)key << 32) | (uint64_t)(nd0o - (uint32_t)((r & 3) + 8 * (r >> 2)));
        *reinterpret_cast<uint64_t*>(kbase + off) = k64;
        off += dstep;
      }
    }
    slot = (int)(off / 8) - ql * C;
  }
  qcnt = h ? C - 1 - slot : slot;  // this lane's entries; ≤ C in total: see the compaction trigger below
  // the query's total (both lanes) in every lane, by one cross-half swap
  const auto sw = __builtin_amdgcn_permlane32_swap((uint32_t)qcnt, (uint32_t)qcnt, false, false);
  const int total = (int)(sw[0] + sw[1]);
  if (STATS) {
    stat_add(2, __ockl_wfred_add_u32((uint32_t)(qcnt - before)));
    stat_add(10, __builtin_amdgcn_s_memrealtime() - t_a0);
  }
  // compact when fewer than 32 free slots remain (a tile adds ≤ 16 per lane, ≤ 32 per query) — or, to raise the band
  // limit sooner, once the buffer passes kTrig and has grown by kGrow since its last compaction
  uint64_t need = __ballot(lane < 32 && (total > C - 32 || (total > kTrig && total >= kept + kGrow) ||
                                         (EX && total >= kept + kExactGrow)));
  while (need != 0ull) {
    const int l = __builtin_ctzll(need);
    need &= need - 1;
    int m;
    float lim;
    uint64_t kth_l = 0;
    if constexpr (EX)
      compact_exact<C>(gkeys + (size_t)(qg * 32 + l) * C, __builtin_amdgcn_readlane(qcnt, l),
                       __builtin_amdgcn_readlane(qcnt, l + 32), K, m, lim, kth_l, &sm.tie[qg * 32 + l]);
    else
      compact16_s16<C, MODE == kModeHL>(gkeys + (size_t)(qg * 32 + l) * C, __builtin_amdgcn_readlane(qcnt, l),
                       __builtin_amdgcn_readlane(qcnt, l + 32), sm, qg * 32 + l, K, STATS ? stats : nullptr, m, lim);
    if (col == l) {
      qcnt = h ? 0 : m;  // the kept band is written densely at the front
      kept = m;
      if (upd) thf = fmaxf(thf, lim);  // the seed may be above a buffer's own limit
      // a table piece publishes its limit to the query's other pieces (shared_limit below)
      if (share != nullptr && h == 0 && lim > -INFINITY) atomicMax(share + sm.qpos[qg * 32 + l], f2key(lim));
      // a query whose band overflowed is searched again in exact mode: stop appending for it here
      if (!EX && sm.ovf[qg * 32 + l]) thf = INFINITY;
      if (EX) *kthp = kth_l;
    }
  }
  return thf;
}

// Window end: replay what this wave recorded.  An entry is (chunk << 8 | chain mask).  The recorded tiles are walked
// with a wave-uniform cursor in batches of kReplayBatch: all of a
// batch's fragment loads (from the fp16 table, L2/MALL-resident) are issued together, so a window costs
// ~one memory round trip per batch instead of one per chunk, and tiles of quiet chains are not recomputed.
constexpr int kReplayBatch = 8;
// Cursor over a query group's pending fired tiles: FIFO entries [head, tail) of `fired` (a ring), the entry being
// expanded (chunk cc, tiles rem).  Wave-uniform.
struct ReplayCursor {
  int head;
  int64_t cc;
  uint32_t rem;
};
// Fold chains per 256-domain chunk: tile t folds into chain t % kChains; a fired chunk is recorded as
// (chunk << 8 | chain mask) and its replay recomputes the tiles of the firing chains: one chain per tile.
constexpr int kChains = 8;
static_assert(kChains == 8, "next_tile reads the chain mask as the chunk's tile mask");
// Next pending tile (its first domain), or −1.
__device__ __forceinline__ int64_t next_tile(ReplayCursor& cur, int tail, const uint32_t* fired) {
  while (cur.rem == 0u && cur.head < tail) {
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane(fired[cur.head++ & (kFifo - 1)]);
    cur.cc = e >> 8;
    cur.rem = e & 255u;
  }
  if (cur.rem == 0u) return -1;
  const int t = __builtin_ctz(cur.rem);
  cur.rem &= cur.rem - 1;
  return cur.cc * kChunk + t * 32;
}
__device__ __forceinline__ half8 tile_fragment(const _Float16* __restrict__ emb16, int64_t dt, int h, int col) {
  const int64_t c = dt / kChunk, t = (dt % kChunk) / 32;
  return *reinterpret_cast<const half8*>(emb16 + ((c * 2 + h) * kChunk + col) * 8 + t * 256);
}

template <int C, bool STATS, class SM, int MODE>
__device__ __forceinline__ float replay_window(const _Float16* __restrict__ emb16, const _Float16* __restrict__ emb16lo,
                                               half8 b, half8 bl, float thf, int& qcnt,
                                               int& kept, ReplayCursor& cur, int tail, int64_t nd, uint64_t* __restrict__ gkeys,
                                               SM& sm, int qg, int K, int upd, unsigned long long* stats,
                                               const SgemvSplit& sp, const float* __restrict__ emb = nullptr,
                                               const float* qv = nullptr, uint64_t* kthp = nullptr,
                                               uint32_t* __restrict__ share = nullptr) {
  constexpr bool HL = MODE == kModeHL;
  const int lane = threadIdx.x & 63;
  const int col = lane & 31;
  const int h = lane >> 5;
  if (STATS) stat_add(0, tail - cur.head);
  while (true) {
    int64_t ct[kReplayBatch];  // tile start domain, −1 = none
#pragma unroll
    for (int u = 0; u < kReplayBatch; ++u) ct[u] = next_tile(cur, tail, sm.fired[qg]);
    if (ct[0] < 0) break;
    half8 af[kReplayBatch], afl[HL ? kReplayBatch : 1];
#pragma unroll
    for (int u = 0; u < kReplayBatch; ++u)  // unconditional loads (no wait on the spot)
      af[u] = tile_fragment(emb16, ct[u] < 0 ? ct[0] : ct[u], h, col);
    if constexpr (HL) {  // the low parts of the fired tiles' domains (shl)
#pragma unroll
      for (int u = 0; u < kReplayBatch; ++u) afl[u] = tile_fragment(emb16lo, ct[u] < 0 ? ct[0] : ct[u], h, col);
    }
    if (STATS) {  // time the fragment round trip (timing build only: forces the wait here)
      const unsigned long long t_l0 = __builtin_amdgcn_s_memrealtime();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      stat_add(11, __builtin_amdgcn_s_memrealtime() - t_l0);
    }
#pragma unroll
    for (int u = 0; u < kReplayBatch; ++u) {
      if (ct[u] < 0) break;
      floatx16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[u], b, floatx16{}, 0, 0, 0);
      if constexpr (HL) {
        // shl = s16 + d_hi·q_lo + d_lo·q_hi, f32 accumulation.  (The limit may have risen since the tile fired, but
        // testing the tile's s16 against it before the two low-part MFMAs lengthens each tile's dependent chain: A/B
        // at cfg2 21.38 vs 20.98 ms without the test, cfg3 192.8 vs 188.5)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[u], bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afl[u], b, acc, 0, 0, 0);
      }
      thf = append_tile<C, STATS, SM, MODE>(acc, thf, qcnt, kept, ct[u], nd, gkeys, sm, qg, K, upd, stats, sp, emb,
                                          qv, kthp, share);
    }
    if (ct[kReplayBatch - 1] < 0) break;
  }
  return thf;
}

// Seed of a query's band limit before the stream: the K-th largest s16 among the domains of its own window
// [qrow − 64, qrow + 64).  Consecutive domains are windows 2 samples apart, so this window holds close matches and
// its K-th score is far above what the first streamed chunks give; a valid start for the rising limit (K domains
// have s16 ≥ T, so s32 ≥ T − δ: every exact top-K member has shl > T − δ − 2δ', and s16 > T − 2δ for the exact
// mode's s16-scale limit), it removes the first compactions and ≈ 1/4 of the appends.  The wave's window tiles (6 × 32 domains from a tile-aligned base, read from L2/MALL) are scored with
// the stream's own MFMA, recomputed per radix step (a greedy bitwise select over the non-negative keys, ballots
// free: each query's two lanes combine their counts by one shuffle).  Returns −∞ when fewer than K window scores
// are ≥ 0.
constexpr int kSeedHalf = 64;
// The table row a query's seed window is centred at: the query's own row, or with a query table of its own (XQ) row
// qrow·seed_stride clamped into the table (there may be more query rows than domains).
template <bool XQ>
__host__ __device__ __forceinline__ int64_t seed_centre(int64_t qrow, const QueryTab& xq, int64_t nd) {
  if constexpr (XQ) {
    const int64_t c = qrow * (int64_t)xq.seed_stride;
    return c < nd ? c : nd - 1;
  } else {
    return qrow;
  }
}
constexpr int kSeedTiles = (2 * kSeedHalf + 62) / 32 + 1;  // the wave's 32 windows from a tile-aligned base
// LEAN (the 4-set centroid geometry, whose prologue holds 4 sets' fragments): the tiles' addresses as wave-uniform
// offsets (wbase is uniform) plus one per-lane index, instead of a 64-bit pointer per tile and lane.
// Probe (launches with an applied floor f, `probe`: wave-uniform): one count at f decides for the whole set whether the
// bit search runs.  The count is monotone in its threshold, so a query with fewer than K window scores ≥ f ends the
// search at a key below f's, its seed key2f(T) − 2δ lies below f, and the caller's max(seed, f) is f; when no live
// lane of the set (`live`: the slot takes appends) counts K, the search is skipped and −∞ returned for all of them,
// else it runs in full and returns what it always did.  The caller's limit is the same bit for bit on every input;
// on white noise almost no set passes the probe.  `searched` is set where the bit search ran.
// Measured (profiles/r09/): cfg2 runs the search for 921 of 31,008 (set, item) pairs, the prologue falls from 4.9 to
// 0.95 % of wave time (no seeds at all: 0.26 %); first pass 10.22 → 9.84 ms (kernel trace, 25 launches), search against
// the previous library, same process, identical candidates, both orders: 330,750 queries 11.34 / 11.39 → 11.00 /
// 11.05 ms, 165,375 6.99 / 7.03 → 6.57 / 6.58, 82,688 4.16 / 4.05 → 4.02 / 3.90, 41,344 2.44 / 2.45 → 2.32 / 2.34;
// never seeding (fwav_debug_topk_seeds(2)) is the ceiling: 330,750 queries 11.55 → 10.87 where the probe gives 11.07.
template <int MODE, bool LEAN = false>
__device__ __forceinline__ float seed_limit(const _Float16* __restrict__ emb16, int64_t nd, half8 b, int64_t qrow,
                                            int64_t wbase, int K, bool probe, float floor, bool live,
                                            bool& searched) {
  const int lane = threadIdx.x & 63;
  const int col = lane & 31;
  const int h = lane >> 5;
  const half8* afp[kSeedTiles];
  uint32_t wm[kSeedTiles];  // per tile: the lane's 16 outputs that are in its query's window (and the table)
#pragma unroll
  for (int t = 0; t < kSeedTiles; ++t) {
    const int64_t dt = wbase + 32 * t;
    const bool ok = dt >= 0 && dt < nd;
    const int64_t c = ok ? dt / kChunk : 0, tt = ok ? (dt % kChunk) / 32 : 0;
    if constexpr (LEAN)
      afp[t] = reinterpret_cast<const half8*>(emb16 + (c * 2 * kChunk) * 8 + tt * 256) + (h * kChunk + col);
    else
      afp[t] = reinterpret_cast<const half8*>(emb16 + ((c * 2 + h) * kChunk + col) * 8 + tt * 256);
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t d = dt + 4 * h + (r & 3) + 8 * (r >> 2);
      m |= (ok && d < nd && d >= qrow - kSeedHalf && d < qrow + kSeedHalf) ? (1u << r) : 0u;
    }
    wm[t] = m;
  }
  auto count_ge = [&](float thr) {
    int c = 0;
    half8 af[kSeedTiles];  // re-read per step (L2): keeps the prologue's register peak below the stream's
#pragma unroll
    for (int t = 0; t < kSeedTiles; ++t) af[t] = *afp[t];
#pragma unroll
    for (int t = 0; t < kSeedTiles; ++t) {
      const floatx16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[t], b, floatx16{}, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) c += ((wm[t] >> r) & 1u) && acc[r] >= thr ? 1 : 0;
    }
    return c + __shfl_xor(c, 32);
  };
  // No per-lane branches here: the MFMAs and shuffles need the whole wave active (a per-lane early return let the
  // compiler run the select loop under a partial EXEC, which corrupts both); the probe's branch is wave-uniform
  // One loop, one call of count_ge (the probe as a call of its own before the search, with a wave-uniform return,
  // compiled the 4-set kernel to 476 B of scratch per lane; this form to 8 B, the search without a probe to 28 B):
  // step 32 is the probe, step 31 tests key 0x80000000 (+0.0: the window holds K scores ≥ 0, else −∞ is
  // returned whatever the later steps find), steps 30 … 12 the bits below it.
  uint32_t T = 0u;
  bool run = true;  // wave-uniform
  for (int bit = probe ? 32 : 31; bit >= 12 && run; --bit) {
    const bool pr = bit == 32;
    const uint32_t Tc = T | (1u << (bit & 31));
    const int c = count_ge(pr ? floor : key2f(Tc));
    if (pr)
      run = __ballot(live && c >= K) != 0ull;
    else
      T = c >= K ? Tc : T;
  }
  searched = run;
  const bool ok = (T & 0x80000000u) != 0u;
  return ok ? (MODE == kModeHL ? key2f(T) - kF16Delta - 2.0f * kHLDelta : key2f(T) - 2.0f * kF16Delta) : -INFINITY;
}

// NC chunks from the LDS slots as a single unrolled software pipeline over their 8·NC tiles: fragments are read
// 3 tiles ahead and each MFMA is issued one tile before its fold, across chunk boundaries (a per-chunk loop waits
// on its first ds_reads and on its last MFMA at every chunk — half the wave time was parked in those waits).
// With QS query sets per wave each fragment read feeds QS MFMAs (set s: B operand b[s]).  Tile t of a chunk
// folds into max chain t % kChains of its set (8 chains: one per tile); at each chunk end one ballot tests the
// chains' maximum, and a firing chunk is recorded in its set's row as (chunk << 8 | chain mask).
// MODE (timing ablations, STATS builds only): 1 = fold but no ballots/records, 2 = MFMA with a 2-output fold
// (one v_max3 per tile instead of 8; results kept alive through `sink`).
template <int NC, int QS, int MODE = 0>
__device__ __forceinline__ void stream_group(const _Float16* __restrict__ lda0, const half8 (&b)[QS],
                                             const int (&thi)[QS], int cbase, uint32_t (*fired)[kFifo],
                                             int (&nfired)[QS], int lane, int* sink = nullptr) {
  constexpr int NT = 8 * NC;
  constexpr int kChunkHalfs = 512 * 8;  // one 8 KB chunk slot
  auto chunk_of = [](int i) { return i >> 3; };
  auto rd = [&](int i) {
    return *reinterpret_cast<const half8*>(lda0 + chunk_of(i) * kChunkHalfs + (i & 7) * 256);
  };
  half8 a[NT];
  floatx16 acc[NT][QS];
#pragma unroll
  for (int i = 0; i < 3 && i < NT; ++i) a[i] = rd(i);
#pragma unroll
  for (int s = 0; s < QS; ++s) acc[0][s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[s], floatx16{}, 0, 0, 0);
  int r[QS][kChains];
#pragma unroll
  for (int s = 0; s < QS; ++s)
#pragma unroll
    for (int c = 0; c < kChains; ++c) r[s][c] = (int)0x80000000;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if (i + 3 < NT) a[i + 3] = rd(i + 3);
#pragma unroll
    for (int s = 0; s < QS; ++s) {
      if (i + 1 < NT) acc[i + 1][s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i + 1], b[s], floatx16{}, 0, 0, 0);
      constexpr int cm = kChains - 1;
      if (MODE & 2)
        r[s][i & cm] = max(max(r[s][i & cm], __float_as_int(acc[i][s][0])), __float_as_int(acc[i][s][15]));
      else
        r[s][i & cm] = fold16(r[s][i & cm], acc[i][s]);
    }
    if (MODE != 0) {
      if (i == NT - 1) {
#pragma unroll
        for (int s = 0; s < QS; ++s)
#pragma unroll
          for (int c = 0; c < kChains; ++c) *sink ^= r[s][c];
      }
      continue;
    }
    if ((i & 7) == 7) {
#pragma unroll
      for (int s = 0; s < QS; ++s) {
        const int t = thi[s];
        // one test of the max of the chains first: most chunks fire none
        int rm = r[s][0];
#pragma unroll
        for (int c = 1; c < kChains; ++c) rm = max(rm, r[s][c]);
        if (__ballot(rm > t) != 0ull) {
          uint32_t mk = 0u;
#pragma unroll
          for (int c = 0; c < kChains; ++c) mk |= __ballot(r[s][c] > t) != 0ull ? (1u << c) : 0u;
          if (lane == 0) fired[s][nfired[s] & (kFifo - 1)] = ((uint32_t)(cbase + chunk_of(i)) << 8) | mk;
          ++nfired[s];
        }
#pragma unroll
        for (int c = 0; c < kChains; ++c) r[s][c] = (int)0x80000000;
      }
    }
  }
}

__device__ __forceinline__ int ctz_mask(uint32_t x) { return __builtin_ctz(x); }
__device__ __forceinline__ int ctz_mask(uint64_t x) { return __builtin_ctzll(x); }
// f(std::integral_constant<int, I>) for I = 0 .. N−1: loops over per-set register arrays with compile-time indices
// where the body is too large for the unroller
template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<N, I + 1>(f);
  }
}

// ---- Centroid pre-filter (CENT geometry): QS query sets of 32 per wave, one centroid per QS consecutive queries.
// Centroid column j of a wave belongs to set j % QS and stands for its members, the columns QS·(j / QS) + k (k < QS)
// of that set — QS consecutive positions of the active list, i.e. (unpruned) ranges a few samples apart, whose
// embeddings lie close together.  With c the centroid's fp16 vector and ρ_h = max over members |q_hi,h − c_h| per
// head h (the tonal and transient halves of the embedding, each of norm ≤ 1 in the table), every member's fp16 score
// obeys s16(q, d) = (q_hi − c)·d_hi + c·d_hi ≤ s16(c, d) + (ρ_0 + ρ_1)(1 + 2⁻⁹) + 1e-5 (d_hi's heads have norm
// ≤ 1 + 2⁻¹¹; both MFMA accumulations ≤ 16 roundings of ≤ 2).  So one MFMA of the 32 centroids per 32-domain tile
// — a 4:1 (QS = 4) reduction of the fold, the stream's issue bound — decides which sets need their own MFMA and fold
// for that tile: a set is scored only where some centroid of it reaches the smallest member threshold minus the
// centroid's slack.  Exact: a tile skipped for a set holds no domain above any member's threshold.
constexpr int kCentBatch = FWAV_TOPK_CB;
template <int QS>
__device__ __forceinline__ uint64_t cent_set_mask(int s) {
  static_assert(QS == 2 || QS == 4 || QS == 8, "centroid sets: 2, 4 or 8 query sets per wave");
  constexpr uint64_t m = QS == 2 ? 0x5555555555555555ull : (QS == 4 ? 0x1111111111111111ull : 0x0101010101010101ull);
  return m << s;
}
// The lane's centroid (column col = lane & 31, half h = lane >> 5): the fp16 mean of its members' query fragments and
// the constants of its filter threshold (fwav_centroid_bound.h: the worst-case slack (ρ_0 + ρ_1)(1 + 2⁻⁹) + 1e-5 and
// the score-dependent bound's Γ·D + η, 2σ²D², σ²/N²).  `qrow_of(k)` = member k's table row, or −1.
template <int QS, class RowOf>
__device__ __forceinline__ void centroid_setup(const _Float16* __restrict__ emb16, RowOf qrow_of, half8& bc,
                                               CentBound& cb) {
  typedef float floatx8 __attribute__((ext_vector_type(8)));
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5;
  auto frag = [&](int64_t r) {  // the member's fp16 high parts of head h (re-read from L2 in the second pass)
    return *reinterpret_cast<const half8*>(emb16 + (((r >> 8) * 2 + h) * 256 + (r & 255)) * 8);
  };
  floatx8 sum = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int nv = 0;
#pragma unroll
  for (int k = 0; k < QS; ++k) {
    const int64_t r = qrow_of(k);
    if (r >= 0) {
      const half8 m = frag(r);
      ++nv;
#pragma unroll
      for (int i = 0; i < 8; ++i) sum[i] += (float)m[i];
    }
  }
  half8 c;
  float cf[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c[i] = (_Float16)(nv > 0 ? sum[i] / (float)nv : 0.0f);
    cf[i] = (float)c[i];
  }
  CentHead own;  // this lane's head ...
  cent_head_begin(own, cf);
#pragma unroll
  for (int k = 0; k < QS; ++k) {
    const int64_t r = qrow_of(k);
    if (r >= 0) {
      const half8 m = frag(r);
      float mf[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) mf[i] = (float)m[i];
      cent_head_member(own, cf, mf);
    }
  }
  // ... and the other one's (the constants are symmetric in the heads: both lanes of a column get the same)
  const CentHead oth{__shfl_xor(own.n2, 32), __shfl_xor(own.rho, 32), __shfl_xor(own.beta, 32),
                     __shfl_xor(own.perp2, 32)};
  bc = c;
  cb = cent_bound(own, oth);
}
// The lane's centroid filter threshold from the smallest stream threshold (float) of its members (+∞ when no member
// takes appends; −∞ members make the centroid fire on every tile).  `tight` = false: the worst-case slack alone.
template <int QS>
__device__ __forceinline__ int centroid_threshold(const float (&tv)[QS], const CentBound& cb, bool tight) {
  int lane = threadIdx.x & 63;
  // (4 sets: the shuffle addresses computed here, where a limit moved, not held in VGPRs across the whole stream)
  if constexpr (QS >= 4) asm volatile("" : "+v"(lane));
  const int col = lane & 31;
  const int sj = col % QS, base = (lane & 32) + QS * (col / QS);
  float mn = INFINITY;
#pragma unroll
  for (int k = 0; k < QS; ++k) {
    float v = INFINITY;
#pragma unroll
    for (int s = 0; s < QS; ++s) {
      const float x = __shfl(tv[s], base + k);
      v = s == sj ? x : v;
    }
    mn = fminf(mn, v);
  }
  return int_threshold(cent_threshold(cb, mn, tight));
}
// Level 1 of the centroid pre-filter over one group of NC chunks: the 32 centroids scored against every tile (the
// stream's software pipeline: fragments 3 tiles ahead, MFMAs one tile ahead); pend[s] bit i marks tile i of the group
// where some centroid of set s reaches its threshold.  The marked (tile, set) pairs are then scored with the set's
// own queries and their survivors appended at once (k_sim_topk_f16, CENT): no fired-chunk ring, no replay.
template <int NC, int QS>
__device__ __forceinline__ void cent_level1(const _Float16* __restrict__ lda0, half8 bc, int thc,
                                            uint64_t (&pend)[QS]) {
  constexpr int NT = 8 * NC;
  static_assert(NT <= 64, "tile masks are 64-bit");
  constexpr int kChunkHalfs = 512 * 8;
  auto rd = [&](int i) {
    return *reinterpret_cast<const half8*>(lda0 + (i >> 3) * kChunkHalfs + (i & 7) * 256);
  };
#pragma unroll
  for (int s = 0; s < QS; ++s) pend[s] = 0ull;
  half8 a[NT];
  floatx16 acc[NT];
#pragma unroll
  for (int i = 0; i < 3 && i < NT; ++i) a[i] = rd(i);
  acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], bc, floatx16{}, 0, 0, 0);
if constexpr (NT <= 32) {
  // the lane's firing tiles accumulated in a VGPR (bits = 2·bits + fired, one v_addc per tile: tile i at bit NT−1−i),
  // then OR-reduced over the lanes of each set once per group — instead of 4 scalar ops per set and tile
  uint32_t bits = 0u;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if (i + 3 < NT) a[i + 3] = rd(i + 3);
    if (i + 1 < NT) acc[i + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i + 1], bc, floatx16{}, 0, 0, 0);
    const uint64_t m = __ballot(fold16((int)0x80000000, acc[i]) > thc);
    uint64_t co;
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(bits), "=s"(co) : "v"(bits), "s"(m));
  }
  if constexpr (QS == 4) {
    // OR over the lanes of each set without shuffle addresses (VGPRs held across the stream): two row rotations
    // (DPP row_ror:4, :8) leave lane s of every 16-lane row with its row's OR for set s, and the four rows meet in
    // scalar registers
    bits |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits, 0x124, 0xf, 0xf, false);
    bits |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)bits, 0x128, 0xf, 0xf, false);
#pragma unroll
    for (int s = 0; s < QS; ++s) {
      const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)bits, s) |
                         (uint32_t)__builtin_amdgcn_readlane((int)bits, 16 + s) |
                         (uint32_t)__builtin_amdgcn_readlane((int)bits, 32 + s) |
                         (uint32_t)__builtin_amdgcn_readlane((int)bits, 48 + s);
      pend[s] = (uint64_t)(__builtin_bitreverse32(m) >> (32 - NT));
    }
  } else {
#pragma unroll
    for (int off = QS; off < 64; off <<= 1) bits |= (uint32_t)__shfl_xor((int)bits, off);
#pragma unroll
    for (int s = 0; s < QS; ++s)
      pend[s] = (uint64_t)(__builtin_bitreverse32((uint32_t)__builtin_amdgcn_readlane((int)bits, s)) >> (32 - NT));
  }
} else {  // (the wide geometry's 64-tile groups: scalar masks per set)
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if (i + 3 < NT) a[i + 3] = rd(i + 3);
    if (i + 1 < NT) acc[i + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i + 1], bc, floatx16{}, 0, 0, 0);
    const uint64_t m = __ballot(fold16((int)0x80000000, acc[i]) > thc);
#pragma unroll
    for (int s = 0; s < QS; ++s)
      if (m & cent_set_mask<QS>(s)) pend[s] |= 1ull << i;
  }
}
}

// XQ: the queries come from a table of their own (QueryTab xq: the _q entry points) instead of the domain table's
// rows; everything read from the table — the stream, the seeds' tiles, the rescoring rows — is the same.  A separate
// instantiation, so that the plain search's code is what it was without the option.
template <int C, bool STATS, int MODE, int W = k16Waves, int G = kGroup, int QS = k16Sets, bool CENT = false,
          bool XQ = false>
__global__ __launch_bounds__(64 * W, MODE == kModeEX ? kExactWavesPerSimd : (CENT ? kCentWavesPerSimd : kWavesPerSimd)) void k_sim_topk_f16(const _Float16* __restrict__ emb16,
                                                                const float* __restrict__ emb, int64_t nd,
                                                                const int32_t* __restrict__ active,
                                                                const int32_t* __restrict__ n_active_p,
                                                                int64_t q_offset, int K, int32_t* __restrict__ cand,
                                                                uint64_t* __restrict__ gkeys_all,
                                                                int32_t* __restrict__ ovf_list,
                                                                int32_t* __restrict__ n_ovf,
                                                                uint32_t* __restrict__ share_lim,
                                                                const uint32_t* __restrict__ seeds_in,
                                                                float seed_shift, int plan_rt,
                                                                int plan_p, int dbg, unsigned long long* gstats,
                                                                SgemvSplit sp, int32_t* __restrict__ ties,
                                                                FloorCtl fl, QueryTab xq) {
  constexpr bool EX = MODE == kModeEX;
  constexpr bool HL = MODE == kModeHL;
  constexpr int NG = W * QS;  // query groups of 32 per workgroup; wave w owns groups w·QS .. w·QS + QS − 1
  constexpr bool ABL = STATS || FWAV_TOPK_ABL != 0;  // ablation bits honoured
  // 2 × G chunk slots: group g is consumed from one half while group g+1 streams into the other.
  // ALL of the kernel's LDS is one __shared__ object: beside a second one, hipcc waits vmcnt(0) for the in-flight
  // LDS DMA before the first ds_read of every chunk (cdna_hip_programming.md, "three .s-level traps" (a)).
  // (Measured and rejected, tools/experiments/ring_and_knobs.patch: a ring of NB slots with LDS ready/free counters
  // instead of the group barrier)
  constexpr int NB = 2;
  // COLD (the centroid geometry from 4 sets per wave on): the per-set state that level 1 does not read — buffer
  // counts, `kept`, the list positions — stays in the wave's LDS rows (Topk16SmemColdT), so that level 1 carries only
  // b[s], thf[s] and the centroid's constants: 4 sets fit the 128-VGPR budget of 4 waves per SIMD with no scratch
  // access in the stream loop
  constexpr bool COLD = CENT && QS >= 4;
  static_assert(!COLD || !EX, "exact mode keeps its tie row (Topk16SmemT)");
  using SM = std::conditional_t<COLD, Topk16SmemColdT<NG, STATS, W>, Topk16SmemT<NG, STATS, !CENT, W>>;
  struct Lds {
    u32x4 slots[NB * G][512];
    SM sm;
  };
  __shared__ __attribute__((aligned(16))) Lds lds_all;
  u32x4(*slots)[512] = lds_all.slots;
  SM& sm = lds_all.sm;

  const int n_active = *n_active_p;
  constexpr int QB = 32 * NG;  // queries per block
  // a first pass's speculative floor (FloorCtl): every band limit starts there; none applied → the floor-free plan
  const uint32_t fkey = (!EX && fl.key != nullptr) ? __builtin_amdgcn_readfirstlane(*fl.key) : 0u;
  const bool alt = fl.key != nullptr && fkey == 0u;
  const TopkPlan plan = make_plan(n_active, alt ? fl.alt_rt : plan_rt, alt ? fl.alt_p : plan_p, QB);
  int64_t block;
  int piece, npieces, qhalf;
  plan_item(plan, blockIdx.x, block, piece, npieces, qhalf);
  if (block >= plan.nb) return;
  const int Wact = qhalf < 0 ? W : W / 2;  // waves with queries
  if ((int)(threadIdx.x >> 6) >= Wact) return;
  const int qslot0 = qhalf > 0 ? (W / 2) * QS * 32 : 0;  // the second half block's first query slot
  uint64_t* gkeys = gkeys_all + (size_t)blockIdx.x * 32 * NG * C;  // this item's key-buffer region
  const unsigned long long t_kernel = STATS ? __builtin_amdgcn_s_memrealtime() : 0;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably uniform: scalar control flow below
  unsigned long long* stats = nullptr;
  if (STATS) {
    if (lane < kStatsX) sm.wstat[wave][lane] = 0;
    stats = sm.wstat[wave];
  }
  const int col = lane & 31;
  const int h = lane >> 5;
  // dbg (STATS builds only; timing ablations, outputs invalid): 1 = never take the slow path,
  // 2 = skip MFMA + threshold test, 4 = no global chunk loads, 128 = DMA only every other chunk,
  // 256 = no group barrier, 512 = fold without ballots, 1024 = MFMA without fold, 4096 = record the workgroup
  // timeline (combinable with the others), 8192 = no seeded band limits; 2048 = the centroid filter with its
  // worst-case slack alone (outputs valid: the A/B of the score-dependent bound); 64 = the prologue's
  // counters at gstats[16 .. 19], the seed dump and the timeline from gstats[32] on (outputs valid)
  if (!STATS) dbg = FWAV_TOPK_ABL;  // production: 0; ablation builds (-DFWAV_TOPK_ABL=bits) fix the bits at compile time
  half8 b[QS], bl[QS];  // the query's fp16 high and low parts (MFMA B operands)
  float thf[QS];        // band limit: on shl (first pass), on s16 (exact mode)
  int upd[QS];
  float qv[QS][EX ? 16 : 1];  // EX: the exact query vector (sgemv16 keys)
  const int64_t n16 = (int64_t)cdiv(nd, kChunk) * kChunk * 16;  // halfs per fp16 table
  const _Float16* emb16lo = emb16 + n16;
  // where the queries are read: their f32 rows and fp16 high and low parts
  const float* const qemb = XQ ? xq.emb : emb;
  const _Float16* const q16 = XQ ? xq.hi : emb16;
  const _Float16* const q16lo = XQ ? xq.lo : emb16lo;
  uint64_t kth[QS];           // EX: the query's current K-th exact key (0 until K entries)
  float inseed[QS];           // relaunch: the previous pass's band limit at overflow, in this mode's scale
  int32_t qpos[QS];           // the slot's query position in the active list
  // Table pieces of one query block share their band limits: a piece's compaction limit is a valid lower bound for
  // the whole query (K domains of its own chunk range beat it), so every piece filters with the largest limit any
  // piece has found (atomicMax on the f2key, read back at window ends) instead of restarting its own rise.
  uint32_t* share = (npieces > 1 && !EX) ? share_lim : nullptr;
#pragma unroll
  for (int s = 0; s < QS; ++s) {
    const int ql = (wave * QS + s) * 32 + col;
    const int64_t qi = slot_query(block, qslot0 + ql, plan.nb);
    const int32_t q = qi < n_active ? active[qi] : -1;
    const int64_t qrow = (int64_t)(q < 0 ? 0 : q) + q_offset;
    // (COLD loads b[s] with the set's seed, below: the seed of set s runs with s + 1 fragments held, not all QS)
    if constexpr (!COLD)
      b[s] = *reinterpret_cast<const half8*>(q16 + (((qrow >> 8) * 2 + h) * 256 + (qrow & 255)) * 8);
    bl[s] = *reinterpret_cast<const half8*>(q16lo + (((qrow >> 8) * 2 + h) * 256 + (qrow & 255)) * 8);
    upd[s] = (q >= 0 && !(dbg & 1)) ? 1 : 0;
    thf[s] = upd[s] ? -INFINITY : INFINITY;  // slots past n_active never take appends
    qpos[s] = (int32_t)(qi < n_active ? qi : 0);
    if constexpr (COLD) {
      if (h == 0) {
        sm.ovf[ql] = 0;
        sm.qpos[ql] = qpos[s];
        sm.cnt[ql] = 0;
        sm.kept[ql] = 0;
      } else {
        sm.cnt1[ql] = 0;
      }
    } else if (h == 0) {
      sm.ovf[ql] = 0;
      sm.tie[ql] = 0;
      sm.qrow[ql] = qrow;
      sm.qpos[ql] = qpos[s];
    }
    kth[s] = 0ull;
    // relaunch: active = the previous pass's overflow list, whose position qi holds this query's seed (that pass's
    // band limit); seed_shift converts it to this mode's scale (S16 → HL: −(δ + 2δ'); HL → EX: −(δ + 2δ'))
    // (COLD reads it where it is applied, below: nothing held through the seeds' MFMAs)
    inseed[s] = !COLD && seeds_in != nullptr && q >= 0 ? key2f(seeds_in[qi]) - seed_shift : -INFINITY;
    if constexpr (EX) {
      const float* qp = qemb + qrow * 16;
#pragma unroll
      for (int i = 0; i < 16; ++i) qv[s][i] = qp[i];
    }
  }

  // seed the band limits from the queries' own domain windows (tiles from the wave's first query row; XQ: from the
  // window of table rows around seed_centre of the query's row — any K in-table rows give a valid limit)
  // (the debug library's fwav_debug_topk_seeds: 1 = the bit search for every set, floor or not; 2 = no seeds)
  const int seed_mode = kSeedKnob ? fl.seeds : 0;
  const bool no_seed = (ABL && (dbg & 8192)) || seed_mode == 2;  // ablation 8192: no seed
  const bool probe = fkey != 0u && seed_mode != 1;
  const unsigned long long t_seed = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
  if (COLD || !no_seed) {
#pragma unroll
    for (int s = 0; s < QS; ++s) {
      // whole wave (MFMA + shuffles); lanes of unused query slots discard the result
      int64_t qrow_s;
      int qrow_0;  // the set's first slot's row (lane 0 holds it)
      if constexpr (COLD) {  // (read again from the active list: not held through the other sets' seeds)
        const int64_t qi = slot_query(block, qslot0 + (wave * QS + s) * 32 + col, plan.nb);
        const int32_t q = qi < n_active ? active[qi] : -1;
        const int64_t qrow_q = (int64_t)(q < 0 ? 0 : q) + q_offset;
        qrow_s = seed_centre<XQ>(qrow_q, xq, nd);
        qrow_0 = __builtin_amdgcn_readfirstlane((int)qrow_s);
        b[s] = *reinterpret_cast<const half8*>(q16 + (((qrow_q >> 8) * 2 + h) * 256 + (qrow_q & 255)) * 8);
        if (no_seed) continue;
      } else {
        qrow_s = seed_centre<XQ>(sm.qrow[(wave * QS + s) * 32 + col], xq, nd);
        qrow_0 = __builtin_amdgcn_readfirstlane((int)seed_centre<XQ>(sm.qrow[(wave * QS + s) * 32], xq, nd));
      }
      const int64_t wbase = (int64_t)((qrow_0 - kSeedHalf) >> 5) << 5;
      // (COLD keeps no upd[]: a slot that takes no appends has thf = +∞)
      const bool live = COLD ? thf[s] != INFINITY : upd[s] != 0;
      bool searched;
      const float seed = seed_limit<MODE, COLD>(emb16, nd, b[s], qrow_s, wbase, K, probe, key2f(fkey), live, searched);
      if (live) thf[s] = seed;
      if (STATS) stat_add(18, searched ? 1 : 0);
      if (STATS && (dbg & 32768) && gstats != nullptr && h == 0 && upd[s])  // diagnostics: the seeds
        gstats[((dbg & 64) ? 2 * kStats : kStats) + slot_query(block, qslot0 + (wave * QS + s) * 32 + col, plan.nb)] =
            __float_as_uint(seed);
    }
  }
  if (STATS) stat_add(17, __builtin_amdgcn_s_memrealtime() - t_seed);
  if (seeds_in != nullptr) {
#pragma unroll
    for (int s = 0; s < QS; ++s) {
      if constexpr (COLD) {
        const int64_t qi = slot_query(block, qslot0 + (wave * QS + s) * 32 + col, plan.nb);
        if (qi < n_active) thf[s] = fmaxf(thf[s], key2f(seeds_in[qi]) - seed_shift);  // (+∞ stays +∞)
      } else if (upd[s]) {
        thf[s] = fmaxf(thf[s], inseed[s]);
      }
    }
  }
  if (fkey != 0u) {
#pragma unroll
    for (int s = 0; s < QS; ++s)
      if (COLD || upd[s]) thf[s] = fmaxf(thf[s], key2f(fkey));
  }
  // the query sets this wave works on: set position s holds logical set lid[s] (its slots lid[s]·32 + col, its key
  // buffers and LDS rows) — wave w's own sets w·QS + s (dealing sets to other waves between groups by their recent
  // work measured slower: tools/experiments/set_repairing.patch)
  int lid[QS];
#pragma unroll
  for (int s = 0; s < QS; ++s) lid[s] = wave * QS + s;
  half8 bc{};          // CENT: the lane's centroid (fp16, MFMA B operand) ...
  CentBound cb{};     // ... and its filter threshold's constants
  auto setup_centroids = [&]() {
    const int sj = col % QS, mcol0 = QS * (col / QS);
    int ls = lid[0];
#pragma unroll
    for (int s = 1; s < QS; ++s) ls = sj == s ? lid[s] : ls;
    if constexpr (COLD) ls = wave * QS + sj;  // (the select chain over 4 sets became a table in scratch)
    centroid_setup<QS>(q16, [&](int k) -> int64_t {
      const int64_t qi = slot_query(block, qslot0 + ls * 32 + mcol0 + k, plan.nb);
      return qi < n_active ? (int64_t)active[qi] + q_offset : (int64_t)-1;
    }, bc, cb);
  };
  if constexpr (CENT) setup_centroids();
  const int nchunks = (int)cdiv(nd, kChunk);  // < 2^31 / 256: chunk arithmetic stays 32-bit (scalar)
  // this item's chunk range [c0, c1) (the whole table unless the block is split)
  int c0, c1;
  piece_chunks(plan, block, piece, npieces, nchunks, c0, c1);
  const int ngroups = (c1 - c0 + G - 1) / G;
  const u32x4* src = reinterpret_cast<const u32x4*>(emb16);
  // Chunk stream: global → LDS directly (global_load_lds_dwordx4: no staging registers, no ds_write).  The
  // destination of one wave-instruction is wave-uniform base + lane × 16 B, which is exactly the slot layout
  // (thread t ↔ bytes [16t, 16t + 16) of the 8 KB chunk).  Chunks past the end re-read the last one (never
  // consumed).  Group g+1 is issued right after the barrier that retires group g and frees its half.
  auto issue_group = [&](int gg) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      int c_ = c0 + gg * G + j;
      c_ = c_ < c1 ? c_ : c1 - 1;
      if (ABL && (dbg & 4)) c_ = 0;  // ablation: no streaming traffic beyond one L2-resident chunk
      if (ABL && (dbg & 128) && (j & 1)) continue;  // ablation: DMA only every other chunk
      // the chunk's 8 KB = 8 wave-instructions of 64 × 16 B, dealt round-robin over the active waves
      for (int k = wave; k < 8; k += Wact) {
        // inline asm, not the builtin: hipcc would otherwise wait for this DMA (vmcnt(0)) before every ds_read
        // of the other half; completion is counted by hand at the group top
        const unsigned lds_dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(
            (__attribute__((address_space(3))) void*)(&slots[(gg % NB) * G + j][k * 64])));
        const u32x4* gsrc = src + (int64_t)c_ * 512 + k * 64 + lane;
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
      }
    }
  };
  // retire the prologue's ordinary loads (query fragments, active list) before the stream, visibly to hipcc
  // (a load still pending at the loop head is waited on, vmcnt(0), inside every chunk iteration)
  __builtin_amdgcn_s_waitcnt(0x0F70);
  if (STATS) stat_add(16, __builtin_amdgcn_s_memrealtime() - t_kernel);
  if (ngroups > 0) issue_group(0);

  int sink = 0;     // ablation builds: keeps the MFMA / fold results of dbg 512/1024 alive
  int nfired[QS];  // wave-uniform FIFO tail: chunks recorded in sm.fired[group] so far
  ReplayCursor cur[QS];
  int qcnt[QS];    // this lane's entries in its query's two-ended buffer (h = 0: front, h = 1: back)
  int kept[QS];    // the query's buffer size after its last compaction
#pragma unroll
  for (int s = 0; s < QS; ++s) {
    nfired[s] = qcnt[s] = kept[s] = 0;
    cur[s] = ReplayCursor{0, 0, 0u};
  }
  // CENT: the pieces' shared limits, loaded before each group's top wait and applied before the next group's DMA is
  // issued.  (Read after that issue, as rounds 4–5 did, the compiler's wait for the loaded value, vmcnt(0), also
  // waited for the whole next group's DMA: every group's level 1 started only once the group after it had landed.)
  uint32_t shv[QS];
  // CENT: the lane's filter threshold, recomputed only after a group in which some limit of the wave moved (a
  // compaction or a piece's shared limit; cfg2: 0.57 compactions per query over a pass of 1,291 groups)
  int thc = 0;
  bool thc_stale = true;
  for (int g = 0; g < ngroups; ++g) {
    u32x4(*half)[512] = slots + (g % NB) * G;
    const int cg = c0 + g * G;  // first chunk of group g
    const int c_end = cg + G < c1 ? cg + G : c1;
    const bool window_end =
        (c_end - c0 <= kWarmChunks) || ((g + 1) % (kWindowGroups * 4 / G) == 0) || (g + 1 == ngroups);
    if (CENT && share != nullptr) {
#pragma unroll
      for (int s = 0; s < QS; ++s) {
        int32_t qp = qpos[s];
        if constexpr (COLD) qp = sm.qpos[(wave * QS + s) * 32 + col];
        shv[s] = __hip_atomic_load(share + qp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    const unsigned long long t_b0 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
    // RAW: own DMA of group g retired, then every wave's (barrier).  WAR: the other half was last read in
    // iteration g−1, whose ds_reads were all consumed before its waves reached this barrier.
    if (!(ABL && (dbg & 256))) {  // ablation 256: no group barrier (LDS races; timing only)
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      if (STATS) stat_add(12, __builtin_amdgcn_s_memrealtime() - t_b0);
      __builtin_amdgcn_s_setprio(0);
      if (!(ABL && (dbg & 16384))) __builtin_amdgcn_s_barrier();  // 16384: own DMA wait, no barrier
      asm volatile("" ::: "memory");
    }
    const unsigned long long t_b1 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
    if (STATS) stat_add(7, t_b1 - t_b0);
    if (CENT && share != nullptr) {
      // CENT: the pieces' shared limits every group (a filter threshold that rises sooner skips more level-2 work),
      // retired by the wait above
#pragma unroll
      for (int s = 0; s < QS; ++s) {
        const float t0 = thf[s];
        // (COLD keeps no upd[]: a slot that takes no appends has thf = +∞, which no limit moves)
        if ((COLD || upd[s]) && shv[s] != 0u) thf[s] = fmaxf(thf[s], key2f(shv[s]));
        thc_stale |= __ballot(thf[s] != t0) != 0ull;
      }
    }
    // (the DMA issued after level 1 or level 2 instead measured no better: profiles/r04/ab_prefix_dma_barrier.log)
    if (g + 1 < ngroups) issue_group(g + 1);
    if (ABL && (dbg & 2)) continue;
    int thi[QS];
#pragma unroll
    for (int s = 0; s < QS; ++s) thi[s] = int_threshold(HL ? thf[s] - kStreamMargin : thf[s]);
    const _Float16* lda0 = reinterpret_cast<const _Float16*>(half[0]) + ((h * kChunk) + col) * 8;
    if constexpr (CENT) {
      if (thc_stale) {
        float tv[QS];
#pragma unroll
        for (int s = 0; s < QS; ++s) tv[s] = HL ? thf[s] - kStreamMargin : thf[s];
        thc = centroid_threshold<QS>(tv, cb, !(ABL && (dbg & 2048)));
        thc_stale = false;
      }
      uint64_t pend[QS];
      const unsigned long long t_l1 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
      if (c_end - cg == G) {
        cent_level1<G, QS>(lda0, bc, thc, pend);
      } else {
#pragma unroll
        for (int s = 0; s < QS; ++s) pend[s] = 0ull;
        for (int c = cg; c < c_end; ++c) {
          uint64_t pc[QS];
          cent_level1<1, QS>(lda0 + (c - cg) * 512 * 8, bc, thc, pc);
#pragma unroll
          for (int s = 0; s < QS; ++s) pend[s] |= pc[s] << (8 * (c - cg));
        }
      }
      if (STATS) {
        stat_add(13, __builtin_amdgcn_s_memrealtime() - t_l1);
        unsigned long long np = 0;
#pragma unroll
        for (int s = 0; s < QS; ++s) np += __popcll(pend[s]);
        stat_add(14, np);
      }
      __builtin_amdgcn_s_setprio(1);
      // level 2: the marked (tile, set) pairs scored with the set's queries, kCentBatch at a time (their fragments and
      // MFMAs in flight together).  S16: survivors appended at once.  HL: the pairs whose s16 can pass are collected
      // first, then refined in batches of kReplayBatch with their low-part fragments fetched from L2 together (one
      // memory round trip per batch, as the base geometry's replays) and appended.
      static_for<QS>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        using TMask = uint64_t;  // (32-bit masks for ≤ 32-tile groups: 17.15 vs 16.88 ms)
        TMask pm = (TMask)pend[s];
        TMask pass = 0;  // HL: tiles whose s16 passes the set's stream threshold
        // COLD: the set's buffer counts come from its LDS rows for the time its marked pairs are scored
        // (its row index from an opaque lane id: computed here, not held in VGPRs across level 1)
        int qc_l = 0, kp_l = 0, ci = 0;
        if constexpr (COLD) {
          if (pm != 0) {
            int li = lane;
            asm volatile("" : "+v"(li));
            ci = (wave * QS + s) * 32 + (li & 31);
            qc_l = sm.cnt01[(li >> 5) * 32 * NG + ci];
            kp_l = sm.kept[ci];
          }
        }
        int& qc = COLD ? qc_l : qcnt[s];
        int& kp = COLD ? kp_l : kept[s];
        const int up = COLD ? 1 : upd[s];  // (a slot without appends has thf = +∞)
        while (pm != 0) {
          int t[kCentBatch];
          bool on[kCentBatch];
#pragma unroll
          for (int u = 0; u < kCentBatch; ++u) {
            on[u] = pm != 0;
            t[u] = on[u] ? ctz_mask(pm) : t[0];
            if (on[u]) pm &= pm - 1;
          }
          half8 af[kCentBatch];
          floatx16 acc[kCentBatch];
#pragma unroll
          for (int u = 0; u < kCentBatch; ++u)
            af[u] = *reinterpret_cast<const half8*>(lda0 + (t[u] >> 3) * (512 * 8) + (t[u] & 7) * 256);
#pragma unroll
          for (int u = 0; u < kCentBatch; ++u)
            acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[u], b[s], floatx16{}, 0, 0, 0);
#pragma unroll
          for (int u = 0; u < kCentBatch; ++u) {
            if (!on[u]) break;
            if constexpr (HL) {
              if (__ballot(fold16((int)0x80000000, acc[u]) > thi[s]) != 0ull) pass |= (TMask)1 << t[u];
            } else {
              const int64_t dt = (int64_t)(cg + (t[u] >> 3)) * kChunk + (t[u] & 7) * 32;
              const float t0 = thf[s];
              thf[s] = append_tile<C, STATS, SM, MODE>(acc[u], thf[s], qc, kp, dt, nd, gkeys, sm, lid[s], K, up, stats,
                                                       sp, emb, qv[s], &kth[s], share);
              thc_stale |= __ballot(thf[s] != t0) != 0ull;
            }
          }
        }
        if constexpr (HL) {  // shl = s16 + d_hi·q_lo + d_lo·q_hi for the passing tiles, batched
          while (pass != 0) {
            int t[kReplayBatch];
            bool on[kReplayBatch];
#pragma unroll
            for (int u = 0; u < kReplayBatch; ++u) {
              on[u] = pass != 0;
              t[u] = on[u] ? ctz_mask(pass) : t[0];
              if (on[u]) pass &= pass - 1;
            }
            half8 afl[kReplayBatch];
#pragma unroll
            for (int u = 0; u < kReplayBatch; ++u)
              afl[u] = tile_fragment(emb16lo, (int64_t)(cg + (t[u] >> 3)) * kChunk + (t[u] & 7) * 32, h, col);
#pragma unroll
            for (int u = 0; u < kReplayBatch; ++u) {
              if (!on[u]) break;
              const half8 af = *reinterpret_cast<const half8*>(lda0 + (t[u] >> 3) * (512 * 8) + (t[u] & 7) * 256);
              floatx16 a2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, b[s], floatx16{}, 0, 0, 0);
              a2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bl[s], a2, 0, 0, 0);
              a2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(afl[u], b[s], a2, 0, 0, 0);
              const int64_t dt = (int64_t)(cg + (t[u] >> 3)) * kChunk + (t[u] & 7) * 32;
              const float t0 = thf[s];
              thf[s] = append_tile<C, STATS, SM, MODE>(a2, thf[s], qc, kp, dt, nd, gkeys, sm, lid[s], K, up, stats, sp,
                                                       emb, qv[s], &kth[s], share);
              thc_stale |= __ballot(thf[s] != t0) != 0ull;
            }
          }
        }
        if constexpr (COLD) {
          if (pend[s] != 0ull) {
            sm.cnt01[h * 32 * NG + ci] = (uint16_t)qc_l;
            sm.kept[ci] = (uint16_t)kp_l;  // (both lanes of a query hold the same)
          }
        }
      });
    } else if (ABL && (dbg & (512 | 1024)) && c_end - cg == G) {
      // ablations 512: fold without ballots, 1024: MFMA without fold (outputs invalid)
      if (dbg & 1024)
        stream_group<G, QS, 2>(lda0, b, thi, cg, sm.fired + wave * QS, nfired, lane, &sink);
      else
        stream_group<G, QS, 1>(lda0, b, thi, cg, sm.fired + wave * QS, nfired, lane, &sink);
    } else if (c_end - cg == G) {
      stream_group<G, QS>(lda0, b, thi, cg, sm.fired + wave * QS, nfired, lane);
    } else {
      for (int c = cg; c < c_end; ++c)
        stream_group<1, QS>(lda0 + (c - cg) * 512 * 8, b, thi, c, sm.fired + wave * QS, nfired, lane);
    }
    const unsigned long long t_c = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
    if (STATS) stat_add(9, t_c - t_b1);
    if (window_end) {
      // the largest limit the query's pieces have published (CENT reads it every group, above)
      if (share != nullptr && !CENT) {
#pragma unroll
        for (int s = 0; s < QS; ++s) {
          const uint32_t v = __hip_atomic_load(share + qpos[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (upd[s] && v != 0u) thf[s] = fmaxf(thf[s], key2f(v));
        }
      }
      // each wave replays its own fired chunks (compacting inline when a buffer fills); compile-time set indices
      // (static_for): a runtime-indexed per-set array would live in scratch / LDS
      if (!CENT) __builtin_amdgcn_s_setprio(1);
      static_for<QS>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        if constexpr (!CENT) {
          if (nfired[s] > cur[s].head || cur[s].rem != 0u)
            thf[s] = replay_window<C, STATS, SM, MODE>(emb16, emb16lo, b[s], bl[s], thf[s],
                                             qcnt[s], kept[s], cur[s], nfired[s], nd, gkeys, sm, lid[s], K, upd[s],
                                             stats, sp, emb, qv[s], &kth[s], share);
        }
      });
      if (!CENT) __builtin_amdgcn_s_setprio(0);
      if (STATS) stat_add(4, __builtin_amdgcn_s_memrealtime() - t_c);
      // retire the replay's loads and stores here, visibly to hipcc's wait bookkeeping (vmcnt(0) expcnt(7)
      // lgkmcnt(15)): otherwise it keeps them "pending" at the loop head and waits on them before the next
      // chunk's ds_reads — which, at run time, also drains the in-flight chunk DMA
      __builtin_amdgcn_s_waitcnt(0x0F70);
    }
  }
  const unsigned long long t_final = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
  // the final pass reads the counts from LDS (same wave: program order)
  if constexpr (!COLD) {  // (COLD: they are there already)
#pragma unroll
    for (int s = 0; s < QS; ++s) {
      if (h == 0)
        sm.cnt[lid[s] * 32 + col] = qcnt[s];
      else
        sm.cnt1[lid[s] * 32 + col] = qcnt[s];
    }
  }

  auto slot_of = [&](int l) {  // the wave's l-th query slot
    if constexpr (COLD) return wave * QS * 32 + l;
    int ls = lid[0];
#pragma unroll
    for (int s = 1; s < QS; ++s) ls = (l >> 5) == s ? lid[s] : ls;
    return ls * 32 + (l & 31);
  };
  if (npieces > 1) {
    // a table piece hands each query's filtered band to k_merge_pieces: kBandBatch queries' keys and shared limits
    // loaded together (the wave's own appends drained once)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int l0 = 0; l0 < 32 * QS; l0 += kBandBatch) {
      uint64_t v[kBandBatch][C / 64];
      int nb_[kBandBatch];
      uint32_t sh[kBandBatch];
#pragma unroll
      for (int b = 0; b < kBandBatch; ++b) {
        const int qs = slot_of(l0 + b);
        const int64_t qq = slot_query(block, qslot0 + qs, plan.nb);
        const bool ok = l0 + b < 32 * QS && qq < n_active;
        nb_[b] = ok ? piece_band_load<C>(gkeys + (size_t)qs * C, sm, qs, v[b]) : -1;
        sh[b] = ok ? __hip_atomic_load(share_lim + qq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      }
#pragma unroll
      for (int b = 0; b < kBandBatch; ++b) {
        if (nb_[b] < 0) continue;
        const int qs = slot_of(l0 + b);
        const int64_t qq = slot_query(block, qslot0 + qs, plan.nb);
        piece_band<C, HL>(gkeys + (size_t)qs * C, sm, qs, K, share_lim + qq, v[b], nb_[b], sh[b]);
      }
    }
  }
  for (int l = 0; l < (npieces > 1 ? 0 : 32 * QS); ++l) {
    const int qs = slot_of(l);
    const int64_t qq = slot_query(block, qslot0 + qs, plan.nb);
    if (qq >= n_active) continue;
    const int32_t qid = active[qq];
    uint64_t* kq = gkeys + (size_t)qs * C;
    // exact f32 rescoring of the kept band + sort
    int64_t qrow;
    if constexpr (COLD) qrow = (int64_t)qid + q_offset;
    else qrow = sm.qrow[qs];
    compact16<C>(kq, sm, qs, K, emb, cand + (int64_t)qid * K, sp, ties, qid, fkey, fl, qemb, qrow);
    // overflowed: listed for the exact-mode relaunch with its band limit as the seed (same list position)
    if (lane == 0 && sm.ovf[qs]) {
      const int pos = atomicAdd(n_ovf, 1);
      ovf_list[pos] = qid;
      reinterpret_cast<uint32_t*>(n_ovf + 1)[pos] = (uint32_t)sm.ovf[qs];
    }
  }
  if (ABL && sink == 0x7fffffff) cand[0] = sink;
  if (STATS) {
    stat_add(8, __builtin_amdgcn_s_memrealtime() - t_final);
    stat_add(6, __builtin_amdgcn_s_memrealtime() - t_kernel);
    // [15]: per workgroup, the busiest wave's time outside the group barrier (Σ over workgroups; against the mean
    // Σ([6] − [7]) / waves it tells a systematic per-wave imbalance from a per-group one)
    __syncthreads();
    if (gstats != nullptr && threadIdx.x == 0) {
      unsigned long long mx = 0;
      for (int w = 0; w < Wact; ++w) mx = max(mx, sm.wstat[w][6] - sm.wstat[w][7]);
      atomicAdd(gstats + 15, mx);
    }
    if (gstats != nullptr && lane < kStats && lane != 15) atomicAdd(gstats + lane, sm.wstat[wave][lane]);
    // dbg 64: the prologue's counters too (the caller's array then holds 2·kStats entries before any dump)
    if (gstats != nullptr && (dbg & 64) && lane >= kStats && lane < kStatsX)
      atomicAdd(gstats + lane, sm.wstat[wave][lane]);
    // dbg 4096: workgroup timeline (start of its first wave, end of its last) at gstats[16 + 2·block] (dbg 64: 32 +)
    if (gstats != nullptr && (dbg & 4096) && lane == 0) {
      const int t0 = (dbg & 64) ? 2 * kStats : kStats;
      atomicMin(gstats + t0 + 2 * blockIdx.x, t_kernel);
      atomicMax(gstats + t0 + 1 + 2 * blockIdx.x, __builtin_amdgcn_s_memrealtime());
    }
  }
}
