// fwav_topk_merge.h — k_merge_pieces, the merge of a split block's table pieces.
// Part of fwav_topk.hip's translation unit: included there, inside namespace fwav, after the shared constants
// and the headers before it (the file map at the top of fwav_topk.hip); not a header for any other file.
#pragma once

// Merge the pieces of split blocks: per query, the union of its P pieces' bands (piece_band: entries whose key beats
// the shared limit at the piece's end) is filtered once more by the query's final shared limit Lk, rescored in exact
// f32 (sgemv16, the order of every other final pass), sorted (score desc, index asc) and cut to K.  Every exact top-K
// member lies in one piece's chunk range with a key above every limit, so it is in the union; the piece that
// published Lk holds K entries above it, so the union has at least K whenever Lk != 0.  A query flagged by any piece,
// or whose union would not fit one sort (C entries), goes to the exact-mode relaunch list once, seeded with the
// largest flag key (each a valid band limit) or Lk.  One wave per query.
// k_merge_pieces' last step: the band's mb ≤ 64·E keys (staged in LDS) rescored in exact f32 (sgemv16), sorted
// (score desc, index asc), listed if tied, the first K emitted.
template <int E>
__device__ __forceinline__ void merge_band(const uint64_t* __restrict__ sw, int mb, int K, const float* __restrict__ emb,
                                           const float* __restrict__ qemb, int64_t qrow, const SgemvSplit& sp, int32_t* __restrict__ ties, int32_t qid,
                                           int32_t* __restrict__ out, uint32_t fkey, const FloorCtl& fl) {
  const int lane = threadIdx.x & 63;
  uint64_t v[E];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = j * 64 + lane;
    v[j] = e < mb ? sw[e] : 0ull;
  }
  const float4* qp = reinterpret_cast<const float4*>(qemb + qrow * 16);  // qrow: a row of the query table
  float qv[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 x = qp[i];
    qv[4 * i] = x.x; qv[4 * i + 1] = x.y; qv[4 * i + 2] = x.z; qv[4 * i + 3] = x.w;
  }
  // rescore two slots at a time (8 row loads in flight per lane; all E at once held 4·E float4 rows and doubled the
  // kernel's registers)
#pragma unroll
  for (int j0 = 0; j0 < E; j0 += 2) {
    float4 row[2][4];
    int32_t dd[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = j0 + jj < E ? j0 + jj : E - 1;
      dd[jj] = (j0 + jj < E && v[j] != 0ull) ? key_idx(v[j]) : 0;
      const float4* rp = reinterpret_cast<const float4*>(emb + (int64_t)dd[jj] * 16);
#pragma unroll
      for (int i = 0; i < 4; ++i) row[jj][i] = rp[i];
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = j0 + jj;
      if (j < E && v[j] != 0ull) {
        const float acc = sgemv16([&](int k) { return f4c(row[jj][k >> 2], k & 3); }, [&](int k) { return qv[k]; },
                                  sgemv_kind((uint32_t)dd[jj], sp));
        v[j] = make_key(acc, dd[jj]);
      }
    }
  }
  wave_sort_desc<E>(v);
  if (fkey != 0u) {
    uint64_t kth = 0;
#pragma unroll
    for (int j = 0; j < E; ++j)
      if (j == ((K - 1) >> 6)) kth = __shfl(v[j], (K - 1) & 63);
    if (floor_miss(fkey, fl, mb, K, kth, qid)) return;
  }
  record_tie<E>(ties, qid, tie_flags<E>(v, mb, K), v, mb, K, true);
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = j * 64 + lane;
    if (e < K) out[e] = v[j] != 0ull ? key_idx(v[j]) : -1;
  }
}

// One split-block query of k_merge_pieces (defined below the kernel); MP ≥ the plan's pieces.
template <int C, int QB, bool HL, int MP>
__device__ __forceinline__ void merge_query(const TopkPlan& plan, int64_t w, int lane, uint64_t* sw, uint32_t* sh,
                                            const uint64_t* __restrict__ gkeys_all, const int32_t* __restrict__ active,
                                            int n_active, int K, int32_t* __restrict__ cand,
                                            int32_t* __restrict__ ovf_list, int32_t* __restrict__ n_ovf,
                                            const uint32_t* __restrict__ share, const float* __restrict__ emb,
                                            int64_t q_offset, const SgemvSplit& sp, int32_t* __restrict__ ties,
                                            uint32_t fkey, const FloorCtl& fl, const float* __restrict__ qemb);

// k_merge_pieces' union: the pieces' bands hold n = Σ counts entries (cfg2: mean 174, max 268 over 60,416 queries;
// those above the shared limit Lk mean 163; the band kept after the select mean 78, max 113: tools/diag/
// merge_inputs.py, profiles/r06/merge_inputs_cfg2.log).  The entries above Lk are compacted into the wave's LDS row
// and, up to merge_fast(MP)·64 of them, selected from registers; a wider union (long runs of near-equal scores) is
// selected by re-reading it from L2 once per key bit instead, so the register budget — and the occupancy — no longer
// scale with the widest plan's P·(C − 64).
// (The floor's second pass merges 16, 32 or 64 pieces of a low floor: its unions above Lk run to ≈ 800 entries and
// more — thousands with 64 pieces; there the union's key words, merge_hi_rows(MP) rows of them, are selected from LDS
// before the L2 tier: a 64-piece merge of 580 queries 786 µs with 32 rows, 145 with 64.)
constexpr int kMergeFast = 8;
constexpr int merge_hi_rows(int MP) { return MP <= 8 ? 1 : (MP <= 32 ? 32 : 64); }
template <int C, int QB, bool HL, int MP>
__global__ __launch_bounds__(256) void k_merge_pieces(const uint64_t* __restrict__ gkeys_all,
                                                      const int32_t* __restrict__ active,
                                                      const int32_t* __restrict__ n_active_p, int plan_rt, int plan_p,
                                                      int K, int32_t* __restrict__ cand, int32_t* __restrict__ ovf_list,
                                                      int32_t* __restrict__ n_ovf, const uint32_t* __restrict__ share,
                                                      const float* __restrict__ emb, int64_t q_offset, SgemvSplit sp,
                                                      int32_t* __restrict__ ties, FloorCtl fl,
                                                      const float* __restrict__ qemb) {
  const int n_active = *n_active_p;
  const uint32_t fkey = fl.key != nullptr ? __builtin_amdgcn_readfirstlane(*fl.key) : 0u;
  const bool alt = fl.key != nullptr && fkey == 0u;  // the floor did not apply: the floor-free plan (FloorCtl)
  const TopkPlan plan = make_plan(n_active, alt ? fl.alt_rt : plan_rt, alt ? fl.alt_p : plan_p, QB);
  if (plan.R == 0 || plan.halves) return;
  const int lane = threadIdx.x & 63;
  __shared__ uint64_t stage[4][kMergeFast * 64];  // per wave: the union above Lk, then the band (≤ C of it)
  __shared__ uint32_t hstage[4][merge_hi_rows(MP) * 64];  // per wave (16 / 32 pieces): the union's key words
  uint64_t* sw = stage[threadIdx.x >> 6];
  uint32_t* sh = hstage[threadIdx.x >> 6];
  // one wave per split-block query.  (Persistent waves looping over the queries measured the same, cfg2 search 17.40
  // vs 17.39 ms, profiles/r05/ab_merge_persistent.log, but the loop made the compiler hoist per-lane invariants of
  // the body out of it: 131 VGPRs, 3 waves per SIMD.)
  // (wave-uniform values in scalar registers: the query's row, limit and addresses load through the scalar cache)
  const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w < plan.R * QB)
    merge_query<C, QB, HL, MP>(plan, w, lane, sw, sh, gkeys_all, active, n_active, K, cand, ovf_list, n_ovf, share,
                               emb, q_offset, sp, ties, fkey, fl, qemb);
}

// One split-block query w of k_merge_pieces (whole wave; sw: the wave's LDS row).
template <int C, int QB, bool HL, int MP>
__device__ __forceinline__ void merge_query(const TopkPlan& plan, int64_t w, int lane, uint64_t* sw, uint32_t* sh,
                                            const uint64_t* __restrict__ gkeys_all, const int32_t* __restrict__ active,
                                            int n_active, int K, int32_t* __restrict__ cand,
                                            int32_t* __restrict__ ovf_list, int32_t* __restrict__ n_ovf,
                                            const uint32_t* __restrict__ share, const float* __restrict__ emb,
                                            int64_t q_offset, const SgemvSplit& sp, int32_t* __restrict__ ties,
                                            uint32_t fkey, const FloorCtl& fl, const float* __restrict__ qemb) {
  constexpr int E = C / 64;
  constexpr int kBit0 = HL ? 0 : 12;  // the select's resolution (S16 needs the K-th only at ≈ 2^-11)
  constexpr int kHiRows = merge_hi_rows(MP);
  const int64_t block = plan.F + w / QB;
  const int ql = (int)(w % QB);
  const int64_t qq = slot_query(block, ql, plan.nb);
  if (qq >= n_active) return;
  const int P = plan.P;
  // piece headers ((overflow key << 32) | count), lane p < P loading piece p's: one vector load for all of them
  // key region of piece p: base0 + p·pstride (item_of is linear in the piece)
  const int64_t base0 = ((int64_t)plan.item_of(block, 0) * QB + ql) * C;
  const int64_t pstride = (plan.item_of(block, 1) - plan.item_of(block, 0)) * (int64_t)QB * C;
  const uint64_t hdr = lane < P ? gkeys_all[base0 + (int64_t)lane * pstride + C - 1] : 0ull;
  const uint32_t Lk = __builtin_amdgcn_readfirstlane(share[qq]);
  const int32_t qid = __builtin_amdgcn_readfirstlane(active[qq]);
  // prefix of the counts and the largest overflow flag.  Up to 16 pieces: wave-uniform, in SGPRs, and a piece found by
  // comparing against each prefix; 32 / 64 pieces: lane p holds piece p's exclusive prefix and an entry's piece is
  // found by a binary search over the lanes (6 shuffles instead of MP − 1 compares and selects per entry)
  constexpr bool kLanePre = MP > 16;
  int pre[kLanePre ? 1 : MP + 1];
  uint32_t seed = 0u;
  int n = 0, pre_l = 0;
  if constexpr (kLanePre) {
    static_assert(MP <= 64, "one piece per lane");
    const int cnt = lane < P ? (int)(uint32_t)hdr : 0;
    int inc = cnt;  // inclusive prefix over the lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(inc, off);
      if (lane >= off) inc += y;
    }
    pre_l = inc - cnt;
    n = __builtin_amdgcn_readlane(inc, 63);
    uint32_t sd = lane < P ? (uint32_t)(hdr >> 32) : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sd = max(sd, (uint32_t)__shfl_xor((int)sd, off));
    seed = __builtin_amdgcn_readfirstlane(sd);
  } else {
    pre[0] = 0;
#pragma unroll
    for (int p = 0; p < MP; ++p) {
      const uint64_t h = p < P ? (uint64_t)__builtin_amdgcn_readlane((int)(uint32_t)hdr, p) |
                                     ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(hdr >> 32), p) << 32)
                               : 0ull;
      seed = max(seed, (uint32_t)(h >> 32));
      pre[p + 1] = pre[p] + (int)(uint32_t)h;
    }
    n = pre[MP];
  }
  // entry e of the union: piece p (pre[p] ≤ e < pre[p + 1]) at offset e − pre[p]; 0 past the end
  auto entry = [&](int e) -> uint64_t {
    int p = 0, start = 0;
    if constexpr (kLanePre) {
      // the largest p < P with pre[p] ≤ e (a piece of count 0 shares its prefix with the next one, which wins)
#pragma unroll
      for (int step = 32; step > 0; step >>= 1) {
        const int mid = p + step;
        const int pm = __shfl(pre_l, mid < 64 ? mid : 63);
        if (mid < P && pm <= e) p = mid;
      }
      start = __shfl(pre_l, p);
    } else {
#pragma unroll
      for (int pp = 1; pp < MP; ++pp)
        if (pp < P && e >= pre[pp]) {
          p = pp;
          start = pre[pp];
        }
    }
    return e < n ? gkeys_all[base0 + (int64_t)p * pstride + (e - start)] : 0ull;
  };
  const int nu = (n + 63) >> 6;  // 64-entry rows of the union (wave-uniform)
  uint32_t L = Lk;
  int mb = 0;
  if (seed == 0u) {
    // the union's entries above Lk, compacted into the wave's LDS row (kMergeFast rows of loads in flight: one
    // memory round trip for a union of up to kMergeFast·64 entries), with the key bits they all share (a AND, o OR)
    int m = 0;
    uint32_t a = ~0u, o = 0u;
    for (int u0 = 0; u0 < nu; u0 += kMergeFast) {
      uint64_t y[kMergeFast];
#pragma unroll
      for (int i = 0; i < kMergeFast; ++i) y[i] = u0 + i < nu ? entry((u0 + i) * 64 + lane) : 0ull;
#pragma unroll
      for (int i = 0; i < kMergeFast; ++i) {
        const bool in = (uint32_t)(y[i] >> 32) > Lk;
        const uint64_t bm = __ballot(in);
        const int pos = m + __popcll(bm & ((1ull << lane) - 1ull));
        if (in) {
          if (pos < kMergeFast * 64) sw[pos] = y[i];
          if (kHiRows > 1 && pos < kHiRows * 64) sh[pos] = (uint32_t)(y[i] >> 32);
          a &= (uint32_t)(y[i] >> 32);
          o |= (uint32_t)(y[i] >> 32);
        }
        m += __popcll(bm);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      a &= (uint32_t)__shfl_xor((int)a, off);
      o |= (uint32_t)__shfl_xor((int)o, off);
    }
    const uint32_t d = a ^ o;
    const int top = d == 0u ? -1 : 31 - __builtin_clz(d);
    uint32_t T = (top < 0 ? a : a & ~((2u << top) - 1u)) & ~((1u << kBit0) - 1u);
    const int mu = (m + 63) >> 6;
    if (m <= kMergeFast * 64) {
      // the usual case: the union above Lk in registers; its K-th key T by a greedy bitwise select that starts below
      // the bits every entry shares, and the band above T − margin compacted back into the LDS row
      uint64_t x[kMergeFast];
#pragma unroll
      for (int u = 0; u < kMergeFast; ++u) x[u] = u * 64 + lane < m ? sw[u * 64 + lane] : 0ull;
      if (m > K) {
        for (int bit = top; bit >= kBit0; --bit) {
          const uint32_t Tc = T | (1u << bit);
          int c = 0;
#pragma unroll
          for (int u = 0; u < kMergeFast; ++u)
            if (u < mu) c += __popcll(__ballot((uint32_t)(x[u] >> 32) >= Tc));
          if (c >= K) T = Tc;
        }
        L = max(L, f2key(HL ? key2f(T) - 2.5f * kHLDelta : key2f(T) - 2.0f * kF16Delta));
      }
#pragma unroll
      for (int u = 0; u < kMergeFast; ++u) {
        if (u < mu) {
          const bool keep = x[u] != 0ull && (uint32_t)(x[u] >> 32) > L;
          const uint64_t bm = __ballot(keep);
          const int pos = mb + __popcll(bm & ((1ull << lane) - 1ull));
          if (keep && pos < C) sw[pos] = x[u];
          mb += __popcll(bm);
        }
      }
    } else if (kHiRows > 1 && m <= kHiRows * 64) {
      // a wider union (16 / 32 pieces): the select over its key words in LDS, then the band re-streamed from L2
      if (m > K) {
#pragma unroll 1
        for (int bit = top; bit >= kBit0; --bit) {
          const uint32_t Tc = T | (1u << bit);
          // the lane's count over the rows, 8 LDS reads in flight, then one wave sum per bit
          int c = 0;
#pragma unroll 1
          for (int u0 = 0; u0 < mu; u0 += 8) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const int e = (u0 + i) * 64 + lane;
              c += (e < m && sh[e < kHiRows * 64 ? e : 0] >= Tc) ? 1 : 0;
            }
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
          if (c >= K) T = Tc;
        }
        L = max(L, f2key(HL ? key2f(T) - 2.5f * kHLDelta : key2f(T) - 2.0f * kF16Delta));
      }
      for (int u0 = 0; u0 < nu; u0 += kMergeFast) {
        uint64_t y[kMergeFast];
#pragma unroll
        for (int i = 0; i < kMergeFast; ++i) y[i] = u0 + i < nu ? entry((u0 + i) * 64 + lane) : 0ull;
#pragma unroll
        for (int i = 0; i < kMergeFast; ++i) {
          const bool keep = (uint32_t)(y[i] >> 32) > L;
          const uint64_t bm = __ballot(keep);
          const int pos = mb + __popcll(bm & ((1ull << lane) - 1ull));
          if (keep && pos < C) sw[pos] = y[i];
          mb += __popcll(bm);
        }
      }
    } else {
      // a wide union (long runs of near-equal scores): the same select, its entries re-read from L2 for every key bit
#pragma unroll 1
      for (int bit = top; bit >= kBit0; --bit) {
        const uint32_t Tc = T | (1u << bit);
        int c = 0;
#pragma unroll 1
        for (int u = 0; u < nu; ++u) {
          const uint32_t h = (uint32_t)(entry(u * 64 + lane) >> 32);
          c += __popcll(__ballot(h > Lk && h >= Tc));
        }
        if (c >= K) T = Tc;
      }
      L = max(L, f2key(HL ? key2f(T) - 2.5f * kHLDelta : key2f(T) - 2.0f * kF16Delta));
#pragma unroll 1
      for (int u = 0; u < nu; ++u) {
        const uint64_t y = entry(u * 64 + lane);
        const bool keep = (uint32_t)(y >> 32) > L;
        const uint64_t bm = __ballot(keep);
        const int pos = mb + __popcll(bm & ((1ull << lane) - 1ull));
        if (keep && pos < C) sw[pos] = y;
        mb += __popcll(bm);
      }
    }
  }
  if (seed != 0u || mb > C) {
    // a piece overflowed, or the band would not fit one sort: the exact-mode relaunch, seeded with a valid limit
    if (lane == 0) {
      const int pos = atomicAdd(n_ovf, 1);
      ovf_list[pos] = qid;
      reinterpret_cast<uint32_t*>(n_ovf + 1)[pos] = max(seed, L);
    }
    return;
  }
  // same wave: its own ds_writes are ordered before merge_band's reads
  if (C > 128 && mb <= 128)
    merge_band<2>(sw, mb, K, emb, qemb, (int64_t)qid + q_offset, sp, ties, qid, cand + (int64_t)qid * K, fkey, fl);
  else
    merge_band<E>(sw, mb, K, emb, qemb, (int64_t)qid + q_offset, sp, ties, qid, cand + (int64_t)qid * K, fkey, fl);
}
