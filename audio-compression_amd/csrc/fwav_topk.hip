// fwav_topk.hip — fused similarity GEMM + streaming exact top-K on MFMA (gfx950).
//
// Replaces (reference /root/reference/fractal.py):
//   cpu_worker                          :556-632  per range: q = emb[i] (quirk Q1), linear search, pad to K
//   range_candidates_from_embedding_emb :535-541  scores = E_dom @ q ; argpartition top-K ; sort desc
//   pad_candidates                      :544-552
//
// Contract: for every active query q (a range index; its query vector is domain-embedding row q), write
// the K domains with the largest f32 score s(q,d) = emb[d]·emb[q] evaluated in the reference's own order (numpy →
// OpenBLAS sgemv_t: its 4-column microkernel, and for the last columns of each BLAS thread's chunk the 4x2 / 4x1
// tail kernels — fwav_common.h sgemv16 / sgemv_kind, pinned column by column against numpy), in (score desc,
// index asc) order, −1-padded when nd < K.  The scores being the reference's bit for bit, the result can differ from
// the reference's only among exactly equal scores, whose order (and, at the K-th place, set) numpy's introselect /
// argsort decide: every such query is listed in `ties` (record_tie) for fwav_tie_check / fwav.ties.
//
// The n_ranges × n_domains score matrix (4.4e11 entries at cfg2) is never materialised.
//
// One translation unit, one concern per file (the private headers are included below, in this order, inside
// namespace fwav; the debug knobs are TU-local statics shared by the policy and the launcher):
//   fwav_topk_f32.h    k_sim_topk_f32, the all-f32 search (emb16 == NULL)
//   fwav_topk_plan.h   the work plan: query blocks, table pieces, query halves (TopkPlan, make_plan, plan_item)
//   fwav_topk_floor.h  the speculative floor's device side (FloorCtl, the pilot kernels) and the ordered active list
//   fwav_topk_first.h  k_sim_topk_f16 and its device helpers: the fp16 first pass and its relaunch modes
//   fwav_topk_merge.h  k_merge_pieces: the merge of a split block's table pieces
//   this file          the compile-time switches and their guard, the shared constants, the geometry table (kGeo) and
//                      the host policy (first_geometry, host_plan_for, the floor's policy), the workspace layout,
//                      launch_topk, the C ABI and the debug ABI
//
// Production path (emb16 != NULL): the work plan (query blocks, table pieces, query halves);
// k_sim_topk_f16 — 8 waves × 32 queries per workgroup (16 waves, one per CU, above 8 Mi domains), the fp16 table
// streamed through LDS by LDS-DMA in groups of 4 chunks, one fp16 MFMA per 32-domain tile and a max-fold per lane
// (stream_group), fired chunks replayed at window ends into per-query two-ended key buffers with inline compaction
// (replay_window / append_tile / compact16_s16), band limits seeded from each query's own domain window
// (seed_limit) and shared between the table pieces of a query (atomicMax), an exact f32 final pass in the
// reference's sgemv order (compact16) or a band hand-off to k_merge_pieces (piece_band); then the device-side
// overflow lists relaunch the same kernel in the narrower HL and exact modes.  Measurements behind every constant:
// DESIGN.md §3.1.
//
// k_sim_topk_f32 (emb16 == NULL; tests and a reference for the production kernel): workgroup = 4 waves × 32
// queries; each 256-domain chunk is staged row-major in LDS and every lane scores its query against 16 domain rows
// of each 32-domain tile with sgemv16 (VALU), keeps a running threshold θ (one register per lane), and appends
// (score, index) keys that beat θ to the query's LDS buffer; a nearly full buffer is sorted (64-lane bitonic), cut
// to its top K and θ set to the K-th score.  Domains stream in increasing index order, so a later domain whose
// score equals θ can never displace an earlier one: strict '>' is exact.
#include <algorithm>
#include <cstring>
#include <type_traits>
#include "fwav_centroid_bound.h"
#include "fwav_common.h"
#include "fwav_topk_keys.h"
#include "../../include/fwav.h"

// The compile-time switches of the search — all of them: the private headers below define none (tests/test_capi.py).
// Each builds A/B variants of the DEBUG library only (tools/ab_build.sh adds -DFWAV_DEBUG_API): a product build that
// sets one stops here, so libfwav.so is always the measured default.  They cost no code: template arguments,
// constants and the ablation mask.  (The switches that guarded decided code paths and tunables were retired:
// tools/experiments/README.md lists them with their results.)
#if !defined(FWAV_DEBUG_API) && (defined(FWAV_TOPK_ABL) || defined(FWAV_TOPK_CB) || defined(FWAV_TOPK_CENT) || \
    defined(FWAV_TOPK_CG) || defined(FWAV_TOPK_CPMIN) || defined(FWAV_TOPK_CW) || defined(FWAV_TOPK_G) || \
    defined(FWAV_TOPK_QS) || defined(FWAV_TOPK_W))
#error "experiment switches build the debug library only (-DFWAV_DEBUG_API)"
#endif
// Production geometry (the -D overrides build A/B variants: tools/ab_topk.py): chunks per barrier, waves per
// workgroup, query sets of 32 per wave
#ifndef FWAV_TOPK_G
#define FWAV_TOPK_G 4
#endif
#ifndef FWAV_TOPK_W
#define FWAV_TOPK_W 8
#endif
#ifndef FWAV_TOPK_QS
#define FWAV_TOPK_QS 1
#endif
// Centroid geometry (cent_level1): FWAV_TOPK_CENT query sets per wave (0: off), FWAV_TOPK_CW waves per
// workgroup, FWAV_TOPK_CG chunks per barrier
// Same-box A/B (tools/ab_topk.py, identical outputs; profiles/r04/ab_cent_*.log), search ms base → centroid:
//   cfg2 (330,750 queries) 20.36 → 17.47 (QS 2, G 4, 2 workgroups per CU, 4 waves per SIMD), QS 4 / G 3 18.49,
//   QS 4 / G 4 (one workgroup per CU: 2 waves per SIMD) 25.3 — the base kernel held to the same occupancy 25.6;
//   165,375 queries 10.94 → 9.93, 82,688 5.92 → 5.69, 41,344 (one rank's eighth) 3.32 → 3.53 (fewer, longer items:
//   the base geometry is kept below kCentMinQ); cfg3 (hi/lo band, 6.6 M domains) 180 → 195 (kept base).
#ifndef FWAV_TOPK_CENT
#define FWAV_TOPK_CENT 2
#endif
#ifndef FWAV_TOPK_CW
#define FWAV_TOPK_CW 8
#endif
#ifndef FWAV_TOPK_CG
#define FWAV_TOPK_CG 4
#endif
#ifndef FWAV_TOPK_CB
#define FWAV_TOPK_CB 2  // centroid level 2: (tile, set) pairs in flight together (4: +0.8 % cfg2, +10 % at 82,688 queries; 6, 8: spills)
#endif
#ifndef FWAV_TOPK_CPMIN
#define FWAV_TOPK_CPMIN 6  // centroid geometry, up to 1.5 rounds of blocks: at least this many table pieces each
#endif
// Ablation builds (tools/ab_build.sh NAME -DFWAV_TOPK_ABL=<dbg bits>): the production kernel with the given `dbg`
// bits fixed at compile time — the STATS kernel's counters cost registers (it spills), which skews its timings.
#ifndef FWAV_TOPK_ABL
#define FWAV_TOPK_ABL 0
#endif

namespace fwav {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kTopkWaves = 4;
constexpr int kTopkQ = 32 * kTopkWaves;  // queries per workgroup
constexpr int kChunk = 256;              // domains staged per LDS chunk (16 KB of f32 embeddings)
constexpr int kTopkThreads = 64 * kTopkWaves;

// δ ≥ max |s16 − s32| ("Exactness", fwav_topk_first.h): 1.9536e-3 (f16 rounding of both operands) + ≈ 5e-6 (f32
// accumulation of both sums, f16 subnormals) = 1.9584e-3.  2.5e-3 → 2.0e-3: cfg3 792 → 719 ms, cfg2 unchanged.
constexpr float kF16Delta = 2.0e-3f;
// δ' ≥ max |shl − s32| (see "Exactness"); the stream fires a tile when s16 > lim − kStreamMargin
constexpr float kHLDelta = 1.0e-5f;
constexpr float kStreamMargin = kF16Delta + 2.0f * kHLDelta;
// Search modes (template MODE of k_sim_topk_f16; launched as a chain, each relaunch on the previous pass's overflow
// list, seeded with its band limits):
//   kModeS16: band on s16 (width 2δ), keys s16 — no low-part MFMAs in the replays;
//   kModeHL : band on shl (width 2.5δ'), keys shl — three MFMAs per replayed tile, overflows only on ≥ 192 domains
//             within ≈ 2δ' of the K-th (runs of identical tiles);
//   kModeEX : exact keys (sgemv16 on the VALU for rows passing the s16 filter), a compaction keeps exactly the top K,
//             so nothing can overflow.
constexpr int kModeS16 = 0, kModeHL = 1, kModeEX = 2;
constexpr int kGroup = FWAV_TOPK_G;     // chunks per barrier
constexpr int k16Waves = FWAV_TOPK_W;   // waves per workgroup
constexpr int k16Sets = FWAV_TOPK_QS;   // query sets of 32 per wave (each LDS fragment feeds k16Sets MFMAs)
constexpr int k16Cap = 256;  // key-buffer entries per query (global workspace)
static_assert(k16Cap >= 128 && (k16Cap & (k16Cap - 1)) == 0, "the final bitonic sort needs a power-of-two buffer");
// (A/B at cfg2: 512 entries 24.4 ms vs 21.2 ms for 256 — fewer compactions do not pay for the longer final sort)
constexpr int k16QB = 32 * k16Waves * k16Sets;  // queries per block (one workgroup's query set)
// a first pass's table pieces per split block (merge: P·(C − 64) keys per query at most) ...
constexpr int kPlanMaxPieces = 8;
// ... and any plan's, the floor's later passes included (k_merge_pieces is instantiated for ≤ 8, 16 and 32 pieces)
constexpr int kMaxPieces = 64;
static_assert(kPlanMaxPieces <= kMaxPieces, "first-pass plans stay within the merge's widest instantiation");
// A query table of the search's own (the _q entry points; compress_audio(query="range")): local query i reads row
// q_offset + i of emb (f32, 16 columns) and of its tiled fp16 high and low parts, and the first pass seeds its band
// limit from the table rows around min(row·seed_stride, n_domains − 1).  The plain entry points search with the domain
// table's own rows (quirk Q1) and pass an empty one, which their kernels (XQ = false) never read.
struct QueryTab {
  const float* emb = nullptr;
  const _Float16* hi = nullptr;
  const _Float16* lo = nullptr;
  int seed_stride = 1;
};

// The first pass's seed policy (seed_limit): 0 = where a floor is applied, one probe at the floor decides per query set
// whether the seeds' bit search runs; 1 = always the search; 2 = never seed.  Every policy returns the same candidates.
#ifdef FWAV_DEBUG_API
static int g_seed_mode = 0;  // fwav_debug_topk_seeds (debug library only)
constexpr bool kSeedKnob = true;
#else
constexpr int g_seed_mode = 0;
constexpr bool kSeedKnob = false;  // the product's kernels do not read FloorCtl::seeds
#endif

#include "fwav_topk_f32.h"
#include "fwav_topk_plan.h"
#include "fwav_topk_floor.h"
#include "fwav_topk_first.h"
#include "fwav_topk_merge.h"

// ------------------------------------------------------------------------------------------------ host policy
// The first pass's mode: S16 (→ HL → EX relaunches) for tables of at most kHLFirstMinDomains domains, HL (→ EX) for
// larger ones.  Same-box A/B (tools/ab_topk.py, identical outputs): cfg2 (1.3 M domains, noise) S16 20.0–20.1 ms vs
// HL 20.7–21.0 — its bands never overflow, and HL's three-MFMA replays cost more; cfg3 (6.6 M, speech-like) S16
// 254–258 ms vs HL 186–189 (30.5 % of the queries overflow the S16 band and are searched again); a cfg4 shard (86 M,
// noise) S16 1,135 ms vs HL 960.
constexpr int64_t kHLFirstMinDomains = int64_t(1) << 22;
#ifdef FWAV_DEBUG_API
static int g_first_mode = -1;  // fwav_debug_topk_mode (debug library only): force S16 / HL
#else
constexpr int g_first_mode = -1;  // the product library has no process-global knobs
#endif
__host__ inline int first_mode(int64_t nd) {
  if (g_first_mode >= 0) return g_first_mode;
  return nd > kHLFirstMinDomains ? kModeHL : kModeS16;
}
// Host-side plan: default policy from the device's workgroup slots, or a diagnostic override.
#ifdef FWAV_DEBUG_API
static int g_plan_rt = -1, g_plan_p = -1;  // fwav_debug_topk_plan (debug library only)
static int g_tail_wb = -1;  // fwav_debug_topk_tail (debug library only): the last piece's weight in 1/16
#else
constexpr int g_plan_rt = -1, g_plan_p = -1;
constexpr int g_tail_wb = -1;
#endif
// Per-device caches (the caller makes the stream's device current: fwav.engine wraps every call in
// torch.cuda.device); kMaxDev bounds the device ordinal.
constexpr int kMaxDev = 64;
static int current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) dev = 0;
  return dev;
}
// First-pass geometry.  Tables of more than kWideMinDomains domains (an fp16 table of > 128 MB, on its way past the
// 256 MB Infinity Cache) take the wide workgroup (kGeoWide): 16 waves × 32 queries, one workgroup per CU (its LDS holds
// 2 × 8 chunk slots, one barrier per 8 chunks), so a CU streams the table once for 512 queries where the base
// geometry streams it twice for 2 × 256.  Same-box A/B on a cfg4 shard (86.4 M domains × 337,500 queries, identical
// outputs): base 973.8 ms, W = 16 / G = 4 963.3, W = 16 / G = 8 944.0, QS = 2 (233 VGPRs: 2 waves per SIMD) 1,088;
// cfg2 (1.3 M domains, MALL-resident table): base 20.7 ms, wide 21.7; cfg3 (6.6 M, a 212 MB table): base 187.6,
// wide 193.4; cfg4 shard again: base 962.2, wide 945.6 — so the wide geometry is used only where the table (32 B per
// domain) no longer fits the Infinity Cache.  Relaunches on overflow lists keep the base geometry (few queries).
constexpr int64_t kWideMinDomains = int64_t(1) << 23;
#ifdef FWAV_DEBUG_API
static int g_wide = -1;  // fwav_debug_topk_geometry (debug library only): force base / wide / centroid
static int g_cent_sets = -1;  // fwav_debug_topk_cent_sets (debug library only): the centroid geometry's sets per wave
#else
constexpr int g_wide = -1;
constexpr int g_cent_sets = -1;
#endif
// first-pass geometries
// (kGeoCent4, the centroid geometry with 4 sets per wave, is internal: the debug entry points' geometry codes stay
// 0 … 3, where it is forced as code 2 with fwav_debug_topk_cent_sets(4) and reported by its block layout, geo_code)
constexpr int kGeoBase = 0, kGeoWide = 1, kGeoCent = 2, kGeoCentWide = 3, kGeoCent4 = 4;
constexpr int kGeos = 5;
[[maybe_unused]] constexpr int kGeoCodes = 4;  // (the debug entry points' range)
// What a first-pass geometry is — the one place that says so: the block size, the occupancy query, the kernel and
// merge launches (with_geometry) and the debug entry points all read this table.
struct Geo {
  int W, G, QS;  // waves per workgroup, chunks per barrier, query sets of 32 per wave
  bool cent;     // the centroid pre-filter
  bool hl;       // hi/lo first passes are instantiated (else S16 only)
  bool stats;    // the debug library's counter kernel (STATS) is instantiated
  constexpr int qb() const { return 32 * W * QS; }  // queries per block
};
// wide: 16 waves, one workgroup per CU, one barrier per 8 chunks; centroid wide: that with 2 sets per wave;
// kGeoCent4: the centroid geometry with 4 sets per wave (1,024 queries per workgroup, Topk16SmemColdT) — one centroid
// per 4 consecutive queries halves level 1's tiles per query once more, 4 chunks per barrier (LDS
// 80,016 B; cfg2 search 11.69 ms vs 11.94 with 3)
constexpr Geo kGeo[kGeos] = {
    {k16Waves, kGroup, k16Sets, false, true, true},                                                    // kGeoBase
    {16, 8, 1, false, true, false},                                                                    // kGeoWide
    {FWAV_TOPK_CW, FWAV_TOPK_CG, FWAV_TOPK_CENT > 0 ? FWAV_TOPK_CENT : 4, true, true, true},           // kGeoCent
    {16, 8, 2, true, true, false},                                                                     // kGeoCentWide
    {FWAV_TOPK_CW, 4, 4, true, false, true},                                                           // kGeoCent4
};
static int geometry_qb(int geo) { return kGeo[geo].qb(); }
// f(geometry, mode), both as std::integral_constant, for the run-time first-pass geometry and mode (S16 where the
// geometry has no hi/lo instantiation: first_geometry picks such a geometry for S16 passes only)
template <class F>
static void with_geometry(int geo, int mode, F&& f) {
  auto go = [&](auto g) {
    if constexpr (kGeo[decltype(g)::value].hl) {
      if (mode == kModeHL) return f(g, std::integral_constant<int, kModeHL>{});
    }
    f(g, std::integral_constant<int, kModeS16>{});
  };
  switch (geo) {
    case kGeoWide: return go(std::integral_constant<int, kGeoWide>{});
    case kGeoCent: return go(std::integral_constant<int, kGeoCent>{});
    case kGeoCentWide: return go(std::integral_constant<int, kGeoCentWide>{});
    case kGeoCent4: return go(std::integral_constant<int, kGeoCent4>{});
    default: return go(std::integral_constant<int, kGeoBase>{});
  }
}
// The code the debug entry points report for a first-pass geometry: what fwav_debug_topk_qb and
// fwav_debug_topk_plan_cover need of it is the block layout, and kGeoCent4's 1,024-query blocks of 32 query groups
// (two halves of 512) are kGeoCentWide's.
constexpr int geo_code(int geo) { return geo == kGeoCent4 ? kGeoCentWide : geo; }
constexpr bool geo_is_cent(int geo) { return geo == kGeoCent || geo == kGeoCent4; }  // 8 waves, two workgroups per CU
constexpr int kCentDoubleBelow = 4;  // centroid geometry, blocks on at most half the slots: pieces doubled below this count
constexpr int kTailWeight = 12;  // multi-round plans of split blocks: the last piece's table share in 1/16 (16, 0: even)
// centroid geometry, up to 1.5 rounds of blocks: at least FWAV_TOPK_CPMIN table pieces each, and this many with the
// speculative floor (profiles/r05/plan_floor_ab*.log)
constexpr int kCentFloorPieces = 3;
// The centroid geometry for first passes of at least this many queries.  Below the speculative floor's minimum the
// centroid geometry lost to the base one (cold limits: 41,344 queries 3.42 vs 3.26 ms); with the floor it wins from
// 32,768 queries on (round 6, tools/ab/eighth_geo_prof.sh, profiles/r06/eighth_geo_*.log, floor on / base geometry,
// floor off, base geometry → floor on, centroid: 32,768 queries 2.73 / 2.80 → 2.42 ms, 41,344 2.93 / 3.22 → 2.88,
// 55,000 4.38 / 4.35 → 3.75), not at 20,672 (2.12 / 2.07 → 2.36: 41 blocks of 512 fill 328 of the 512 slots)
constexpr int64_t kCentMinQ = 32768;
// ... and with 4 sets per wave (kGeoCent4, S16 first passes) from this many queries on.  Same-process A/B against
// the 2-set geometry, identical candidates (profiles/r08/ab_sizes.log), search ms 2 sets → 4 sets: 330,750 queries
// 13.30 → 11.81, 262,144 10.61 → 9.44, 220,000 9.69 → 9.04, 165,375 7.28 → 7.19, 82,688 4.13 → 3.85, 41,344 (81
// blocks of 512 → 41 of 1,024 on 512 slots) 2.46 → 2.95.  (82,688 keeps 2 sets: DESIGN §10.)
constexpr int64_t kCent4MinQ = 131072;
static int first_geometry(int64_t nd, int64_t max_q) {
  // (4 sets are instantiated for S16 passes only: a hi/lo first pass runs kGeoCent whatever g_cent_sets asks for; a
  // forced kGeoCent is the 2-set geometry unless g_cent_sets says 4)
  const bool s16 = first_mode(nd) == kModeS16;
  if (g_wide >= 0) return g_wide == kGeoCent && g_cent_sets == 4 && s16 ? kGeoCent4 : g_wide;
  // tables past the Infinity Cache: the centroid filter in the wide geometry.  A cfg4 shard (337,500 queries × 86.4 M
  // domains, hi/lo band, identical outputs): wide 920 ms → centroid wide 632 ms
  // (profiles/r04/ab_centwide_cfg4_q337500.log)
  if (nd > kWideMinDomains) return max_q >= kCentMinQ ? kGeoCentWide : kGeoWide;
  // (S16 first passes only: for hi/lo ones the centroid geometry lost, cfg3 195 vs 180 ms base)
  const bool cent = FWAV_TOPK_CENT > 0 && max_q >= kCentMinQ && s16;
  const bool four = g_cent_sets < 0 ? max_q >= kCent4MinQ : g_cent_sets == 4;
  if (cent && four) return kGeoCent4;
  return cent ? kGeoCent : kGeoBase;
}

static void topk_device_slots(int geo, int& cus, int& per_cu) {
  static int cs[kGeos][kMaxDev] = {{0}}, ws[kGeos][kMaxDev] = {{0}};
  const int dev = current_device();
  int& c = cs[geo][dev];
  int& w = ws[geo][dev];
  if (c == 0) {
    // (of the mode each geometry is chosen for: the wide ones serve tables past kWideMinDomains, hi/lo passes)
    hipError_t occ = hipErrorUnknown;
    with_geometry(geo, geo == kGeoWide || geo == kGeoCentWide ? kModeHL : kModeS16, [&](auto g, auto mode) {
      constexpr Geo ge = kGeo[decltype(g)::value];
      occ = hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &w, k_sim_topk_f16<k16Cap, false, decltype(mode)::value, ge.W, ge.G, ge.QS, ge.cent>, 64 * ge.W, 0);
    });
    if (!(hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && occ == hipSuccess &&
          c > 0 && w > 0)) {
      c = 256;  // MI355X: 256 CUs × 2 base (1 wide) workgroups
      w = (geo == kGeoBase || geo_is_cent(geo)) ? 2 : 1;
    }
  }
  cus = c;
  per_cu = w;
}
// Default policy.  Whole-table items, dispatched in order, fill the slots round after round; the last round's
// workgroups run faster when they have a CU to themselves, but once that round holds more blocks than there are
// CUs, the surplus doubles up on a few CUs and finishes last (cfg2: 1292 blocks on 256 CUs × 2 → the last 268 blocks
// include 12 that ran 3.5 ms past the rest).  So the last 2·(surplus) blocks are split into 4 table pieces, which
// fill in beside the lone workgroups (cfg2 A/B: 24.9 → 22.6 ms; splitting more blocks costs more than it saves,
// since every piece restarts the rising limit: 268 blocks in 2 pieces 24.2 ms, 512 in 2 25.3 ms).  Few blocks
// (at most half the slots) are each split into up to 8 pieces so that the table passes use the idle CUs.
static bool floor_by_default(int64_t max_q, int64_t nd);  // (defined with the floor, below)
// floored: whether the first pass runs with the speculative floor (−1: as the launch decides, floor_by_default)
static void host_plan_for(int64_t max_q, int64_t nd, int geo, int& rt, int& P, int floored = -1) {
  if (g_plan_rt >= 0) {  // diagnostic override
    rt = g_plan_rt;
    P = g_plan_p;
  } else {
    int cus, per_cu;
    topk_device_slots(geo, cus, per_cu);
    const int64_t slots = (int64_t)cus * per_cu;
    const int64_t nb = cdiv(max_q > 0 ? max_q : 1, geometry_qb(geo));
    rt = 0;
    P = 1;
    if (2 * nb <= slots) {
      // every block split, pieces in piece-major order (TopkPlan::pm): the later pieces of a block start from the
      // limits its earlier pieces published, so twice the pieces that fit one round pay (one process per
      // configuration, identical outputs: 41,344 queries 3.60 → 3.35 ms with 6 pieces instead of 3 block-major;
      // 65,536: 5.29 → 4.83 with 4 instead of 2; 20,672: 2.25 → 2.08 with 6, block-major before)
      rt = (int)nb;
      int64_t p = slots / nb;
      if (p < (geo_is_cent(geo) ? kCentDoubleBelow : 4)) p *= 2;
      P = (int)(p < kPlanMaxPieces ? p : kPlanMaxPieces);
    } else if (2 * nb <= 3 * slots) {
      // up to 1.5 rounds of blocks: every block in max(3, ⌊2·slots / nb⌋) pieces, piece-major — later rounds start
      // from the earlier pieces' limits (82,688 queries: 6.43 → 5.92 ms with 3 pieces; 165,375: 11.27 → 10.81 with
      // 3, 10.72 with 4; the tail split below stays for more blocks: all of cfg2 in 2 / 3 / 4 piece-major pieces
      // 20.8 / 20.5 / 20.7 vs 20.2–20.4 ms)
      // The centroid geometry takes at least 6 (its first pass is cheap, so the table pieces' restarted limits weigh
      // less than the balance of ≈ 4–8 rounds of short items: cfg2 646 blocks in 3 / 4 / 5 / 6 / 8 pieces 17.37 /
      // 16.94 / 17.02 / 16.89 / 17.40 ms, 165,375 queries in 3 / 4 / 6 10.04 / 9.92 / 9.68;
      // profiles/r04/plan_sweep_cent_cfg2.log)
      rt = (int)nb;
      int64_t p = 2 * slots / nb;
      // With the speculative floor (§3.1b of DESIGN) no piece starts cold, and fewer, longer pieces pay: cfg2 in 3 / 4 /
      // 6 pieces 15.72 / 15.95 / 16.02 ms, 165,375 queries 8.66 / 8.89 / 8.75 (profiles/r05/plan_floor_ab*.log)
      const bool fl = floored < 0 ? floor_by_default(max_q, nd) : floored != 0;
      const int64_t pmin = geo_is_cent(geo) ? (fl ? kCentFloorPieces : FWAV_TOPK_CPMIN) : 3;
      if (p < pmin) p = pmin;
      P = (int)(p < kPlanMaxPieces ? p : kPlanMaxPieces);
    } else {
      const int64_t last = nb % slots == 0 ? slots : nb % slots;  // blocks in the last round
      if (last > cus) {
        // piece-major: the whole last round in 4 pieces (cfg2, one process per plan: 20.29–20.49 → 19.93 ms; the
        // block-major plan split only its 2·(surplus) doubled-up blocks)
        rt = (int)last;
        P = 4;
      } else if (5 * last <= 3 * cus) {
        // a last round of lone workgroups on at most 60 % of the CUs: its blocks as 4 table pieces each.  Same-box
        // A/B (identical outputs), last-round blocks → ms unsplit / split: 60 → 12.45 / 9.39, 134 (one rank's half
        // of cfg2) 12.54 / 11.24, 200 12.60 / 12.74, 250 13.13 / 13.33
        rt = (int)last;
        P = 4;
        // piece-major (base geometry): the round before it too, so that the short round's pieces follow pieces of
        // their own blocks (cfg3, one process per plan: 177.1–177.6 → 175.3–175.7 ms)
        if (geo == kGeoBase && nb >= last + slots) rt = (int)(last + slots);
      }
    }
  }
  // every piece streams at least 16 chunks (4,096 domains)
  const int64_t pmax = cdiv(nd, kChunk) / 16;
  if (P > pmax) P = (int)(pmax > 1 ? pmax : 1);
  // one round of split blocks, two workgroups to a CU: the pieces whose items start in the round's second half run as
  // their CU's younger workgroup and get the smaller share of the table (piece_chunks)
  if (g_plan_rt < 0 && P > 1 && P <= 0xFF) {
    const int tail_wb = g_tail_wb >= 0 ? g_tail_wb : kTailWeight;
    int cus, per_cu;
    topk_device_slots(geo, cus, per_cu);
    const int64_t slots = (int64_t)cus * per_cu;
    const int64_t nb = cdiv(max_q > 0 ? max_q : 1, geometry_qb(geo));
    const TopkPlan pl = make_plan(max_q, rt, P, geometry_qb(geo));
    if (per_cu == 2 && pl.F == 0 && pl.R == nb && pl.pm && pl.items() <= slots &&
        2 * pl.items() > slots) {
      // every block's pieces weighed by their own items' side of slots / 2 (TopkPlan::ybound).  (Round 6 first
      // weighed whole pieces, from the first piece past slots / 2 on: one rank's eighth of cfg2, 81 blocks × 6
      // pieces in one round, 2.56 → 2.53 ms, profiles/r06/ab_young.log)
      if (slots / 2 < 0xFFF) P |= (1 << 30) | (int)((slots / 2) << 8);
    } else if (tail_wb > 0 && tail_wb != 16 && pl.F == 0 && pl.R == nb && pl.pm && pl.items() > slots) {
      // several rounds of split blocks, piece-major: the items that start last are the blocks' last pieces, and the
      // launch ends with the slowest of them, so the last piece of every block takes tail_wb / 16 of the others'
      // share of the table.  Same process (tools/diag/topk_reps.py, FWAV_DEBUG_TOPK_TAIL, profiles/r06/tail_sweep.log):
      // cfg2 (646 centroid blocks × 3 pieces) 14.26–14.46 ms even, 13.98 / 14.02–14.06 / 14.16 / 14.22 at 11 / 12 /
      // 13 / 14; 165,375 queries 7.72 → 7.57 at 12
      P |= ((P - 1) << 8) | (tail_wb << 16) | (16 << 21);
    }
  }
}
// ---------------------------------------------------------------------------------------- speculative floor
// A first pass of at least kFloorMinQ queries over at least kFloorMinD domains starts every band
// limit at a floor guessed from kFloorPilots pilot queries (FloorCtl); the queries it cuts are searched again.
// Measured (tools/seed_ab.py, profiles/r05/seed_floor_cfg2.log): cfg2's search 17.01 ms unseeded, 15.27 / 14.71 /
// 14.12 ms with one floor of 1.80 / 1.85 / 1.88 for every query (0.05 / 0.38 / 1.7 % of the queries below it, their
// misses not counted), 12.20 ms with each query's own exact K-th score.
// The later passes cost a round of table pieces whatever their size (≈ 0.5–1 ms: a piece's cost is mostly the rise
// of its limit), so the floor pays only where it saves more than that (tools/floor_pass_ab.py, pilots' 10th-smallest
// estimate, same box): 330,750 queries 18.15 → 15.90 ms, 165,375 9.70 → 8.65, 82,688 6.14 → 5.33, but 41,344 (one
// rank's share at N = 8) 3.40 → 3.94 (profiles/r05/floor_pass_ab.log, floor_pass_ab_mid.log) — in the base
// geometry; with the centroid geometry the floor pays from 32,768 queries on (round 6, kCentMinQ)
constexpr int64_t kFloorMinQ = 32768, kFloorMinD = 65536;
// ... and tables of at most kFloorMaxD domains: the later passes' pieces grow with the table, and at cfg4's
// 86.4 M domains the second pass took 204 ms after a 511 ms first pass (a 262,144-query search, profiles/r05/
// kernel_stats_bench_cfg2.txt: the cfg4 affine-roofline extra of bench.py)
constexpr int64_t kFloorMaxD = int64_t(1) << 22;
// the second pass's table pieces per split block: the most of 64 / 32 / 16 with which the misses expected at the
// floor's rank (≈ 2 % of the launch) fill at most one round of workgroup slots (the pass's latency is the length of
// one piece: 82,688 queries 4.86 → 4.60 ms with 32 instead of 16, profiles/r06/ab_floor_p2_quarter.log; 41,344: 64
// pieces 370 → 231 µs, their merge 67 → 145 µs, profiles/r06/timeline_eg_41344_f-_g-_p{32,64}.txt); cfg2's ≈ 5,000
// misses in 21 blocks × 16 pieces fill one round, 32 pieces would take two
constexpr int kFloorP2 = 16, kFloorP2Few = 32, kFloorP2Fewest = 64;
// second pass: up to kFloorSplit blocks (of 256 misses) split into kFloorP2 pieces, any further ones
// whole-table (a floor that cut more than 5 % of cfg2's queries)
constexpr int kFloorSplit = 64;
// The second pass runs at a lower floor, the pilots' smallest estimate − kFloor2Margin, meant to lie below every K-th
// score (cfg2: the smallest of all 330,750 is 1.720; the pilots' smallest estimate is 1.75–1.85 depending on which
// queries they are — with fwav_prune's active-list order margins of 0.06 / 0.10 still cut 11 / 15 queries, and each
// call then paid a cold third pass: tools/diag/floor_misses.py, profiles/r05/floor_misses*.log), so that its table
// pieces do not start cold either; the queries that one cuts (normally none) take a floor-free third pass.  (Full
// score rows for them, launch_topk_large, measured 3.6 ms per launch: one workgroup per row streams it repeatedly.)
constexpr float kFloor2Margin = 0.15f;
// (The later passes in the centroid geometry, on the miss list in its atomic order, measured slower: 330,750 /
// 165,375 / 82,688 / 41,344 queries 14.14 → 14.70 / 7.72 → 8.13 / 4.38 → 4.78 / 2.69 → 3.20 ms, round 6,
// profiles/r06/ab_floor_geo2.log — consecutive misses are unrelated queries, so the centroids' slack is large.)
static_assert(kFloorP2 >= 1 && kFloorP2Fewest <= kMaxPieces, "second-pass pieces outside the merge");
#ifdef FWAV_DEBUG_API
static int g_floor_mode = -1;      // fwav_debug_topk_floor: −1 auto, 0 off, 1 / 3 forced value, 2 pilot at any size
static uint32_t g_floor_key = 0u;
static int g_floor_rank = kFloorRank;
static float g_floor2_margin = kFloor2Margin;
#else
constexpr int g_floor_mode = -1;
constexpr uint32_t g_floor_key = 0u;
constexpr int g_floor_rank = kFloorRank;
constexpr float g_floor2_margin = kFloor2Margin;
#endif
static int floor_mode() { return g_floor_mode; }
// the first pass of max_q queries over nd domains runs with the floor (K ≤ 64, the fp16 search)
static bool floor_by_default(int64_t max_q, int64_t nd) {
  const int fmode = floor_mode();
  return fmode != 0 && (fmode > 0 || (max_q >= kFloorMinQ && nd >= kFloorMinD && nd <= kFloorMaxD));
}
// second-pass plan (base geometry) for a miss list of at most max_q queries: every piece streams ≥ 16 chunks
#ifdef FWAV_DEBUG_API
static int g_floor_p2 = 0;  // fwav_debug_topk_floor_pieces (debug library only; 0: by the launch's size)
#else
constexpr int g_floor_p2 = 0;
#endif
static void floor_plan(int64_t max_q, int64_t nd, int& rt, int& P) {
  rt = kFloorSplit;
  const int64_t pmax = cdiv(nd, kChunk) / 16;
  int cus, per_cu;
  topk_device_slots(kGeoBase, cus, per_cu);
  const int64_t blocks = cdiv(cdiv(max_q > 0 ? max_q : 1, 50), k16QB);  // ≈ 2 % of the launch, in 256-query blocks
  const int64_t slots = (int64_t)cus * per_cu;
  // 64 pieces where they fit one round, else as many from 16 to 32 as fit it (cfg2, ≈ 4,200–5,600 misses, 21–26
  // blocks expected: 19 pieces 13.82 vs 13.87–13.92 ms with 16, and 23 / 26 / 30 faster still on the misses of that
  // run, 17 blocks — but the floor's miss count varies run to run, so the round is sized for the 2 % estimate;
  // profiles/r06/floor_p2_sweep.log)
  const int64_t per = blocks > 0 ? slots / blocks : kFloorP2Fewest;
  const int p2 = g_floor_p2 > 0 ? g_floor_p2
                                : (per >= kFloorP2Fewest ? kFloorP2Fewest
                                                         : (int)std::max<int64_t>(kFloorP2, std::min<int64_t>(per, kFloorP2Few)));
  P = (int)std::max<int64_t>(1, std::min<int64_t>(p2, pmax));
}


// Key-buffer bytes: enough for the first pass in either geometry (a diagnostic override may switch it between the
// size query and the launch), for the relaunches' base plan and for the floor's second pass.
static size_t f16_keys_bytes(int64_t max_q, int64_t nd) {
  const int64_t q = max_q > 0 ? max_q : 1;
  size_t items_q = (size_t)make_plan(q, 0, 1, k16QB).items() * k16QB;
  {
    int rt2, P2;
    floor_plan(q, nd, rt2, P2);
    const size_t n2 = (size_t)make_plan(q, rt2, P2, k16QB).items() * k16QB;
    items_q = n2 > items_q ? n2 : items_q;
  }
  for (int gf = 0; gf < 2 * kGeos; ++gf) {  // each geometry with and without the floor (a debug knob may switch it)
    int rt, P;
    const int geo = gf % kGeos;
    host_plan_for(q, nd, geo, rt, P, gf / kGeos);
    const int qb = geometry_qb(geo);
    const size_t n = (size_t)make_plan(q, rt, P, qb).items() * qb;
    items_q = n > items_q ? n : items_q;
  }
  return items_q * k16Cap * sizeof(uint64_t);
}

// The fp16 search's workspace (K ≤ 64), in byte offsets from its start; one definition for the launch, the size query
// and fwav_debug_sim_topk_layout (tests read the tail through it, never by arithmetic of their own).
//   keys      u64 key buffers (f16_keys_bytes)        share   u32[q] shared band limits of split blocks
//   ovf2      i32[q] overflow list of the HL relaunch  n_ovf2  i32 count, then seeds2 u32[q]
//   ovf1      i32[q] overflow list of the first pass   n_ovf1  i32 count, then seeds1 u32[q]
//   miss      i32[q] floor misses of the first pass    n_miss  i32
//   miss2     i32[q] floor misses of the second pass   n_miss2 i32
//   floor_key u32[2]
//   order     i32[q] the active list in ascending query order (k_order_*), n_order i32[2] its length, a flag
//   order_bits u32[⌈q/32⌉] its bitmap                  order_bsum u32 per 8,192 queries: the bitmap's block counts
//   pilot     f32 pilot scores + estimates (only when the floor can run: floor_by_default, or any size in the debug
//             library)
struct TopkLayout {
  size_t keys, share, ovf2, n_ovf2, seeds2, ovf1, n_ovf1, seeds1, miss, n_miss, miss2, n_miss2, floor_key, order,
      n_order, order_bits, order_bsum, pilot, total;
};
constexpr size_t kPilotBytes = ((size_t)kFloorPilots * kFloorSlices * kFloorJ + kFloorPilots) * sizeof(float);
static TopkLayout topk_layout(int64_t max_q, int64_t nd) {
  const size_t q = (size_t)(max_q > 0 ? max_q : 1);
  TopkLayout L;
  L.keys = 0;
  L.share = f16_keys_bytes(max_q, nd);
  L.ovf2 = L.share + 4 * q;
  L.n_ovf2 = L.ovf2 + 4 * q;
  L.seeds2 = L.n_ovf2 + 4;
  L.ovf1 = L.seeds2 + 4 * q;
  L.n_ovf1 = L.ovf1 + 4 * q;
  L.seeds1 = L.n_ovf1 + 4;
  L.miss = L.seeds1 + 4 * q;
  L.n_miss = L.miss + 4 * q;
  L.miss2 = L.n_miss + 4;
  L.n_miss2 = L.miss2 + 4 * q;
  L.floor_key = L.n_miss2 + 4;
  L.order = L.floor_key + 8;
  L.n_order = L.order + 4 * q;
  L.order_bits = L.n_order + 8;
  L.order_bsum = L.order_bits + 4 * (size_t)order_words(q);
  L.pilot = L.order_bsum + 4 * (size_t)cdiv((int64_t)order_words(q), kOrderWords);
#ifdef FWAV_DEBUG_API
  const bool pilots = true;  // a debug knob may force the floor after the size query
#else
  const bool pilots = floor_by_default(max_q, nd);
#endif
  L.total = L.pilot + (pilots ? kPilotBytes : 0);
  return L;
}

template <int C>
static size_t topk_lds_bytes() {
  return (size_t)kTopkQ * C * sizeof(uint64_t) + 16 * kChunk * sizeof(float) + 3 * kTopkQ * sizeof(int);
}

// XQ: the queries are rows of the table xq (the _q entry points), not of emb / emb16
template <int C, bool XQ = false>
static int launch_topk(const float* emb, const _Float16* emb16, int64_t nd, const int32_t* active,
                       const int32_t* n_active, int64_t max_q, int64_t q_offset, int K, int32_t* cand, hipStream_t st,
                       uint64_t* gkeys, SgemvSplit sp, int32_t* ties, int dbg = 0,
                       unsigned long long* stats = nullptr, QueryTab xq = QueryTab{}) {
  const float* const qemb = XQ ? xq.emb : emb;
  const int64_t grid = cdiv(max_q, kTopkQ);
  if (ties != nullptr) (void)hipMemsetAsync(ties, 0, sizeof(int32_t), st);
  if (grid == 0) return FWAV_OK;
  if (emb16 != nullptr) {
    if (gkeys == nullptr) {
      set_error("fwav_sim_topk: fp16 search needs its key workspace (fwav_sim_topk_workspace_size)");
      return FWAV_ERR_WORKSPACE;
    }
    const int64_t q1 = max_q > 0 ? max_q : 1;
    // workspace tail (TopkLayout): two overflow lists, each list[q], count, seeds u32[q] (seeds[i] = f2key of the
    // band limit of list[i]), the floor's miss lists, its keys and the pilots' scores
    const TopkLayout lay = topk_layout(max_q, nd);
    char* const wb = reinterpret_cast<char*>(gkeys);
    uint32_t* share = reinterpret_cast<uint32_t*>(wb + lay.share);  // u32[q]: shared band limits of split blocks
    int32_t* ovf2 = reinterpret_cast<int32_t*>(wb + lay.ovf2);
    int32_t* n_ovf2 = reinterpret_cast<int32_t*>(wb + lay.n_ovf2);
    int32_t* ovf1 = reinterpret_cast<int32_t*>(wb + lay.ovf1);
    int32_t* n_ovf1 = reinterpret_cast<int32_t*>(wb + lay.n_ovf1);
    const uint32_t* seeds1 = reinterpret_cast<const uint32_t*>(wb + lay.seeds1);
    const uint32_t* seeds2 = reinterpret_cast<const uint32_t*>(wb + lay.seeds2);
    (void)hipMemsetAsync(n_ovf1, 0, sizeof(int32_t), st);
    (void)hipMemsetAsync(n_ovf2, 0, sizeof(int32_t), st);
    // Geometry: k16Waves waves × k16Sets query sets of 32 per workgroup.  Measured at cfg2 (W, QS=1): W = 8
    // 27.9 ms, W = 7 31.6 ms, W = 6 44.5 ms — an even 4 waves per SIMD beats a fuller last round of workgroups.
#ifdef FWAV_DEBUG_API
    const bool stats_first = (stats != nullptr && !(dbg & (1 << 17))) || (dbg & 65535) != 0;
#else
    constexpr bool stats_first = false;  // counter / ablation launches: debug library only
    (void)dbg;
#endif
    // counter builds run the base geometry, or with dbg bit 18 the product's own geometry where it has a counter
    // kernel (Geo::stats)
    int geo = stats_first && !(dbg & (1 << 18)) ? kGeoBase : first_geometry(nd, max_q);
    if (stats_first && !kGeo[geo].stats) geo = kGeoBase;
    const int mode1 = first_mode(nd);
    // the floor's miss lists (first and second pass), its two keys, the pilots' scores
    int32_t* miss = reinterpret_cast<int32_t*>(wb + lay.miss);
    int32_t* n_miss = reinterpret_cast<int32_t*>(wb + lay.n_miss);
    int32_t* miss2 = reinterpret_cast<int32_t*>(wb + lay.miss2);
    int32_t* n_miss2 = reinterpret_cast<int32_t*>(wb + lay.n_miss2);
    uint32_t* floor_key = reinterpret_cast<uint32_t*>(wb + lay.floor_key);
    float* pilot = reinterpret_cast<float*>(wb + lay.pilot);
    // One first pass (search + merge of split blocks) over act[0 .. *nact) in geometry g with plan (rt, P) and floor
    // fl; `diag`: the debug library's counter / ablation launches may replace the search
    // (with a floor the device runs the floor-free plan fl.alt_* when the floor did not apply: the grid, the shared
    // limits and the merge cover both plans)
    auto first_pass = [&](const int32_t* act, const int32_t* nact, int g, int rt, int P, FloorCtl fl, bool diag) {
      fl.seeds = g_seed_mode;
      const TopkPlan pl0 = make_plan(max_q, rt, P, geometry_qb(g));
      const TopkPlan pla = fl.key != nullptr ? make_plan(max_q, fl.alt_rt, fl.alt_p, geometry_qb(g)) : pl0;
      struct {
        int64_t n, R;
        int P;
        int64_t items() const { return n; }
      } pl{std::max(pl0.items(), pla.items()), std::max(pl0.R, pla.R), std::max(pl0.P, pla.P)};
      if ((pl0.R > 0 && !pl0.halves) || (pla.R > 0 && !pla.halves))
        (void)hipMemsetAsync(share, 0, (size_t)q1 * sizeof(uint32_t), st);
      with_geometry(g, mode1, [&](auto gt, auto mt) {
        constexpr Geo ge = kGeo[decltype(gt)::value];
        constexpr int MODE = decltype(mt)::value;
        auto search = [&](auto counters) {
          constexpr bool STATS = decltype(counters)::value;
          k_sim_topk_f16<k16Cap, STATS, MODE, ge.W, ge.G, ge.QS, ge.cent, XQ><<<pl.items(), 64 * ge.W, 0, st>>>(
              emb16, emb, nd, act, nact, q_offset, K, cand, gkeys, ovf1, n_ovf1, share, nullptr, 0.0f, rt, P,
              STATS ? dbg & 65535 : 0, STATS ? stats : nullptr, sp, ties, fl, xq);
        };
        bool counted = false;
#ifdef FWAV_DEBUG_API
        if constexpr (ge.stats) {
          counted = diag && stats_first;
          if (counted) search(std::true_type{});
        }
#endif
        (void)diag;
        if (!counted) search(std::false_type{});
        if (pl.R > 0) {
          // one merge wave per split-block query; the narrowest instantiation that holds the plan's pieces
          auto merge = [&](auto mp) {
            constexpr int QB = ge.qb();
            k_merge_pieces<k16Cap, QB, MODE == kModeHL, decltype(mp)::value><<<cdiv(pl.R * QB, 4), 256, 0, st>>>(
                gkeys, act, nact, rt, P, K, cand, ovf1, n_ovf1, share, emb, q_offset, sp, ties, fl, qemb);
          };
          if (pl.P <= 8) merge(std::integral_constant<int, 8>{});
          else if (pl.P <= 16) merge(std::integral_constant<int, 16>{});
          else if (pl.P <= 32) merge(std::integral_constant<int, 32>{});
          else merge(std::integral_constant<int, kMaxPieces>{});
        }
      });
    };
    // Speculative floor (FloorCtl): from the exact scores of kFloorPilots evenly spaced queries against every
    // (K/8)-th domain (k_floor_pilot), a guess at the lowest K-th score of the search; the queries it may cut are
    // searched again at a lower floor, and the few that one cuts without any (base geometry, table pieces).
    // the centroid geometry's passes on the search's own ascending copy of the caller's active list (order_active;
    // every pass below reads it), where it was measured; the other geometries on the caller's order (ascending ids
    // are not better everywhere: cfg3's sliced search on ascending slices ran 373 instead of 347 ms per step,
    // profiles/r06/active_order/cfg3_*.log)
    const int32_t* order = active;
    const int32_t* n_order = n_active;
    if (geo_is_cent(geo)) {
      int32_t* const ord = reinterpret_cast<int32_t*>(wb + lay.order);
      int32_t* const n_ord = reinterpret_cast<int32_t*>(wb + lay.n_order);
      order_active(active, n_active, max_q, reinterpret_cast<uint32_t*>(wb + lay.order_bits),
                   reinterpret_cast<uint32_t*>(wb + lay.order_bsum), ord, n_ord, st);
      order = ord;
      n_order = n_ord;
    }
    const int fmode = floor_mode();
    // (counter launches run without the floor unless dbg bit 19 asks for the product's floor too)
    const bool use_floor = (!stats_first || (dbg & (1 << 19))) && K <= 64 && floor_by_default(max_q, nd);
    int rt, P;
    host_plan_for(max_q, nd, geo, rt, P, use_floor ? 1 : 0);
    FloorCtl fl{nullptr, nullptr, nullptr};
    if (use_floor) {
      (void)hipMemsetAsync(n_miss, 0, sizeof(int32_t), st);
      (void)hipMemsetAsync(n_miss2, 0, sizeof(int32_t), st);
      if (fmode == 1 || fmode == 3) {  // debug: a forced floor value (3: the second pass's too)
        (void)hipMemsetD32Async((hipDeviceptr_t)floor_key, (int)g_floor_key, 1, st);
        (void)hipMemsetD32Async((hipDeviceptr_t)(floor_key + 1), fmode == 3 ? (int)g_floor_key : 0, 1, st);
      } else {
        const int j = K < kFloorJ ? K : kFloorJ, stride = K / j;
        float* est = pilot + (size_t)kFloorPilots * kFloorSlices * kFloorJ;
        k_floor_pilot<<<kPilotGroups * kFloorSlices, 256, 0, st>>>(emb, nd, order, n_order, q_offset, stride, pilot,
                                                                   qemb);
        k_floor_est<<<kFloorPilots, 64, 0, st>>>(pilot, kFloorSlices, j, est);
        k_floor_reduce<<<1, kFloorPilots, 0, st>>>(est, g_floor_rank, n_order, fmode == 2 ? 0 : (int)kFloorMinQ,
                                                   g_floor2_margin, floor_key);
      }
      int rt_nf, P_nf;  // the plan when the device finds the floor does not apply
      host_plan_for(max_q, nd, geo, rt_nf, P_nf, 0);
      fl = FloorCtl{floor_key, miss, n_miss, rt_nf, P_nf};
    }
    first_pass(order, n_order, geo, rt, P, fl, true);
    if (use_floor) {
      int rt2, P2;
      floor_plan(max_q, nd, rt2, P2);
      first_pass(miss, n_miss, kGeoBase, rt2, P2, FloorCtl{floor_key + 1, miss2, n_miss2, rt2, P2}, false);
      first_pass(miss2, n_miss2, kGeoBase, rt2, P2, FloorCtl{nullptr, nullptr, nullptr}, false);
    }
    // Queries whose band overflowed the buffer (large groups of equal or nearly equal scores) are searched again by
    // the same kernel in a narrower mode, on the device-side overflow list (no host sync; a relaunch exits at once
    // when its list is empty): after an S16 first pass the HL mode, then the exact mode for what still overflows;
    // after an HL first pass the exact mode, whose compactions keep exactly the top K, so nothing overflows.
    const TopkPlan pl_re = make_plan(max_q, 0, 1, k16QB);
    const int32_t* ex_in = ovf1;
    const int32_t* ex_n = n_ovf1;
    const uint32_t* ex_seeds = seeds1;
    if (mode1 == kModeS16) {
      k_sim_topk_f16<k16Cap, false, kModeHL, k16Waves, kGroup, k16Sets, false, XQ><<<pl_re.items(), 64 * k16Waves, 0, st>>>(
          emb16, emb, nd, ovf1, n_ovf1, q_offset, K, cand, gkeys, ovf2, n_ovf2, nullptr, seeds1, kStreamMargin, 0, 1, 0,
          nullptr, sp, ties, FloorCtl{nullptr, nullptr, nullptr}, xq);
      ex_in = ovf2;
      ex_n = n_ovf2;
      ex_seeds = seeds2;
    }
#ifdef FWAV_DEBUG_API
    if (stats != nullptr && (dbg & (1 << 17)))  // diagnostic: counters of the exact-mode relaunch only
      k_sim_topk_f16<k16Cap, true, kModeEX, k16Waves, kGroup, k16Sets, false, XQ><<<pl_re.items(), 64 * k16Waves, 0, st>>>(
          emb16, emb, nd, ex_in, ex_n, q_offset, K, cand, gkeys, ovf2, n_ovf2, nullptr, ex_seeds, kStreamMargin, 0, 1, 0,
          stats, sp, ties, FloorCtl{nullptr, nullptr, nullptr}, xq);
    else
#endif
      k_sim_topk_f16<k16Cap, false, kModeEX, k16Waves, kGroup, k16Sets, false, XQ><<<pl_re.items(), 64 * k16Waves, 0, st>>>(
          emb16, emb, nd, ex_in, ex_n, q_offset, K, cand, gkeys, ovf2, n_ovf2, nullptr, ex_seeds, kStreamMargin, 0, 1, 0,
          nullptr, sp, ties, FloorCtl{nullptr, nullptr, nullptr}, xq);
  } else {
    const size_t lds = topk_lds_bytes<C>();
    static bool attr32[kMaxDev] = {false};  // a function attribute is set per device
    const int dev = current_device();
    if (!attr32[dev]) {
      (void)hipFuncSetAttribute((const void*)k_sim_topk_f32<C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      attr32[dev] = true;
    }
    k_sim_topk_f32<C><<<grid, kTopkThreads, lds, st>>>(emb, nd, active, n_active, q_offset, K, cand, sp, ties, qemb);
  }
  FWAV_LAUNCH_CHECK("fwav_sim_topk");
  return FWAV_OK;
}

// fwav_topk_large.hip (K > 64)
int64_t large_batch(int64_t nd, int64_t max_q);
size_t large_workspace_bytes(int64_t nd, int64_t max_q);
int launch_topk_large(const float* emb, int64_t nd, const int32_t* active, const int32_t* n_active, int64_t max_q,
                      int64_t q_offset, int K, int32_t* cand, float* S, SgemvSplit sp, int32_t* ties, hipStream_t st);
int launch_score_rows(const float* emb, int64_t nd, const int32_t* rows, int64_t n_rows, int64_t q_offset,
                      SgemvSplit sp, float* S, hipStream_t st, const float* qemb);  // (qemb NULL: the rows of emb)

}  // namespace fwav

using namespace fwav;

extern "C" {

int fwav_topk_max_k(void) { return 4096; }

int64_t fwav_tie_list_size(int64_t max_q) { return 1 + (int64_t)kTieRec * (max_q > 0 ? max_q : 1); }

// Workspace of fwav_sim_topk: for K <= 64 the fp16 search's global key buffers (max_q queries), for K > 64
// the score rows of one query batch (≤ 1 GiB).
size_t fwav_sim_topk_workspace_size(int64_t max_q, int64_t n_domains, int k) {
  const int64_t q = max_q > 0 ? max_q : 1;
  if (k > 64) return large_workspace_bytes(n_domains, q);
  // key buffers, shared limits u32[q], two overflow lists (list, count, seeds), the floor's two miss lists (list,
  // count), its two keys, the pilots' scores when the floor can run (TopkLayout)
  return topk_layout(q, n_domains).total;
}

// Exact top-K over all nd domains for the local queries listed in active[0 .. *n_active) (device count,
// at most max_q); local query i uses embedding row q_offset + i and writes cand row i.  Rows of queries
// not listed are not touched.  emb16 (tiled fp16 copy from fwav_pool_embed) selects the fp16 pre-filter
// kernel; NULL runs the all-f32-MFMA kernel.  Both return identical candidates.
int fwav_sim_topk(const float* emb, const void* emb16, int64_t nd, const int32_t* active, const int32_t* n_active,
                  int64_t max_q, int64_t q_offset, int K, int blas_threads, int32_t* cand, int32_t* ties,
                  void* workspace, size_t ws_bytes, void* stream) {
  FWAV_CHECK_ARG(emb && active && n_active && cand && nd > 0 && max_q >= 0, FWAV_ERR_ARG, "fwav_sim_topk: bad args");
  FWAV_CHECK_ARG(blas_threads >= 1 && blas_threads <= 4096, FWAV_ERR_ARG, "fwav_sim_topk: blas_threads outside [1, 4096]");
  FWAV_CHECK_ARG(K >= 1 && K <= fwav_topk_max_k(), FWAV_ERR_K, "fwav_sim_topk: K=%d outside [1, %d]", K,
                 fwav_topk_max_k());
  FWAV_CHECK_ARG(nd < (int64_t)0x7fffffff, FWAV_ERR_SHAPE, "fwav_sim_topk: nd too large");
  hipStream_t st = (hipStream_t)stream;
  if (K > 64) {
    FWAV_CHECK_ARG(workspace && ws_bytes >= fwav_sim_topk_workspace_size(max_q, nd, K), FWAV_ERR_WORKSPACE,
                   "fwav_sim_topk: workspace too small");
    if (ties != nullptr) (void)hipMemsetAsync(ties, 0, sizeof(int32_t), st);
    if (max_q == 0) return FWAV_OK;
    return launch_topk_large(emb, nd, active, n_active, max_q, q_offset, K, cand, (float*)workspace,
                             make_sgemv_split(nd, blas_threads), ties, st);
  }
  FWAV_CHECK_ARG(emb16 == nullptr || (workspace && ws_bytes >= fwav_sim_topk_workspace_size(max_q, nd, K)),
                 FWAV_ERR_WORKSPACE, "fwav_sim_topk: workspace too small");
  return launch_topk<128>(emb, (const _Float16*)emb16, nd, active, n_active, max_q, q_offset, K, cand, st,
                          (uint64_t*)workspace, make_sgemv_split(nd, blas_threads), ties);
}

// Exact reference score rows for the host's tie resolution: scores[i·nd + d] = emb[d] · emb[q_offset + rows[i]] in
// the reference's sgemv order for `blas_threads` OpenBLAS threads (fractal.py:537).
int fwav_score_rows(const float* emb, int64_t nd, const int32_t* rows, int64_t n_rows, int64_t q_offset,
                    int blas_threads, float* scores, void* stream) {
  FWAV_CHECK_ARG(emb && rows && scores && nd > 0 && nd < (int64_t)0x7fffffff && n_rows >= 0, FWAV_ERR_ARG,
                 "fwav_score_rows: bad args");
  FWAV_CHECK_ARG(blas_threads >= 1 && blas_threads <= 4096, FWAV_ERR_ARG, "fwav_score_rows: blas_threads outside [1, 4096]");
  if (n_rows == 0) return FWAV_OK;
  return launch_score_rows(emb, nd, rows, n_rows, q_offset, make_sgemv_split(nd, blas_threads), scores,
                           (hipStream_t)stream, nullptr);
}

// ---- the search with a query table of its own (include/fwav.h, "queries from another table")
// The shared argument checks of fwav_sim_topk_q and fwav_debug_sim_topk_q (host only), and the kernels' QueryTab.
static int query_tab(const char* what, const float* emb, const void* emb16, int64_t nd, const float* qemb,
                     const void* qemb16, int64_t n_query_rows, int seed_stride, int64_t max_q, int64_t q_offset, int K,
                     QueryTab& xq) {
  FWAV_CHECK_ARG(emb && qemb && nd > 0 && max_q >= 0, FWAV_ERR_ARG, "%s: bad args", what);
  FWAV_CHECK_ARG((emb16 == nullptr) == (qemb16 == nullptr), FWAV_ERR_ARG,
                 "%s: emb16 and qemb16 go together (both for the fp16 search, neither for the all-f32 one)", what);
  FWAV_CHECK_ARG(n_query_rows > 0 && n_query_rows < (int64_t)0x7fffffff && q_offset >= 0 && q_offset < n_query_rows,
                 FWAV_ERR_SHAPE, "%s: q_offset %lld outside the %lld query rows", what, (long long)q_offset,
                 (long long)n_query_rows);
  FWAV_CHECK_ARG(seed_stride >= 0, FWAV_ERR_ARG, "%s: negative seed_stride", what);
  FWAV_CHECK_ARG(K >= 1 && K <= 64, FWAV_ERR_K, "%s: K=%d outside [1, 64]", what, K);
  FWAV_CHECK_ARG(nd < (int64_t)0x7fffffff, FWAV_ERR_SHAPE, "%s: nd too large", what);
  const _Float16* q16 = (const _Float16*)qemb16;
  // (the tiled table's low parts follow its high parts: ceil(n_query_rows / 256)·256·16 halfs each, fwav_emb16_elems)
  xq = QueryTab{qemb, q16, q16 != nullptr ? q16 + cdiv(n_query_rows, kChunk) * kChunk * 16 : nullptr, seed_stride};
  return FWAV_OK;
}

int fwav_sim_topk_q(const float* emb, const void* emb16, int64_t nd, const float* qemb, const void* qemb16,
                    int64_t n_query_rows, int seed_stride, const int32_t* active, const int32_t* n_active,
                    int64_t max_q, int64_t q_offset, int K, int blas_threads, int32_t* cand, int32_t* ties,
                    void* workspace, size_t ws_bytes, void* stream) {
  QueryTab xq;
  const int rc = query_tab("fwav_sim_topk_q", emb, emb16, nd, qemb, qemb16, n_query_rows, seed_stride, max_q, q_offset,
                           K, xq);
  if (rc != FWAV_OK) return rc;
  FWAV_CHECK_ARG(active && n_active && cand, FWAV_ERR_ARG, "fwav_sim_topk_q: bad args");
  FWAV_CHECK_ARG(blas_threads >= 1 && blas_threads <= 4096, FWAV_ERR_ARG,
                 "fwav_sim_topk_q: blas_threads outside [1, 4096]");
  FWAV_CHECK_ARG(emb16 == nullptr || (workspace && ws_bytes >= fwav_sim_topk_workspace_size(max_q, nd, K)),
                 FWAV_ERR_WORKSPACE, "fwav_sim_topk_q: workspace too small");
  return launch_topk<128, true>(emb, (const _Float16*)emb16, nd, active, n_active, max_q, q_offset, K, cand,
                                (hipStream_t)stream, (uint64_t*)workspace, make_sgemv_split(nd, blas_threads), ties, 0,
                                nullptr, xq);
}

int fwav_score_rows_q(const float* emb, int64_t nd, const float* qemb, const int32_t* rows, int64_t n_rows,
                      int64_t q_offset, int blas_threads, float* scores, void* stream) {
  FWAV_CHECK_ARG(emb && qemb && rows && scores && nd > 0 && nd < (int64_t)0x7fffffff && n_rows >= 0 && q_offset >= 0,
                 FWAV_ERR_ARG, "fwav_score_rows_q: bad args");
  FWAV_CHECK_ARG(blas_threads >= 1 && blas_threads <= 4096, FWAV_ERR_ARG,
                 "fwav_score_rows_q: blas_threads outside [1, 4096]");
  if (n_rows == 0) return FWAV_OK;
  return launch_score_rows(emb, nd, rows, n_rows, q_offset, make_sgemv_split(nd, blas_threads), scores,
                           (hipStream_t)stream, qemb);
}

#ifdef FWAV_DEBUG_API  // ---- debug library only (include/fwav_debug.h)
// Diagnostic ablations of the fp16 search kernel (timing only; see k_sim_topk_f16 `dbg`).
int fwav_debug_sim_topk(const float* emb, const void* emb16, int64_t nd, const int32_t* active, const int32_t* n_active,
                        int64_t max_q, int64_t q_offset, int K, int32_t* cand, void* workspace, size_t ws_bytes, int dbg,
                        unsigned long long* stats, void* stream) {
  FWAV_CHECK_ARG(emb && emb16 && workspace && K >= 1 && K <= 64, FWAV_ERR_ARG, "fwav_debug_sim_topk: bad args");
  // the key buffers depend on the work plan of THIS max_q (a split plan for fewer queries can need more than a
  // whole-block plan for more): a workspace sized for another query count once ran off its end
  FWAV_CHECK_ARG(ws_bytes >= fwav_sim_topk_workspace_size(max_q, nd, K), FWAV_ERR_WORKSPACE,
                 "fwav_debug_sim_topk: workspace too small for max_q=%lld", (long long)max_q);
  return launch_topk<128>(emb, (const _Float16*)emb16, nd, active, n_active, max_q, q_offset, K, cand,
                          (hipStream_t)stream, (uint64_t*)workspace, make_sgemv_split(nd, 1), nullptr, dbg, stats);
}

// fwav_debug_sim_topk with the queries of fwav_sim_topk_q: the forced geometry, mode, floor and plan apply alike.
int fwav_debug_sim_topk_q(const float* emb, const void* emb16, int64_t nd, const float* qemb, const void* qemb16,
                          int64_t n_query_rows, int seed_stride, const int32_t* active, const int32_t* n_active,
                          int64_t max_q, int64_t q_offset, int K, int32_t* cand, void* workspace, size_t ws_bytes,
                          int dbg, unsigned long long* stats, void* stream) {
  FWAV_CHECK_ARG(emb16 && qemb16 && workspace && active && n_active && cand, FWAV_ERR_ARG,
                 "fwav_debug_sim_topk_q: bad args");
  QueryTab xq;
  const int rc = query_tab("fwav_debug_sim_topk_q", emb, emb16, nd, qemb, qemb16, n_query_rows, seed_stride, max_q,
                           q_offset, K, xq);
  if (rc != FWAV_OK) return rc;
  FWAV_CHECK_ARG(ws_bytes >= fwav_sim_topk_workspace_size(max_q, nd, K), FWAV_ERR_WORKSPACE,
                 "fwav_debug_sim_topk_q: workspace too small for max_q=%lld", (long long)max_q);
  return launch_topk<128, true>(emb, (const _Float16*)emb16, nd, active, n_active, max_q, q_offset, K, cand,
                                (hipStream_t)stream, (uint64_t*)workspace, make_sgemv_split(nd, 1), nullptr, dbg, stats,
                                xq);
}

// The table row at which fwav_sim_topk_q's first pass centres the seed window of query row `row` (the kernels' own
// seed_centre, on the host): min(row·seed_stride, n_domains − 1).
int64_t fwav_debug_seed_centre(int64_t row, int seed_stride, int64_t nd) {
  if (row < 0 || seed_stride < 0 || nd <= 0) return -1;
  QueryTab xq;
  xq.seed_stride = seed_stride;
  return seed_centre<true>(row, xq, nd);
}

// Diagnostic override of the first pass's mode: 0 = S16 (→ HL → exact relaunches), 1 = HL (→ exact), −1 = by table
// size (default).  Every mode returns the same candidates.
int fwav_debug_topk_mode(int mode) {
  FWAV_CHECK_ARG(mode >= -1 && mode <= 1, FWAV_ERR_ARG, "fwav_debug_topk_mode: mode outside [-1, 1]");
  g_first_mode = mode;
  return FWAV_OK;
}

// Diagnostic override of the first pass's geometry: 0 = base (8 waves, 256 queries per workgroup), 1 = wide (16
// waves, 512 queries, one workgroup per CU), −1 = by table size (default).  Both return the same candidates.
int fwav_debug_topk_geometry(int wide) {
  FWAV_CHECK_ARG(wide >= -1 && wide < kGeoCodes, FWAV_ERR_ARG, "fwav_debug_topk_geometry: outside [-1, 3]");
  g_wide = wide;
  return FWAV_OK;
}

// Diagnostic override of the centroid geometry's query sets per wave (include/fwav_debug.h): 2, 4, −1 = by the query
// count (default).
int fwav_debug_topk_cent_sets(int sets) {
  FWAV_CHECK_ARG(sets == -1 || sets == 2 || sets == 4, FWAV_ERR_ARG, "fwav_debug_topk_cent_sets: not -1, 2 or 4");
  g_cent_sets = sets;
  return FWAV_OK;
}

// Diagnostic override of the speculative floor (include/fwav_debug.h).
int fwav_debug_topk_floor(int mode, float value) {
  FWAV_CHECK_ARG(mode >= -1 && mode <= 4, FWAV_ERR_ARG, "fwav_debug_topk_floor: mode outside [-1, 4]");
  FWAV_CHECK_ARG(mode != 4 || (value >= 0.0f && value < 4.0f), FWAV_ERR_ARG,
                 "fwav_debug_topk_floor: the second pass's margin must lie in [0, 4)");
  FWAV_CHECK_ARG((mode != 1 && mode != 3) || (value == value && value > -INFINITY && value < INFINITY), FWAV_ERR_ARG,
                 "fwav_debug_topk_floor: the forced floor must be finite");
  g_floor_mode = mode == 4 ? 2 : mode;
  g_floor2_margin = mode == 4 ? value : kFloor2Margin;
  g_floor_rank = mode == 2 && value >= 1.0f && value <= (float)kFloorPilots ? (int)value : kFloorRank;
  uint32_t u;
  std::memcpy(&u, &value, sizeof u);
  g_floor_key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // f2key
  return FWAV_OK;
}

// Diagnostic override of the first passes' seed policy (include/fwav_debug.h): 0 = probe at the floor, then search
// (the default), 1 = always search, 2 = never seed.
int fwav_debug_topk_seeds(int mode) {
  FWAV_CHECK_ARG(mode >= 0 && mode <= 2, FWAV_ERR_ARG, "fwav_debug_topk_seeds: mode outside [0, 2]");
  g_seed_mode = mode;
  return FWAV_OK;
}

// Diagnostic override of the floor's second-pass table pieces per split block (1 … 64; 0: by the launch's size, the
// default).  Re-query fwav_sim_topk_workspace_size afterwards.
int fwav_debug_topk_floor_pieces(int p2) {
  FWAV_CHECK_ARG(p2 >= 0 && p2 <= kMaxPieces, FWAV_ERR_ARG, "fwav_debug_topk_floor_pieces: outside [0, %d]", kMaxPieces);
  g_floor_p2 = p2;
  return FWAV_OK;
}

// Host-side check of the work plan (no device needed): for every item of the plan of n queries (rt, pieces as in
// fwav_debug_topk_plan; wide: the 16-wave geometry) and every query slot its workgroup runs, count[position] += 1.
// A query of a whole-table block or a query half must be counted once, one of a block split into P table pieces P
// times.  *items = the launch's grid.
int fwav_debug_topk_plan_cover(int64_t n, int rt, int pieces, int wide, int32_t* count, int64_t* items) {
  FWAV_CHECK_ARG(n >= 0 && count && items && wide >= 0 && wide < kGeoCodes &&
                     (pieces == -1 || (pieces >= 1 && pieces <= kMaxPieces)), FWAV_ERR_ARG,
                 "fwav_debug_topk_plan_cover: bad args");  // (any plan's pieces: the floor's later passes take 16)
  // 0 base, 1 wide, 2 centroid, 3 centroid wide (and the 4-set centroid geometry's layout)
  const int W = kGeo[wide].W, sets = kGeo[wide].QS, qb = kGeo[wide].qb();
  const TopkPlan pl = make_plan(n, rt, pieces, qb);
  *items = pl.items();
  for (int64_t it = 0; it < pl.items(); ++it) {
    int64_t block;
    int piece, np, qhalf;
    plan_item(pl, it, block, piece, np, qhalf);
    if (block >= pl.nb) continue;
    const int wact = qhalf < 0 ? W : W / 2;
    const int qslot0 = qhalf > 0 ? (W / 2) * sets * 32 : 0;
    for (int ql = 0; ql < wact * sets * 32; ++ql) {
      const int64_t qi = slot_query(block, qslot0 + ql, pl.nb);
      if (qi < n) ++count[qi];
    }
  }
  return FWAV_OK;
}

// The first pass fwav_sim_topk would launch for max_q queries over nd domains on the current device (no launch):
// geometry (1 = wide), first-pass mode (0 = S16, 1 = HL), whole-table blocks F, split blocks R, pieces P (−1: query
// halves), grid.
// The default first-pass plan's chunk range of every table piece of split block `block` (mod the split blocks;
// piece_chunks, with the floor as the launch would decide it): c01[2p], c01[2p + 1] = [c0, c1) of piece p < *np (at
// most kMaxPieces); *np = 1 for an unsplit plan.
int fwav_debug_topk_piece_chunks(int64_t max_q, int64_t nd, int64_t block, int32_t* c01, int32_t* np) {
  FWAV_CHECK_ARG(max_q > 0 && nd > 0 && block >= 0 && c01 && np, FWAV_ERR_ARG, "fwav_debug_topk_piece_chunks: bad args");
  const int geo = first_geometry(nd, max_q);
  int rt, P;
  host_plan_for(max_q, nd, geo, rt, P);
  const TopkPlan pl = make_plan(max_q, rt, P, geometry_qb(geo));
  const int n = pl.halves || pl.R == 0 ? 1 : pl.P;
  const int nchunks = (int)cdiv(nd, kChunk);
  const int64_t b = pl.F + (pl.R > 0 ? block % pl.R : 0);  // a split block
  for (int p = 0; p < n; ++p) piece_chunks(pl, b, p, n, nchunks, c01[2 * p], c01[2 * p + 1]);
  *np = n;
  return FWAV_OK;
}

int fwav_debug_topk_plan_info(int64_t max_q, int64_t nd, int32_t* info, int64_t* blocks) {
  FWAV_CHECK_ARG(max_q >= 0 && nd > 0 && info && blocks, FWAV_ERR_ARG, "fwav_debug_topk_plan_info: bad args");
  const int geo = first_geometry(nd, max_q);
  int rt, P;
  host_plan_for(max_q, nd, geo, rt, P);
  const TopkPlan pl = make_plan(max_q, rt, P, geometry_qb(geo));
  info[0] = geo_code(geo);
  info[1] = first_mode(nd);
  info[2] = pl.halves ? -1 : pl.P;
  blocks[0] = pl.F;
  blocks[1] = pl.R;
  blocks[2] = pl.items();
  return FWAV_OK;
}

// Queries per block (one workgroup's query slots) of first-pass geometry geo (0 base, 1 wide, 2 centroid, 3 centroid
// wide).
int64_t fwav_debug_topk_qb(int geo) { return geo >= 0 && geo < kGeoCodes ? geometry_qb(geo) : -1; }

// Byte offsets of the fp16 search's workspace regions for max_q queries over nd domains (K ≤ 64), in the order of
// TopkLayout: keys, share, ovf2, n_ovf2, seeds2, ovf1, n_ovf1, seeds1, miss, n_miss, miss2, n_miss2, floor_key,
// order, n_order, order_bits, order_bsum, pilot, total (19 values; total = fwav_sim_topk_workspace_size of this
// library).
int fwav_debug_sim_topk_layout(int64_t max_q, int64_t nd, int64_t* offsets) {
  FWAV_CHECK_ARG(max_q >= 0 && nd > 0 && offsets, FWAV_ERR_ARG, "fwav_debug_sim_topk_layout: bad args");
  const TopkLayout L = topk_layout(max_q > 0 ? max_q : 1, nd);
  const size_t v[19] = {L.keys,      L.share, L.ovf2,    L.n_ovf2,     L.seeds2,     L.ovf1,  L.n_ovf1,
                        L.seeds1,    L.miss,  L.n_miss,  L.miss2,      L.n_miss2,    L.floor_key, L.order,
                        L.n_order,   L.order_bits,       L.order_bsum, L.pilot,      L.total};
  for (int i = 0; i < 19; ++i) offsets[i] = (int64_t)v[i];
  return FWAV_OK;
}

// Diagnostic override of the fp16 search's work plan (rt < 0: default policy).  Re-query
// fwav_sim_topk_workspace_size after changing it.
int fwav_debug_topk_tail(int wb) {
  FWAV_CHECK_ARG(wb >= -1 && wb <= 31, FWAV_ERR_ARG, "fwav_debug_topk_tail: weight outside [-1, 31]");
  g_tail_wb = wb;
  return FWAV_OK;
}

int fwav_debug_topk_plan(int rt, int pieces) {
  FWAV_CHECK_ARG(pieces == -1 || (pieces >= 1 && pieces <= kMaxPieces), FWAV_ERR_ARG,
                 "fwav_debug_topk_plan: pieces outside [1, %d] (or -1: query halves)", kMaxPieces);
  g_plan_rt = rt;
  g_plan_p = rt < 0 ? -1 : pieces;
  return FWAV_OK;
}

#endif  // FWAV_DEBUG_API

}  // extern "C"
