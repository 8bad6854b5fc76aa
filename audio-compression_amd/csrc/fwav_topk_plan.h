// fwav_topk_plan.h — the work plan of the fp16 search (host and device).
// Part of fwav_topk.hip's translation unit: included there, inside namespace fwav, after the shared constants
// and the headers before it (the file map at the top of fwav_topk.hip); not a header for any other file.
#pragma once

// Work plan of the fp16 search.  The n_blocks query blocks are items of one launch, dispatched in order: the first
// F = nb − R blocks stream the whole table, then each of the last R = min(nb, rt) blocks is split into P pieces of
// the table (contiguous chunk ranges) so that the launch's tail is made of short items: without the split the last
// round of whole-table workgroups runs on a fraction of the slots and takes ≈ 1/5 of the kernel.  A piece ends with
// its exact top K (f32 keys, sorted), and k_merge_pieces merges a split block's P lists.  Each item owns one
// key-buffer region (QB queries × C entries).  Every workgroup recomputes the plan from the device-side active
// count, so the launch needs no host sync; the grid and workspace cover the plan of max_q.
// P < 0 selects query halves instead of table pieces: each of the last R blocks becomes two items of half its
// queries (W/2 waves, the other waves exit at once) that stream the whole table — no merge, no restarted limits, and a
// half block on a CU of its own runs its waves faster than a full block.
// Piece-major order (pm) of the split blocks: split item j is piece j / R of block F + j % R, so the first round runs
// the first pieces of all blocks and a later piece of a block starts after its earlier pieces have published their
// limits.
constexpr int kOldWeight = 17, kYoungWeight = 15;  // piece_chunks: a CU's older / younger workgroup
struct TopkPlan {
  int64_t nb, F, R;
  int P, qb;
  // two-class table split (piece_chunks): pieces [0, young) weigh wa, [young, P) wb (young 0: an even split)
  int young, wa, wb;
  // one-round plans (bit 30 of P): the first item index that starts as its CU's younger workgroup (0: none); each
  // block's pieces weigh kOldWeight / kYoungWeight by their own items' side of it
  int ybound;
  bool halves, pm;
  __host__ __device__ int64_t items() const { return F + R * P; }
  // the item of table piece p of split block b
  __host__ __device__ int64_t item_of(int64_t b, int p) const { return pm ? F + (int64_t)p * R + (b - F) : F + (b - F) * P + p; }
};
// P: table pieces per split block, −1 for query halves; bits 8 and up: TopkPlan::young (plan_young)
__host__ __device__ inline TopkPlan make_plan(int64_t n_queries, int rt, int P, int qb) {
  TopkPlan pl;
  pl.qb = qb;
  pl.nb = cdiv(n_queries > 0 ? n_queries : 0, qb);
  const bool by_item = P > 0 && ((P >> 30) & 1);
  pl.ybound = by_item ? ((P >> 8) & 0xFFF) : 0;  // bits 8–19
  pl.young = P > 0 && !by_item ? ((P >> 8) & 0xFF) : 0;
  pl.wb = P > 0 && !by_item ? ((P >> 16) & 0x1F) : 0;  // bits 16–20 / 21–25: the weights (0: the younger pair)
  pl.wa = P > 0 && !by_item ? ((P >> 21) & 0x1F) : 0;
  if (pl.wa == 0 || pl.wb == 0) {
    pl.wa = kOldWeight;
    pl.wb = kYoungWeight;
  }
  P = P > 0 ? (P & 0xFF) : P;
  pl.halves = P < 0;
  pl.P = pl.halves ? 2 : (P < 1 ? 1 : (P > kMaxPieces ? kMaxPieces : P));
  pl.R = pl.P == 1 ? 0 : (pl.nb < rt ? pl.nb : (int64_t)rt);
  pl.F = pl.nb - pl.R;
  pl.pm = !pl.halves && pl.P > 1 && pl.R > 0;
  return pl;
}
// Chunk range [c0, c1) of table piece `piece` of `np`.  Even, unless the plan is one round of workgroups two to a CU
// (TopkPlan::young): a CU's younger workgroup loses the issue arbitration to its older one (oldest-first) and ran
// its piece 13 % longer (41,344 queries, pieces 3–5 vs 0–2: 1.95 vs 1.72 ms median, tools/topk_timeline.py TL_R,
// profiles/r06/timeline_pieces_eighth.log), so the older pieces take 17 / 16 of the mean and the younger 15 / 16.
__host__ __device__ inline void piece_chunks(const TopkPlan& pl, int64_t block, int piece, int np, int nchunks, int& c0,
                                             int& c1) {
  if (pl.ybound > 0 && np == pl.P && block >= pl.F) {
    // by each piece's own item: older (item < ybound) kOldWeight, younger kYoungWeight
    int64_t a = 0, tot = 0;
    for (int p = 0; p < np; ++p) {
      const int w = pl.item_of(block, p) < pl.ybound ? kOldWeight : kYoungWeight;
      if (p < piece) a += w;
      tot += w;
    }
    const int w = pl.item_of(block, piece) < pl.ybound ? kOldWeight : kYoungWeight;
    c0 = (int)((int64_t)nchunks * a / tot);
    c1 = (int)((int64_t)nchunks * (a + w) / tot);
    return;
  }
  if (pl.young <= 0 || pl.young >= np || np != pl.P) {
    c0 = (int)((int64_t)nchunks * piece / np);
    c1 = (int)((int64_t)nchunks * (piece + 1) / np);
    return;
  }
  auto cum = [&](int p) -> int64_t {
    return p <= pl.young ? (int64_t)p * pl.wa : (int64_t)pl.young * pl.wa + (int64_t)(p - pl.young) * pl.wb;
  };
  const int64_t tot = cum(np);
  c0 = (int)((int64_t)nchunks * cum(piece) / tot);
  c1 = (int)((int64_t)nchunks * cum(piece + 1) / tot);
}
// Query (position in the active list) of slot ql = group·32 + col of query block `block`.  Interleaved: a block's
// query groups come from different regions of the list (group g of block b is query group g·nb + b), so every block
// mixes regions and block run times even out, which shortens the launch's tail.
__host__ __device__ inline int64_t slot_query(int64_t block, int ql, int64_t nb) {
  return ((int64_t)(ql >> 5) * nb + block) * 32 + (ql & 31);
}
// item → (block, table piece, table pieces, query half: −1 = the whole block)
__host__ __device__ inline void plan_item(const TopkPlan& pl, int64_t item, int64_t& block, int& piece, int& np,
                                          int& qhalf) {
  qhalf = -1;
  if (item < pl.F) {
    block = item; piece = 0; np = 1;
  } else {
    const int64_t j = item - pl.F;
    block = pl.F + j / pl.P;
    if (pl.halves) {
      piece = 0; np = 1; qhalf = (int)(j % 2);
    } else if (pl.pm) {
      // items past this plan (the grid covers the plan of max_q, the device count may be smaller) map to no block
      block = j < pl.R * pl.P ? pl.F + j % pl.R : pl.nb;
      piece = j < pl.R * pl.P ? (int)(j / pl.R) : 0; np = pl.P;
    } else {
      piece = (int)(j % pl.P); np = pl.P;
    }
  }
}
