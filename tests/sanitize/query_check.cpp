// Host-side sanitizer check of the entry points that take a query table of their own (include/fwav.h, "queries from a
// table of their own"; compress_audio(query="range")): their argument checks, the seed window's centre — row ·
// seed_stride clamped into the table, through the kernels' own code — and the work plan and workspace when the query
// rows outnumber the domains.  Built like plan_check.cpp (tests/test_sanitize_query.py: every .hip source with
// AddressSanitizer + UndefinedBehaviorSanitizer on the host side only) and run on the CPU; every call below returns
// before any kernel launch.  Exit 0 = every check held and no sanitizer report.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/fwav_debug.h"

static int g_fail = 0;
#define CHECK(c, ...)                                           \
  do {                                                          \
    if (!(c)) {                                                 \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                        \
      std::fprintf(stderr, "\n");                               \
      ++g_fail;                                                 \
    }                                                           \
  } while (0)

int main() {
  void* p = reinterpret_cast<void*>(64);
  const float* fp = static_cast<const float*>(p);
  int32_t* ip = static_cast<int32_t*>(p);
  float* wp = static_cast<float*>(p);
  const int imax = std::numeric_limits<int>::max();

  // ---- the seed window's centre: min(row · stride, nd − 1), no overflow at the largest legal arguments
  long centres = 0;
  const int64_t nds[] = {1, 40, 77, 257, 21027, 1321977, 86398977, 0x7ffffffeLL};
  const int strides[] = {0, 1, 2, 4, 16, 1 << 20, imax};
  for (int64_t nd : nds) {
    for (int st : strides) {
      for (int64_t row : {(int64_t)0, (int64_t)1, nd / 4, nd - 1, nd, 2 * nd + 3, (int64_t)0x7ffffffeLL}) {
        const int64_t c = fwav_debug_seed_centre(row, st, nd);
        const long double want = (long double)row * st;
        const int64_t w = want < (long double)nd ? (int64_t)want : nd - 1;
        CHECK(c == w && c >= 0 && c < nd, "centre(%lld, %d, %lld) = %lld, want %lld", (long long)row, st, (long long)nd,
              (long long)c, (long long)w);
        ++centres;
      }
    }
  }
  CHECK(fwav_debug_seed_centre(-1, 1, 10) == -1 && fwav_debug_seed_centre(1, -1, 10) == -1 &&
            fwav_debug_seed_centre(1, 1, 0) == -1, "centre: bad arguments");

  // ---- the plan and the workspace with more query rows than domains (275 ranges of 77 domains, and larger)
  long plans = 0;
  const int64_t shapes[][2] = {{77, 275}, {40, 33}, {257, 2100}, {2049, 2100}, {60000, 2100}, {21027, 330750},
                               {1321977, 2700000}};
  for (auto& sh : shapes) {
    const int64_t nd = sh[0], q = sh[1];
    for (int geo = -1; geo <= 3; ++geo) {
      for (int sets : {-1, 2, 4}) {
        CHECK(fwav_debug_topk_geometry(geo) == FWAV_OK && fwav_debug_topk_cent_sets(sets) == FWAV_OK, "knobs");
        int32_t info[3] = {-9, -9, -9};
        int64_t blocks[3] = {-9, -9, -9};
        CHECK(fwav_debug_topk_plan_info(q, nd, info, blocks) == FWAV_OK, "plan_info");
        const int g = info[0], P = info[2] < 0 ? -1 : info[2];
        std::vector<int32_t> count((size_t)q, 0);
        int64_t items = -1;
        CHECK(fwav_debug_topk_plan_cover(q, (int)blocks[1], P, g, count.data(), &items) == FWAV_OK, "plan_cover");
        int64_t bad = 0;
        for (int64_t i = 0; i < q; ++i) bad += (count[i] == 1 || (P > 1 && count[i] == P)) ? 0 : 1;
        CHECK(bad == 0 && items == blocks[2], "nd=%lld q=%lld geo=%d: %lld queries covered wrongly", (long long)nd,
              (long long)q, g, (long long)bad);
        const size_t ws = fwav_sim_topk_workspace_size(q, nd, 64);
        CHECK(ws >= (size_t)items * (size_t)fwav_debug_topk_qb(g) * 256 * 8, "workspace %zu", ws);
        // a workspace one byte short is refused by both entry points before any device work
        CHECK(fwav_sim_topk_q(fp, p, nd, fp, p, q, 4, ip, ip, q, 0, 64, 1, ip, ip, p, ws - 1, nullptr) ==
                  FWAV_ERR_WORKSPACE, "sim_topk_q workspace");
        CHECK(fwav_debug_sim_topk_q(fp, p, nd, fp, p, q, 4, ip, ip, q, 0, 64, ip, p, ws - 1, 0, nullptr, nullptr) ==
                  FWAV_ERR_WORKSPACE, "debug_sim_topk_q workspace");
        ++plans;
      }
    }
  }
  CHECK(fwav_debug_topk_geometry(-1) == FWAV_OK && fwav_debug_topk_cent_sets(-1) == FWAV_OK, "reset");

  // ---- argument checks: rejected before any HIP call, with a message
  const size_t ws = fwav_sim_topk_workspace_size(10, 1000, 64);
  auto topk = [&](const float* emb, const void* e16, int64_t nd, const float* qe, const void* q16, int64_t nq, int st,
                  const int32_t* act, int64_t mq, int64_t off, int K, int thr, size_t bytes) {
    return fwav_sim_topk_q(emb, e16, nd, qe, q16, nq, st, act, ip, mq, off, K, thr, ip, nullptr, p, bytes, nullptr);
  };
  CHECK(topk(nullptr, p, 1000, fp, p, 2000, 4, ip, 10, 0, 64, 1, ws) == FWAV_ERR_ARG, "null emb");
  CHECK(topk(fp, p, 1000, nullptr, p, 2000, 4, ip, 10, 0, 64, 1, ws) == FWAV_ERR_ARG, "null qemb");
  CHECK(topk(fp, p, 1000, fp, nullptr, 2000, 4, ip, 10, 0, 64, 1, ws) == FWAV_ERR_ARG, "emb16 without qemb16");
  CHECK(topk(fp, nullptr, 1000, fp, p, 2000, 4, ip, 10, 0, 64, 1, ws) == FWAV_ERR_ARG, "qemb16 without emb16");
  CHECK(topk(fp, p, 1000, fp, p, 2000, 4, nullptr, 10, 0, 64, 1, ws) == FWAV_ERR_ARG, "null active");
  CHECK(topk(fp, p, 0, fp, p, 2000, 4, ip, 10, 0, 64, 1, ws) == FWAV_ERR_ARG, "no domains");
  CHECK(topk(fp, p, 1000, fp, p, 2000, 4, ip, -1, 0, 64, 1, ws) == FWAV_ERR_ARG, "negative max_q");
  CHECK(topk(fp, p, 1000, fp, p, 2000, -1, ip, 10, 0, 64, 1, ws) == FWAV_ERR_ARG, "negative stride");
  CHECK(topk(fp, p, 1000, fp, p, 2000, 4, ip, 10, 0, 64, 0, ws) == FWAV_ERR_ARG, "threads");
  CHECK(topk(fp, p, 1000, fp, p, 0, 4, ip, 10, 0, 64, 1, ws) == FWAV_ERR_SHAPE, "no query rows");
  CHECK(topk(fp, p, 1000, fp, p, 2000, 4, ip, 10, 2000, 64, 1, ws) == FWAV_ERR_SHAPE, "offset past the query rows");
  CHECK(topk(fp, p, 1000, fp, p, 2000, 4, ip, 10, -1, 64, 1, ws) == FWAV_ERR_SHAPE, "negative offset");
  CHECK(topk(fp, p, 1000, fp, p, (int64_t)1 << 31, 4, ip, 10, 0, 64, 1, ws) == FWAV_ERR_SHAPE, "query rows past int32");
  CHECK(topk(fp, p, (int64_t)1 << 31, fp, p, 2000, 4, ip, 10, 0, 64, 1, ws) == FWAV_ERR_SHAPE, "domains past int32");
  CHECK(topk(fp, p, 1000, fp, p, 2000, 4, ip, 10, 0, 65, 1, ws) == FWAV_ERR_K, "K > 64");
  CHECK(topk(fp, p, 1000, fp, p, 2000, 4, ip, 10, 0, 0, 1, ws) == FWAV_ERR_K, "K = 0");
  CHECK(topk(fp, p, 1000, fp, p, 2000, imax, ip, 10, 1999, 64, 1, ws - 1) == FWAV_ERR_WORKSPACE, "largest stride");
  CHECK(fwav_last_error() != nullptr && fwav_last_error()[0] != 0, "message");
  CHECK(fwav_embed_rows(nullptr, 10, 8, reinterpret_cast<const double*>(p), wp, nullptr, nullptr) == FWAV_ERR_ARG, "rows");
  CHECK(fwav_embed_rows(fp, 10, 0, reinterpret_cast<const double*>(p), wp, nullptr, nullptr) == FWAV_ERR_ARG, "rs 0");
  CHECK(fwav_embed_rows(fp, 10, 1 << 20, reinterpret_cast<const double*>(p), wp, nullptr, nullptr) == FWAV_ERR_SHAPE,
        "rs large");
  CHECK(fwav_embed_rows(fp, 0, 8, reinterpret_cast<const double*>(p), wp, p, nullptr) == FWAV_OK, "no rows");
  CHECK(fwav_embed_rows_exact(fp, 10, 51, reinterpret_cast<const double*>(p), wp, nullptr, nullptr) == FWAV_ERR_ARG,
        "no plan");
  CHECK(fwav_embed_rows_exact(fp, 0, 19, reinterpret_cast<const double*>(p), wp, nullptr, nullptr) == FWAV_OK, "no rows");
  CHECK(fwav_embed_rows_exact(fp, -1, 8, reinterpret_cast<const double*>(p), wp, nullptr, nullptr) == FWAV_ERR_ARG, "n");
  CHECK(fwav_prune_q(fp, 10, 95, 8, 1e-4f, 1, fp, 100, 50, 64, nullptr, ip, ip, ip, nullptr) == FWAV_ERR_SHAPE, "prune rows");
  CHECK(fwav_prune_q(fp, 10, 0, 8, 1e-4f, 1, nullptr, 100, 50, 64, nullptr, ip, ip, ip, nullptr) == FWAV_ERR_ARG, "prune q");
  CHECK(fwav_prune_q(fp, 10, 0, 8, 1e-4f, 1, fp, 100, 0, 64, nullptr, ip, ip, ip, nullptr) == FWAV_ERR_ARG, "prune nd");
  CHECK(fwav_prune(fp, 10, 95, 8, 1e-4f, 1, fp, 100, 64, nullptr, ip, ip, ip, nullptr) == FWAV_ERR_SHAPE, "plain prune");
  CHECK(fwav_score_rows_q(fp, 100, nullptr, ip, 1, 0, 1, wp, nullptr) == FWAV_ERR_ARG, "score rows q");
  CHECK(fwav_score_rows_q(fp, 100, fp, ip, 1, -1, 1, wp, nullptr) == FWAV_ERR_ARG, "score rows offset");
  CHECK(fwav_score_rows_q(fp, 100, fp, ip, 0, 0, 1, wp, nullptr) == FWAV_OK, "score rows none");
  CHECK(fwav_tie_check_q(fp, 10, 8, ip, 64, fp, 100, fp, nullptr, 0, 1, ip, 10, 0, ip, nullptr) == FWAV_ERR_ARG, "tie q");
  CHECK(fwav_tie_check_q(fp, 10, 8, ip, 64, fp, 100, fp, fp, -1, 1, ip, 10, 0, ip, nullptr) == FWAV_ERR_ARG, "tie offset");
  std::printf("query_check: %ld seed centres, %ld plans with more queries than domains, %d failures\n", centres, plans,
              g_fail);
  return g_fail == 0 ? 0 : 1;
}
