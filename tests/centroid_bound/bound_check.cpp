// Host driver of csrc/fwav_centroid_bound.h for tests/test_centroid_bound.py: the functions the kernel calls, on
// centroids and members given on stdin.
//   input : per case  "nm  c[16]  q_0[16] … q_{nm−1}[16]  nt  t_0 … t_{nt−1}"  (hex floats; head h = values 8h … 8h+7)
//   output: per case and t one line "tight old" (%a): cent_threshold with the score-dependent bound, and without.
#include <cstdio>
#include <vector>

#include "fwav_centroid_bound.h"

static bool read16(float (&v)[2][8]) {
  for (int h = 0; h < 2; ++h)
    for (int i = 0; i < 8; ++i)
      if (std::scanf("%a", &v[h][i]) != 1) return false;
  return true;
}

int main() {
  int nm;
  while (std::scanf("%d", &nm) == 1) {
    float c[2][8];
    if (nm < 0 || nm > 64 || !read16(c)) return 2;
    fwav::CentHead head[2];
    for (int h = 0; h < 2; ++h) fwav::cent_head_begin(head[h], c[h]);
    for (int m = 0; m < nm; ++m) {
      float q[2][8];
      if (!read16(q)) return 2;
      for (int h = 0; h < 2; ++h) fwav::cent_head_member(head[h], c[h], q[h]);
    }
    const fwav::CentBound b = fwav::cent_bound(head[0], head[1]);
    const fwav::CentBound b2 = fwav::cent_bound(head[1], head[0]);  // the other lane of the column
    if (b.slack != b2.slack || b.gd != b2.gd || b.k0 != b2.k0 || b.k2 != b2.k2) return 3;
    int nt;
    if (std::scanf("%d", &nt) != 1 || nt < 0 || nt > 4096) return 2;
    for (int i = 0; i < nt; ++i) {
      float t;
      if (std::scanf("%a", &t) != 1) return 2;
      std::printf("%a %a\n", (double)fwav::cent_threshold(b, t, true), (double)fwav::cent_threshold(b, t, false));
    }
  }
  return 0;
}
