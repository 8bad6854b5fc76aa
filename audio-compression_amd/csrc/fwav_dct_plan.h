// fwav_dct_plan.h — scipy.fftpack.dct(x, type=2, norm='ortho') for a runtime length n, bit-exact in float32 and float64.
//
// fwav_dct.h fixes three plans at compile time (n = 4, 8, 16).  This header runs pocketfft's general real-FFT plan
// (rfftp) inside the same T_dcst23 wrapper: the backward passes in factor order (radb4, radb2, radb3, radb5 and the
// generic odd-prime pass radbg, with runtime ido / l1), ping-ponging between two buffers, copy_and_norm by
// fct = 1/sqrt(2n), then the twiddle post-pass.  Each product and sum is rounded separately in T
// (-ffp-contract=off), in pocketfft's own order, so the results are scipy's bit for bit wherever pocketfft itself
// takes rfftp and not Bluestein: every n < 50, and above that every n whose largest prime factor squared is ≤ n
// (dct_plan_supported in fwav_pool_embed.hip; the range here is 4 … 64).
//
// The plan (factors, twiddle offsets) and every constant come from the host (dct_plan_build / dct_plan_constants in
// fwav_pool_embed.hip, pocketfft's factorize + comp_twiddle); this header only walks them.  The two work buffers are
// reached through a strided column view, so the device keeps them column-interleaved in LDS (element i of lane t at
// i·S + t: a wave's accesses are conflict-free) while the host instantiation (fwav_debug_dct2_plan) uses stride 1.
// Pinned: tests/test_exact_dct.py against scipy for every supported n, both precisions.
#pragma once

#include "fwav_dct.h"

namespace fwav {

constexpr int kPlanMaxN = 64;
constexpr int kPlanMaxFact = 4;  // 54 = 2·3·3·3 is the longest factor list up to 64
// Table layout (doubles): head [0] n, [1] number of factors, [2 + 3k ..] = factor k's (ip, twiddle offset, extra
// table offset; offsets into a precision block's `mem`), [14] doubles per precision block; [16 .. 16 + n) w =
// np.linspace(1, 2, n); then the float32 block and the float64 block (values rounded to that precision).
constexpr int kPlanHead = 16;
// Precision block: [0] fct, [1] sqrt2, [2] taui (radb3), [3 .. 6] tr11, ti11, tr12, ti12 (radb5), [7] unused;
// [8 .. 8 + n) T_dcst23's twiddles; [8 + n ..) rfftp's twiddle memory (comp_twiddle order).
constexpr int kPlanConst = 8;
// The longest rfftp twiddle memory up to n = 64 is 94 values (n = 47: the generic pass's 2·ip table); 2n + 16 bounds
// every supported n (checked by dct_plan_build).
constexpr int plan_block_max(int nmax) { return kPlanConst + nmax + 2 * nmax + 16; }

// Element i of one column of a buffer whose columns are interleaved with stride S.
template <class T, int S>
struct Col {
  T* p;
  FWAV_HD T& operator[](int i) const { return p[i * S]; }
};

template <class T>
struct PlanK {
  int n, nf;
  int ip[kPlanMaxFact], tw[kPlanMaxFact], tws[kPlanMaxFact];
  const T* k;  // one precision block
};

// arr[k] for a run-time k without a run-time-indexed array (which the device would keep in scratch memory).
FWAV_HD int plan_pick(const int (&arr)[kPlanMaxFact], int k) {
  static_assert(kPlanMaxFact == 4, "plan_pick selects among four factors");
  return k == 0 ? arr[0] : k == 1 ? arr[1] : k == 2 ? arr[2] : arr[3];
}

// pocketfft rfftp::radb4 with runtime ido / l1 (the operation order of fwav_dct.h's radb4).
template <class T, class V>
FWAV_HD void radb4_rt(int ido, int l1, V cc, V ch, const T* wa, T sqrt2) {
  auto CC = [&](int a, int b, int c) -> T { return cc[a + ido * (b + 4 * c)]; };
  auto CH = [&](int a, int b, int c) -> T& { return ch[a + ido * (b + l1 * c)]; };
  auto WA = [&](int x, int i) -> T { return wa[i + x * (ido - 1)]; };
  for (int k = 0; k < l1; ++k) {
    T tr1, tr2;
    pm(tr2, tr1, CC(0, 0, k), CC(ido - 1, 3, k));
    const T tr3 = (T)2 * CC(ido - 1, 1, k);
    const T tr4 = (T)2 * CC(0, 2, k);
    pm(CH(0, k, 0), CH(0, k, 2), tr2, tr3);
    pm(CH(0, k, 3), CH(0, k, 1), tr1, tr4);
  }
  if ((ido & 1) == 0) {
    for (int k = 0; k < l1; ++k) {
      T tr1, tr2, ti1, ti2;
      pm(ti1, ti2, CC(0, 3, k), CC(0, 1, k));
      pm(tr2, tr1, CC(ido - 1, 0, k), CC(ido - 1, 2, k));
      CH(ido - 1, k, 0) = tr2 + tr2;
      CH(ido - 1, k, 1) = sqrt2 * (tr1 - ti1);
      CH(ido - 1, k, 2) = ti2 + ti2;
      CH(ido - 1, k, 3) = -sqrt2 * (tr1 + ti1);
    }
  }
  if (ido <= 2) return;
  for (int k = 0; k < l1; ++k) {
    for (int i = 2; i < ido; i += 2) {
      const int ic = ido - i;
      T ci2, ci3, ci4, cr2, cr3, cr4, ti1, ti2, ti3, ti4, tr1, tr2, tr3, tr4;
      pm(tr2, tr1, CC(i - 1, 0, k), CC(ic - 1, 3, k));
      pm(ti1, ti2, CC(i, 0, k), CC(ic, 3, k));
      pm(tr4, ti3, CC(i, 2, k), CC(ic, 1, k));
      pm(tr3, ti4, CC(i - 1, 2, k), CC(ic - 1, 1, k));
      pm(CH(i - 1, k, 0), cr3, tr2, tr3);
      pm(CH(i, k, 0), ci3, ti2, ti3);
      pm(cr4, cr2, tr1, tr4);
      pm(ci2, ci4, ti1, ti4);
      // MULPM(a, b, c, d, e, f): a = c·e + d·f, b = c·f − d·e
      CH(i, k, 1) = WA(0, i - 2) * ci2 + WA(0, i - 1) * cr2;
      CH(i - 1, k, 1) = WA(0, i - 2) * cr2 - WA(0, i - 1) * ci2;
      CH(i, k, 2) = WA(1, i - 2) * ci3 + WA(1, i - 1) * cr3;
      CH(i - 1, k, 2) = WA(1, i - 2) * cr3 - WA(1, i - 1) * ci3;
      CH(i, k, 3) = WA(2, i - 2) * ci4 + WA(2, i - 1) * cr4;
      CH(i - 1, k, 3) = WA(2, i - 2) * cr4 - WA(2, i - 1) * ci4;
    }
  }
}

// pocketfft rfftp::radb2.
template <class T, class V>
FWAV_HD void radb2_rt(int ido, int l1, V cc, V ch, const T* wa) {
  auto CC = [&](int a, int b, int c) -> T { return cc[a + ido * (b + 2 * c)]; };
  auto CH = [&](int a, int b, int c) -> T& { return ch[a + ido * (b + l1 * c)]; };
  auto WA = [&](int x, int i) -> T { return wa[i + x * (ido - 1)]; };
  for (int k = 0; k < l1; ++k) pm(CH(0, k, 0), CH(0, k, 1), CC(0, 0, k), CC(ido - 1, 1, k));
  if ((ido & 1) == 0) {
    for (int k = 0; k < l1; ++k) {
      CH(ido - 1, k, 0) = (T)2 * CC(ido - 1, 0, k);
      CH(ido - 1, k, 1) = (T)-2 * CC(0, 1, k);
    }
  }
  if (ido <= 2) return;
  for (int k = 0; k < l1; ++k) {
    for (int i = 2; i < ido; i += 2) {
      const int ic = ido - i;
      T ti2, tr2;
      pm(CH(i - 1, k, 0), tr2, CC(i - 1, 0, k), CC(ic - 1, 1, k));
      pm(ti2, CH(i, k, 0), CC(i, 0, k), CC(ic, 1, k));
      CH(i, k, 1) = WA(0, i - 2) * ti2 + WA(0, i - 1) * tr2;
      CH(i - 1, k, 1) = WA(0, i - 2) * tr2 - WA(0, i - 1) * ti2;
    }
  }
}

// pocketfft rfftp::radb3.  taur = −1/2; taui = sqrt(3)/2 rounded to T (K[2]).
template <class T, class V>
FWAV_HD void radb3_rt(int ido, int l1, V cc, V ch, const T* wa, const T* K) {
  const T taur = (T)-0.5, taui = K[2];
  auto CC = [&](int a, int b, int c) -> T { return cc[a + ido * (b + 3 * c)]; };
  auto CH = [&](int a, int b, int c) -> T& { return ch[a + ido * (b + l1 * c)]; };
  auto WA = [&](int x, int i) -> T { return wa[i + x * (ido - 1)]; };
  for (int k = 0; k < l1; ++k) {
    const T tr2 = (T)2 * CC(ido - 1, 1, k);
    const T cr2 = CC(0, 0, k) + taur * tr2;
    CH(0, k, 0) = CC(0, 0, k) + tr2;
    const T ci3 = ((T)2 * taui) * CC(0, 2, k);
    pm(CH(0, k, 2), CH(0, k, 1), cr2, ci3);
  }
  if (ido == 1) return;
  for (int k = 0; k < l1; ++k) {
    for (int i = 2, ic = ido - 2; i < ido; i += 2, ic -= 2) {
      const T tr2 = CC(i - 1, 2, k) + CC(ic - 1, 1, k);
      const T ti2 = CC(i, 2, k) - CC(ic, 1, k);
      const T cr2 = CC(i - 1, 0, k) + taur * tr2;
      const T ci2 = CC(i, 0, k) + taur * ti2;
      CH(i - 1, k, 0) = CC(i - 1, 0, k) + tr2;
      CH(i, k, 0) = CC(i, 0, k) + ti2;
      const T cr3 = taui * (CC(i - 1, 2, k) - CC(ic - 1, 1, k));
      const T ci3 = taui * (CC(i, 2, k) + CC(ic, 1, k));
      T di2, di3, dr2, dr3;
      pm(dr3, dr2, cr2, ci3);
      pm(di2, di3, ci2, cr3);
      CH(i, k, 1) = WA(0, i - 2) * di2 + WA(0, i - 1) * dr2;
      CH(i - 1, k, 1) = WA(0, i - 2) * dr2 - WA(0, i - 1) * di2;
      CH(i, k, 2) = WA(1, i - 2) * di3 + WA(1, i - 1) * dr3;
      CH(i - 1, k, 2) = WA(1, i - 2) * dr3 - WA(1, i - 1) * di3;
    }
  }
}

// pocketfft rfftp::radb5.  K[3 .. 6] = cos(2π/5), sin(2π/5), cos(4π/5), sin(4π/5) rounded to T.
template <class T, class V>
FWAV_HD void radb5_rt(int ido, int l1, V cc, V ch, const T* wa, const T* K) {
  const T tr11 = K[3], ti11 = K[4], tr12 = K[5], ti12 = K[6];
  auto CC = [&](int a, int b, int c) -> T { return cc[a + ido * (b + 5 * c)]; };
  auto CH = [&](int a, int b, int c) -> T& { return ch[a + ido * (b + l1 * c)]; };
  auto WA = [&](int x, int i) -> T { return wa[i + x * (ido - 1)]; };
  for (int k = 0; k < l1; ++k) {
    const T ti5 = CC(0, 2, k) + CC(0, 2, k);
    const T ti4 = CC(0, 4, k) + CC(0, 4, k);
    const T tr2 = CC(ido - 1, 1, k) + CC(ido - 1, 1, k);
    const T tr3 = CC(ido - 1, 3, k) + CC(ido - 1, 3, k);
    CH(0, k, 0) = CC(0, 0, k) + tr2 + tr3;
    const T cr2 = CC(0, 0, k) + tr11 * tr2 + tr12 * tr3;
    const T cr3 = CC(0, 0, k) + tr12 * tr2 + tr11 * tr3;
    const T ci5 = ti5 * ti11 + ti4 * ti12;
    const T ci4 = ti5 * ti12 - ti4 * ti11;
    pm(CH(0, k, 4), CH(0, k, 1), cr2, ci5);
    pm(CH(0, k, 3), CH(0, k, 2), cr3, ci4);
  }
  if (ido == 1) return;
  for (int k = 0; k < l1; ++k) {
    for (int i = 2, ic = ido - 2; i < ido; i += 2, ic -= 2) {
      T tr2, tr3, tr4, tr5, ti2, ti3, ti4, ti5;
      pm(tr2, tr5, CC(i - 1, 2, k), CC(ic - 1, 1, k));
      pm(ti5, ti2, CC(i, 2, k), CC(ic, 1, k));
      pm(tr3, tr4, CC(i - 1, 4, k), CC(ic - 1, 3, k));
      pm(ti4, ti3, CC(i, 4, k), CC(ic, 3, k));
      CH(i - 1, k, 0) = CC(i - 1, 0, k) + tr2 + tr3;
      CH(i, k, 0) = CC(i, 0, k) + ti2 + ti3;
      const T cr2 = CC(i - 1, 0, k) + tr11 * tr2 + tr12 * tr3;
      const T ci2 = CC(i, 0, k) + tr11 * ti2 + tr12 * ti3;
      const T cr3 = CC(i - 1, 0, k) + tr12 * tr2 + tr11 * tr3;
      const T ci3 = CC(i, 0, k) + tr12 * ti2 + tr11 * ti3;
      const T cr5 = tr5 * ti11 + tr4 * ti12;
      const T cr4 = tr5 * ti12 - tr4 * ti11;
      const T ci5 = ti5 * ti11 + ti4 * ti12;
      const T ci4 = ti5 * ti12 - ti4 * ti11;
      T dr2, dr3, dr4, dr5, di2, di3, di4, di5;
      pm(dr4, dr3, cr3, ci4);
      pm(di3, di4, ci3, cr4);
      pm(dr5, dr2, cr2, ci5);
      pm(di2, di5, ci2, cr5);
      CH(i, k, 1) = WA(0, i - 2) * di2 + WA(0, i - 1) * dr2;
      CH(i - 1, k, 1) = WA(0, i - 2) * dr2 - WA(0, i - 1) * di2;
      CH(i, k, 2) = WA(1, i - 2) * di3 + WA(1, i - 1) * dr3;
      CH(i - 1, k, 2) = WA(1, i - 2) * dr3 - WA(1, i - 1) * di3;
      CH(i, k, 3) = WA(2, i - 2) * di4 + WA(2, i - 1) * dr4;
      CH(i - 1, k, 3) = WA(2, i - 2) * dr4 - WA(2, i - 1) * di4;
      CH(i, k, 4) = WA(3, i - 2) * di5 + WA(3, i - 1) * dr5;
      CH(i - 1, k, 4) = WA(3, i - 2) * dr5 - WA(3, i - 1) * di5;
    }
  }
}

// pocketfft rfftp::radbg, the generic backward pass for an odd prime factor ip > 5.  cs: the 2·ip "extra" table
// (cos, sin of 2πj/ip).  The pass uses cc as scratch; the result is in ch.
template <class T, class V>
FWAV_HD void radbg_rt(int ido, int ip, int l1, V cc, V ch, const T* wa, const T* cs) {
  const int ipph = (ip + 1) / 2;
  const int idl1 = ido * l1;
  auto CC = [&](int a, int b, int c) -> T { return cc[a + ido * (b + ip * c)]; };
  auto CH = [&](int a, int b, int c) -> T& { return ch[a + ido * (b + l1 * c)]; };
  auto C1 = [&](int a, int b, int c) -> T { return cc[a + ido * (b + l1 * c)]; };
  auto C2 = [&](int a, int b) -> T& { return cc[a + idl1 * b]; };
  auto CH2 = [&](int a, int b) -> T& { return ch[a + idl1 * b]; };
  for (int k = 0; k < l1; ++k)
    for (int i = 0; i < ido; ++i) CH(i, k, 0) = CC(i, 0, k);
  for (int j = 1, jc = ip - 1; j < ipph; ++j, --jc) {
    const int j2 = 2 * j - 1;
    for (int k = 0; k < l1; ++k) {
      CH(0, k, j) = (T)2 * CC(ido - 1, j2, k);
      CH(0, k, jc) = (T)2 * CC(0, j2 + 1, k);
    }
  }
  if (ido != 1) {
    for (int j = 1, jc = ip - 1; j < ipph; ++j, --jc) {
      const int j2 = 2 * j - 1;
      for (int k = 0; k < l1; ++k) {
        for (int i = 1, ic = ido - i - 2; i <= ido - 2; i += 2, ic -= 2) {
          CH(i, k, j) = CC(i, j2 + 1, k) + CC(ic, j2, k);
          CH(i, k, jc) = CC(i, j2 + 1, k) - CC(ic, j2, k);
          CH(i + 1, k, j) = CC(i + 1, j2 + 1, k) - CC(ic + 1, j2, k);
          CH(i + 1, k, jc) = CC(i + 1, j2 + 1, k) + CC(ic + 1, j2, k);
        }
      }
    }
  }
  for (int l = 1, lc = ip - 1; l < ipph; ++l, --lc) {
    for (int ik = 0; ik < idl1; ++ik) {
      C2(ik, l) = CH2(ik, 0) + cs[2 * l] * CH2(ik, 1) + cs[4 * l] * CH2(ik, 2);
      C2(ik, lc) = cs[2 * l + 1] * CH2(ik, ip - 1) + cs[4 * l + 1] * CH2(ik, ip - 2);
    }
    int iang = 2 * l;
    int j = 3, jc = ip - 3;
    auto next = [&]() {
      iang += l;
      if (iang > ip) iang -= ip;
    };
    for (; j < ipph - 3; j += 4, jc -= 4) {
      next();
      const T ar1 = cs[2 * iang], ai1 = cs[2 * iang + 1];
      next();
      const T ar2 = cs[2 * iang], ai2 = cs[2 * iang + 1];
      next();
      const T ar3 = cs[2 * iang], ai3 = cs[2 * iang + 1];
      next();
      const T ar4 = cs[2 * iang], ai4 = cs[2 * iang + 1];
      for (int ik = 0; ik < idl1; ++ik) {
        C2(ik, l) += ar1 * CH2(ik, j) + ar2 * CH2(ik, j + 1) + ar3 * CH2(ik, j + 2) + ar4 * CH2(ik, j + 3);
        C2(ik, lc) += ai1 * CH2(ik, jc) + ai2 * CH2(ik, jc - 1) + ai3 * CH2(ik, jc - 2) + ai4 * CH2(ik, jc - 3);
      }
    }
    for (; j < ipph - 1; j += 2, jc -= 2) {
      next();
      const T ar1 = cs[2 * iang], ai1 = cs[2 * iang + 1];
      next();
      const T ar2 = cs[2 * iang], ai2 = cs[2 * iang + 1];
      for (int ik = 0; ik < idl1; ++ik) {
        C2(ik, l) += ar1 * CH2(ik, j) + ar2 * CH2(ik, j + 1);
        C2(ik, lc) += ai1 * CH2(ik, jc) + ai2 * CH2(ik, jc - 1);
      }
    }
    for (; j < ipph; ++j, --jc) {
      next();
      const T war = cs[2 * iang], wai = cs[2 * iang + 1];
      for (int ik = 0; ik < idl1; ++ik) {
        C2(ik, l) += war * CH2(ik, j);
        C2(ik, lc) += wai * CH2(ik, jc);
      }
    }
  }
  for (int j = 1; j < ipph; ++j)
    for (int ik = 0; ik < idl1; ++ik) CH2(ik, 0) += CH2(ik, j);
  for (int j = 1, jc = ip - 1; j < ipph; ++j, --jc) {
    for (int k = 0; k < l1; ++k) {
      CH(0, k, j) = C1(0, k, j) - C1(0, k, jc);
      CH(0, k, jc) = C1(0, k, j) + C1(0, k, jc);
    }
  }
  if (ido == 1) return;
  for (int j = 1, jc = ip - 1; j < ipph; ++j, --jc) {
    for (int k = 0; k < l1; ++k) {
      for (int i = 1; i <= ido - 2; i += 2) {
        CH(i, k, j) = C1(i, k, j) - C1(i + 1, k, jc);
        CH(i, k, jc) = C1(i, k, j) + C1(i + 1, k, jc);
        CH(i + 1, k, j) = C1(i + 1, k, j) + C1(i, k, jc);
        CH(i + 1, k, jc) = C1(i + 1, k, j) - C1(i, k, jc);
      }
    }
  }
  for (int j = 1; j < ip; ++j) {
    const int is = (j - 1) * (ido - 1);
    for (int k = 0; k < l1; ++k) {
      int idij = is;
      for (int i = 1; i <= ido - 2; i += 2) {
        const T t1 = CH(i, k, j), t2 = CH(i + 1, k, j);
        CH(i, k, j) = wa[idij] * t1 - wa[idij + 1] * t2;
        CH(i + 1, k, j) = wa[idij] * t2 + wa[idij + 1] * t1;
        idij += 2;
      }
    }
  }
}

// T_dcst23::exec(c, fct, ortho = true, type = 2, cosine = true) for the plan P: scipy.fftpack.dct(c, norm='ortho') in
// place in c; ch is the second work buffer (n elements, contents irrelevant).
template <class T, class V>
FWAV_HD void dct2_ortho_plan(V c, V ch, const PlanK<T>& P) {
  const int N = P.n;
  const int NS2 = (N + 1) / 2;
  const T* K = P.k;
  const T* tw = K + kPlanConst;
  const T* mem = tw + N;
  const T fct = K[0], sqrt2 = K[1];
  c[0] *= (T)2;
  if ((N & 1) == 0) c[N - 1] *= (T)2;
  for (int i = 1; i < N - 1; i += 2) {  // MPINPLACE(c[i+1], c[i])
    const T t = c[i + 1];
    c[i + 1] -= c[i];
    c[i] += t;
  }
  // rfftp::exec(c, fct, r2hc = false)
  V p1 = c, p2 = ch;
  for (int k = 0, l1 = 1; k < P.nf; ++k) {
    const int ip = plan_pick(P.ip, k);
    const int ido = N / (ip * l1);
    const T* wa = mem + plan_pick(P.tw, k);
    if (ip == 4) radb4_rt<T>(ido, l1, p1, p2, wa, sqrt2);
    else if (ip == 2) radb2_rt<T>(ido, l1, p1, p2, wa);
    else if (ip == 3) radb3_rt<T>(ido, l1, p1, p2, wa, K);
    else if (ip == 5) radb5_rt<T>(ido, l1, p1, p2, wa, K);
    else radbg_rt<T>(ido, ip, l1, p1, p2, wa, mem + plan_pick(P.tws, k));
    const V t = p1;
    p1 = p2;
    p2 = t;
    l1 *= ip;
  }
  if (p1.p != c.p) {  // copy_and_norm
    for (int i = 0; i < N; ++i) c[i] = fct * p1[i];
  } else {
    for (int i = 0; i < N; ++i) c[i] *= fct;
  }
  for (int i = 1, ic = N - 1; i < NS2; ++i, --ic) {
    const T t1 = tw[i - 1] * c[ic] + tw[ic - 1] * c[i];
    const T t2 = tw[i - 1] * c[i] - tw[ic - 1] * c[ic];
    c[i] = (T)0.5 * (t1 + t2);
    c[ic] = (T)0.5 * (t1 - t2);
  }
  if ((N & 1) == 0) c[NS2] *= tw[NS2 - 1];
  c[0] *= sqrt2 * (T)0.5;
}

}  // namespace fwav
