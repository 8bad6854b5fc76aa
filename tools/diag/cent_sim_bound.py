"""Centroid pre-filter model with the score-dependent bound (csrc/fwav_centroid_bound.h, in numpy): level-2 (tile,
set) pairs per query set of 32 with one centroid per g = 2 and g = 4 consecutive queries, on the real cfg2 embedding
table (tools/diag/cent_emb_cfg2.py writes it to /tmp/cfg2_emb.npy with the oracle).  16 query sets sampled with a
fixed seed; every limit starts at max(own-window seed, floor) and rises at window ends to the exact K-th score so far
minus the band width, as tools/diag/cent_sim.py does.  CPU only.
usage: python tools/diag/cent_sim_bound.py [floor=1.85] [sets=16]"""
import sys

import numpy as np

E = np.load('/tmp/cfg2_emb.npy')
nd, nq, K = len(E), 330750, 64
D16 = 2e-3
CD, ETA = np.float32(1 + 2.0 ** -9), np.float32(1e-5)
floor = float(sys.argv[1]) if len(sys.argv) > 1 else 1.85
nsamp = int(sys.argv[2]) if len(sys.argv) > 2 else 16
E16 = E.astype(np.float16).astype(np.float32)  # what the MFMA scores


def bound_consts(Qh, g):
    """Per centroid of g consecutive rows of Qh (fp16 values as f32): c, slack, gd, k0, k2 (cent_bound)."""
    M = Qh.reshape(-1, g, 2, 8)
    c = M.mean(1).astype(np.float16).astype(np.float32)  # [n, 2, 8]
    e = M - c[:, None]
    n2 = (c * c).sum(2)  # [n, 2]
    e2 = (e * e).sum(3)  # [n, g, 2]
    ec = (e * c[:, None]).sum(3)
    en = np.sqrt(e2)
    with np.errstate(divide='ignore', invalid='ignore'):
        b2 = np.where(n2[:, None] > 0, np.minimum(ec * ec / n2[:, None], e2), 0.0)
    beta = np.where(n2[:, None] > 0, np.sqrt(b2) + 2.0 ** -20 * en, 0.0).max(1)
    perp2 = ((e2 - b2) + 2.0 ** -18 * e2).max(1)
    rho = en.max(1)
    slack = rho.sum(1) * CD + ETA
    N2 = n2.sum(1) * (1 - 2.0 ** -20)
    s2 = perp2.sum(1) * (1 + 2.0 ** -20)
    gd = beta.sum(1) * CD + ETA
    return c.reshape(-1, 16), slack, gd, 2 * s2 * CD * CD, s2 / N2


def threshold(tmin, slack, gd, k0, k2, tight):
    old = tmin - slack
    t = tmin - gd
    A = 1 + k2
    rad = np.maximum(k0 * A * (1 + 2.0 ** -12) - k2 * t * t, 0)
    s = (t - np.sqrt(rad)) / A
    ok = tight & (t > 0) & np.isfinite(t) & (s > 0)
    return np.where(ok, np.maximum(old, s), old)


def sim(q0, g, win=128, warm=32):
    Q = E16[q0:q0 + 32]
    c, slack, gd, k0, k2 = bound_consts(Q, g)
    th = np.empty(32, np.float32)
    for i in range(32):
        w = E16[max(0, q0 + i - 64):q0 + i + 64] @ Q[i]
        th[i] = max(np.sort(w)[-K] - 2 * D16, floor)
    pairs = {True: 0, False: 0}
    fires = 0
    top = None
    nch = -(-nd // 256)
    chunk = 0
    while chunk < nch:
        c1 = min(nch, chunk + (4 if chunk < warm else win))
        blk = E16[chunk * 256:c1 * 256]
        S, Sc = blk @ Q.T, blk @ c.T
        nt = -(-len(blk) // 32)
        pad = nt * 32 - len(blk)
        if pad:
            S = np.vstack([S, np.full((pad, 32), -9, np.float32)])
            Sc = np.vstack([Sc, np.full((pad, len(c)), -9, np.float32)])
        tcm = Sc.reshape(nt, 32, -1).max(1)
        tmin = th.reshape(-1, g).min(1)
        for tight in (True, False):
            pairs[tight] += int((tcm > threshold(tmin, slack, gd, k0, k2, tight)[None]).any(1).sum())
        fires += int((S.reshape(nt, 32, 32).max(1) > th[None]).any(1).sum())
        allv = S[:len(blk)] if top is None else np.vstack([top, S[:len(blk)]])
        top = -np.partition(-allv, K - 1, axis=0)[:K]
        th = np.maximum(th, top[K - 1] - 2 * D16)
        chunk = c1
    return pairs[True], pairs[False], fires, nch * 8


rng = np.random.default_rng(7)
starts = np.sort(rng.integers(0, nq // 32, nsamp)) * 32
tot = {2: [0, 0, 0], 4: [0, 0, 0]}
for q0 in starts:
    for g in (2, 4):
        a, b, f, nt = sim(int(q0), g)
        tot[g][0] += a
        tot[g][1] += b
        tot[g][2] += f
        print(f"set at query {q0} g {g}: level-2 pairs {a} (worst-case slack {b}) of {nt} tiles, firing tiles {f}",
              flush=True)
for g in (2, 4):
    print(f"g {g}: level-2 pairs per query set {tot[g][0] / nsamp:.0f} (worst-case slack {tot[g][1] / nsamp:.0f}), "
          f"firing tiles {tot[g][2] / nsamp:.0f}; floor {floor}")
print(f"g 4 / g 2 pairs: {tot[4][0] / max(tot[2][0], 1):.2f}")
