"""Inputs of the decode edge tests (test helper, shared by tests/golden/make_decode_edges.py, the CPU pin of O.decode
and tests/test_gpu_decode_edges.py).

``build(rs, nr, kind)`` returns one match table of nr ranges over a pool of N_POOL tiles: first the edge rows below
(one label each in ``names``), then random rows, and in the last five rows edge rows again, so that the final, partly
filled thread group of the decode kernel holds them.  With convergence_eps = 0 a range's reconstruction depends on
nothing but its own row, so a test may decode any slice [a, b) alone and compare it with rows [a, b) of one decode of
the whole table.  The builder asserts that its edges are what they claim (on the oracle's own sums, never on a
device's output): the ``den`` pair straddles 1e-12 within a factor 2, a third tile has den exactly 1e-12 (`>` and `>=`
part only there), −0.0 is present in s, o and the pool."""
import hashlib

import numpy as np

from affine_edges import same_bits_or_nan  # noqa: F401  (bit-equal, any NaN matches any NaN, nothing else relaxed)
from oracle import fractal_oracle as O

F32 = np.float32
N_POOL = 200
N_PLAIN = 180   # pool rows [0, N_PLAIN) are plain random tiles; the special tiles follow
(P_CONST, P_HI, P_LO, P_TINY, P_PAL, P_T, P_TM, P_A, P_B, P_NZ,
 P_BIG, P_BIGC, P_INF, P_NAN, P_EQ) = range(N_PLAIN, N_PLAIN + 15)
N_TAIL = 5
DEN_THR = F32(1e-12)   # the validity threshold of the scale solve (fractal.py:1409, :1440)

KINDS = ("finite", "nonfinite", "tiny", "flush", "huge")
SCALE = {"tiny": 1e-20, "flush": 1e-30, "huge": 1e19}

# (iterations, convergence_eps, s_clip, s_damping)
PARAMS = (
    (8, 1e-3, 16.0, 0.0),
    (1, 1e-3, 16.0, 0.0),
    (2, 1e-3, 16.0, 0.5),
    (3, 1e-3, 16.0, 0.5),
    (5, 0.0, 0.5, 0.2),
    (70, 1e-5, 16.0, 0.7),
    (6, 0.0, 16.0, 1e-6),
    (4, 0.0, 16.0, 1.0),
    (4, 0.0, 16.0, 1.5),
    (3, 0.0, 0.0, 0.0),
    (3, 0.0, -16.0, 0.0),
    (3, 0.0, float("inf"), 0.0),
)
# the shapes recorded in tests/golden/decode_edges.npz: every dispatch path of fwav_decode — the runtime-sized
# resident buckets (rs 1/3/7 → <8,0,4>, 12 → <16,0,2>, 20 → <32,0,1>), the fixed ones (4, 8, 16, 32), the streaming
# kernels with one pairwise leaf (33, 40, 128) and with several (130, 300, 1024)
FIXTURE_RS = (1, 3, 4, 7, 8, 12, 16, 20, 32, 33, 40, 128, 130, 300, 1024)
FIXTURE_NR = 67
FIXTURE_SETS_ALL_KINDS = (0, 2, 4, 6, 9)   # PARAMS 1, 3, 5, 7, 10 for every kind; kind "finite" gets every set


def kw(p):
    it, eps, clip, damp = p
    return dict(iterations=it, convergence_eps=eps, s_clip=clip, s_damping=damp)


def fixture_entries():
    """[(rs, kind, index into PARAMS)] in the order of the fixture."""
    out = []
    for rs in FIXTURE_RS:
        for kind in KINDS:
            for pi in range(len(PARAMS)):
                if kind == "finite" or pi in FIXTURE_SETS_ALL_KINDS:
                    out.append((rs, kind, pi))
    return out


def den_of(tile):
    """Σ (T − mean T)² as the decoder's scale solve evaluates it (numpy's pairwise order)."""
    t = np.asarray(tile, F32)
    tc = t - O.pw_mean(t)[..., None]
    return O.pw_sum(tc * tc)


def _den_pair(rs, rng):
    """T = 0.25 + ε·noise with den just above 1e-12 and at or below it: ε by bisection, nothing hard-coded."""
    noise = rng.normal(0, 1, rs).astype(F32)

    def mk(e):
        return (F32(0.25) + F32(e) * noise).astype(F32)

    lo, hi = 0.0, 1e-3
    assert den_of(mk(lo)) <= DEN_THR < den_of(mk(hi))
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if den_of(mk(mid)) > DEN_THR:
            hi = mid
        else:
            lo = mid
    above, below = mk(hi), mk(lo)
    assert DEN_THR < den_of(above) < 2 * DEN_THR, (rs, den_of(above))
    assert DEN_THR / 2 < den_of(below) <= DEN_THR, (rs, den_of(below))
    return above, below


def _den_exact(rs):
    """A tile with den exactly 1e-12 (the float32 threshold itself: `>` and `>=` part here), or None where none is
    found: (a, −a, b, −b, 0, …) has mean exactly 0 in numpy's order, so den = a² + a² + b² + b²; a carries most of
    it and b is searched among neighbouring floats until the rounded sum is the threshold."""
    if rs < 2:
        return None
    a = F32(np.sqrt(float(DEN_THR) * (0.5 if rs < 4 else 0.375)))
    t = np.zeros((2001, rs), F32)
    if rs < 4:
        av = a.view(np.uint32) + np.arange(-1000, 1001, dtype=np.int64)
        t[:, 0] = av.astype(np.uint32).view(F32)
        t[:, 1] = -t[:, 0]
    else:
        b = F32(np.sqrt(float(DEN_THR) / 2 - float(a * a)))
        bv = b.view(np.uint32) + np.arange(-1000, 1001, dtype=np.int64)
        t[:, 0], t[:, 1] = a, -a
        t[:, 2] = bv.astype(np.uint32).view(F32)
        t[:, 3] = -t[:, 2]
    hit = np.nonzero(den_of(t) == DEN_THR)[0]
    return t[hit[len(hit) // 2]].copy() if len(hit) else None


def build(rs, nr, kind, seed=0):
    """→ (idx i32[nr], s f32[nr], o f32[nr], sym u8[nr], pool f32[N_POOL, rs], names: one label per head row)."""
    assert kind in KINDS
    rng = np.random.default_rng(1000 * rs + seed)
    pool = rng.normal(0, 0.3, (N_POOL, rs)).astype(F32)
    pool[P_CONST] = F32(0.25)                       # den = 0: not valid, the stored s is kept
    if rs >= 2:                                     # rs = 1: den is 0 whatever the tile — plain rows
        pool[P_HI], pool[P_LO] = _den_pair(rs, rng)
    eq = _den_exact(rs)                             # rs 1: den is 0 — the row is one more plain row
    pool[P_EQ] = pool[P_LO] if eq is None else eq
    assert rs < 2 or den_of(pool[P_EQ]) == DEN_THR
    pool[P_TINY] = pool[P_TINY] * F32(1e-30)        # den underflows to 0
    h = rs // 2
    pool[P_PAL, rs - h:] = pool[P_PAL, :h][::-1]    # palindrome: sym 0 and 1 give the same tile
    pool[P_TM] = pool[P_T][::-1]                    # exact mirror of P_T
    pool[P_NZ] = F32(-0.0)                          # every element −0.0
    nonfinite = kind == "nonfinite"
    if nonfinite:
        pool[0] = F32(np.nan)                       # sentinel rows must come out 0 without reading it
        pool[P_BIG] = F32(3e38) * np.where(pool[P_BIG] < 0, F32(-1), F32(1))   # sums and squares overflow
        pool[P_BIGC] = F32(3e38)
        pool[P_INF, rs // 3] = F32(np.inf)
        pool[P_NAN, rs // 2] = F32(np.nan)
    rows, names = [], []

    def row(name, i, s, o, sym):
        rows.append((i, s, o, sym))
        names.append(name)

    row("idx -1 with s, o, sym set", -1, 0.7, 0.3, 1)
    row("idx -7 with s, o, sym set", -7, -1.1, -0.2, 1)
    row("constant tile", P_CONST, 0.9, 0.1, 0)
    row("constant tile, s 40", P_CONST, 40.0, 0.1, 1)
    row("constant tile, s -40", P_CONST, -40.0, -0.1, 0)
    row("constant tile, s 1e30", P_CONST, 1e30, 0.1, 0)
    row("constant tile, s -0.0, o -0.0", P_CONST, -0.0, -0.0, 0)
    row("constant tile, s 0, o -0.0", P_CONST, 0.0, -0.0, 1)
    row("den just above 1e-12", P_HI, 3.0, 0.05, 0)
    row("den at or below 1e-12", P_LO, 3.0, 0.05, 0)
    row("den just above 1e-12, mirrored", P_HI, -3.0, 0.05, 1)
    row("den at or below 1e-12, mirrored", P_LO, -3.0, 0.05, 1)
    row("den exactly 1e-12" if eq is not None else "den below 1e-12 (rs 1: no exact tile)", P_EQ, 3.0, 0.05, 0)
    row("tiny tile", P_TINY, 0.8, 0.1, 0)
    row("tile of -0.0", P_NZ, 0.5, -0.0, 1)
    row("palindrome, sym 0", P_PAL, 0.6, 0.02, 0)
    row("palindrome, sym 1", P_PAL, 0.6, 0.02, 1)
    row("tile, sym 0", P_T, 0.4, -0.03, 0)
    row("mirror tile, sym 1", P_TM, 0.4, -0.03, 1)
    row("same domain, sym 0", P_B, -0.9, 0.07, 0)
    row("same domain, sym 1", P_B, -0.9, 0.07, 1)
    row("sym byte 2", P_T, 0.4, -0.03, 2)
    row("sym byte 255", P_T, 0.4, -0.03, 255)
    row("s 40", P_A, 40.0, 0.0, 0)
    row("s -40", P_A, -40.0, 0.2, 1)
    row("s 1e30", P_A, 1e30, 0.0, 0)
    row("s 0", P_A, 0.0, 0.1, 0)
    row("s -0.0", P_A, -0.0, 0.1, 1)
    row("s 0, o -0.0", P_A, 0.0, -0.0, 0)
    if nonfinite:
        inf, nan = float("inf"), float("nan")
        row("tile of +-3e38", P_BIG, 0.5, 0.1, 0)
        row("tile of +-3e38, mirrored", P_BIG, 0.5, 0.1, 1)
        row("tile of 3e38", P_BIGC, 0.5, 0.1, 0)
        row("tile with inf", P_INF, 0.5, 0.1, 0)
        row("tile with inf, mirrored", P_INF, 0.5, 0.1, 1)
        row("tile with NaN", P_NAN, 0.5, 0.1, 0)
        row("s NaN", P_A, nan, 0.1, 0)
        row("s inf", P_A, inf, 0.1, 0)
        row("s -inf", P_A, -inf, 0.1, 1)
        row("constant tile, s NaN", P_CONST, nan, 0.1, 0)
        row("constant tile, s inf", P_CONST, inf, 0.1, 0)
        row("constant tile, s -inf", P_CONST, -inf, 0.1, 1)
        row("o inf", P_A, 0.5, inf, 0)
        row("o -inf", P_B, 0.5, -inf, 1)
        row("o NaN", P_A, 0.5, nan, 0)
    tail = [("tail: palindrome, sym 1", P_PAL, 0.6, 0.02, 1),
            ("tail: den at or below 1e-12", P_LO, 3.0, 0.05, 0),
            ("tail: tile with NaN", P_NAN, 0.5, 0.1, 1) if nonfinite else ("tail: tile of -0.0", P_NZ, 0.5, -0.0, 0),
            ("tail: constant tile, s -40", P_CONST, -40.0, -0.0, 1),
            ("tail: idx -1 with s, o, sym set", -1, 0.7, 0.3, 1)]
    assert nr >= len(rows) + N_TAIL, f"a decode edge table needs {len(rows) + N_TAIL} rows or more"
    n_rand = nr - len(rows) - N_TAIL
    idx = np.empty(nr, np.int32)
    s = np.empty(nr, F32)
    o = np.empty(nr, F32)
    sym = np.empty(nr, np.uint8)
    n_head = len(rows)
    for j, (i, sv, ov, sy) in enumerate(rows):
        idx[j], s[j], o[j], sym[j] = i, F32(sv), F32(ov), sy
    a, b = n_head, n_head + n_rand
    ri = rng.integers(0, N_PLAIN, n_rand)
    every5 = np.arange(n_rand) % 5 == 0                # every 5th random row: the special tiles too
    ri[every5] = rng.integers(0, N_POOL, int(every5.sum()))
    ri[np.arange(n_rand) % 53 == 52] = -1              # sentinels among the random rows
    idx[a:b] = ri
    s[a:b] = rng.uniform(-1.2, 1.2, n_rand).astype(F32)
    o[a:b] = rng.normal(0, 0.1, n_rand).astype(F32)
    sym[a:b] = rng.random(n_rand) < 0.5
    for j, (_, i, sv, ov, sy) in enumerate(tail):
        idx[b + j], s[b + j], o[b + j], sym[b + j] = i, F32(sv), F32(ov), sy
    # the edges are present
    negz = lambda x: bool(np.any((x == 0) & np.signbit(x)))  # noqa: E731
    assert negz(s) and negz(o) and negz(pool)
    assert den_of(pool[P_CONST]) == 0 and den_of(pool[P_TINY]) == 0
    assert np.array_equal(pool[P_PAL][::-1], pool[P_PAL]) and np.array_equal(pool[P_TM][::-1], pool[P_T])
    if kind in SCALE:
        with np.errstate(all="ignore"):
            pool = pool * F32(SCALE[kind])
            o = o * F32(SCALE[kind])
    return idx, s, o, sym, pool, names


def labels(names, nr):
    """One label per row of a table of nr rows."""
    return names + ["random"] * (nr - len(names) - N_TAIL) + ["tail"] * N_TAIL


def input_digest(idx, s, o, sym, pool):
    """SHA-256 of a built table (its bytes, little-endian as numpy stores them here)."""
    h = hashlib.sha256()
    for a, t in ((idx, "<i4"), (s, "<f4"), (o, "<f4"), (sym, "u1"), (pool, "<f4")):
        h.update(np.ascontiguousarray(a, t).tobytes())
    return h.hexdigest()


def row_digests(rec, nr, rs):
    """u8[nr, 8]: the first 8 bytes of SHA-256 of each range's reconstruction, every NaN first made the one quiet NaN —
    equal digests are `same_bits_or_nan` of the rows (the fixture keeps these where the rows themselves are too large
    for it)."""
    u = np.ascontiguousarray(rec, "<f4").reshape(nr, rs).copy()
    u.view("<u4")[np.isnan(u)] = 0x7FC00000
    out = np.empty((nr, 8), np.uint8)
    for r in range(nr):
        out[r] = np.frombuffer(hashlib.sha256(u[r].tobytes()).digest()[:8], np.uint8)
    return out


def fmt_delta(v):
    """A Δ as the reference's log prints it (fractal.py:1464, ``{delta:.6e}``) and a reader parses it back."""
    return float(f"{float(v):.6e}")


def same_delta(dev, f64, ref):
    """The device's Δ against the oracle's float64 measure and the reference's own float32 value: equal to the
    reference's (the exact check decided), both NaN, equal to the float64 measure (inf and 0 included), or within
    1e-12 relative of it (tests/test_gpu_decode.py's bar)."""
    if dev == ref or (dev != dev and ref != ref):   # a NaN from the exact check is the reference's NaN
        return True
    if dev != dev and f64 != f64:
        return True
    if dev == f64:
        return True
    return bool(np.isfinite(f64) and abs(dev - f64) <= 1e-12 * abs(f64))
