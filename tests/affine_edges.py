"""Inputs of the affine-solve edge tests (test helper, shared by tests/golden/make_affine_edges.py, the CPU pin of
O.affine and tests/test_gpu_affine_edges.py).

``build(rs, K)`` returns one table of N_ROWS (range, candidate row) pairs over a pool of N_POOL tiles: first the edge
rows below, then random rows.  Every row is solved independently of the others, so a test may solve any slice of the
table and compare it with the same slice of a reference computed once.  An edge row holds only the candidates its
edge is about and −1 everywhere else, so that the edge decides the match."""
import numpy as np

F32 = np.float32
N_POOL = 200
N_PLAIN = 180   # pool rows [0, N_PLAIN) are plain random tiles; the special tiles follow
N_ROWS = 67
# special tiles
P_CONST, P_T, P_TM, P_PAL, P_A, P_BIG, P_INF, P_NAN, P_TINY, P_B = range(N_PLAIN, N_PLAIN + 10)

RS_ALL = (4, 5, 8, 16, 19, 32, 40, 130)
K_ALL = (1, 2, 63, 64, 65, 129)
ROWS_ALL = (1, 15, 16, 17, 67)
# the shapes whose reference outputs are recorded in tests/golden/affine_edges.npz: every dispatch path of fwav_affine
# (batched: rs 4/8/16 with K ≤ 64; one wave per range: rs 4/8/16 with K > 64; runtime-sized: any other rs)
FIXTURE_SHAPES = ((4, 64), (8, 2), (16, 65), (5, 63), (19, 17), (32, 129), (130, 1))


def build(rs, K, seed=0):
    """→ (ranges f32[N_ROWS, rs], cand i32[N_ROWS, K], pool f32[N_POOL, rs], names: one label per edge row)."""
    rng = np.random.default_rng(1000 * rs + K + seed)
    pool = rng.normal(0, 0.3, (N_POOL, rs)).astype(F32)
    pool[P_CONST] = F32(0.25)                       # Σd̃² = 0: den = 1e-12
    pool[P_TM] = pool[P_T][::-1]                    # exact mirror of P_T
    h = rs // 2
    pool[P_PAL, rs - h:] = pool[P_PAL, :h][::-1]    # palindrome: the mirrored slot has the same error
    pool[P_BIG] = F32(3e38) * np.sign(pool[P_BIG])  # sums overflow
    pool[P_INF, rs // 3] = F32(np.inf)
    pool[P_NAN, rs // 2] = F32(np.nan)
    pool[P_TINY] = pool[P_TINY] * F32(1e-30)        # Σd̃² underflows to 0
    ranges, cand, names = [], [], []

    def row(name, r, cs, at=0):
        c = np.full(K, -1, np.int32)
        cs = list(cs)[:max(0, K - at)]
        c[at:at + len(cs)] = cs
        ranges.append(np.asarray(r, F32))
        cand.append(c)
        names.append(name)

    def rnd():
        return rng.normal(0, 0.3, rs).astype(F32)

    def plain(n):
        return rng.integers(0, N_PLAIN, n)

    row("all -1", rnd(), [])
    row("-1 tail from K/2", rnd(), plain(K // 2))
    row("only the last slot", rnd(), plain(1), at=K - 1)
    row("constant tile", rnd(), [P_CONST])
    row("constant range", np.full(rs, 0.3, F32), plain(2))
    row("tile, mirror", rnd(), [P_T, P_TM])
    row("mirror, tile", rnd(), [P_TM, P_T])
    row("palindromic tile", rnd(), [P_PAL])
    row("same domain twice", rnd(), [P_B, P_B])
    row("s clipped high", F32(40) * pool[P_A] + F32(0.5), [P_A])
    row("s clipped low, mirrored", F32(-40) * pool[P_A][::-1], [P_A])
    row("overflowing tile", rnd(), [P_BIG])
    row("overflowing tile after a finite one", rnd(), [P_B, P_BIG])
    row("tile with inf", rnd(), [P_INF])
    row("tile with inf after a finite one", rnd(), [P_B, P_INF])
    row("NaN tile after a finite one", rnd(), [P_B, P_NAN, P_A])
    row("NaN tile in the last slot", rnd(), [P_NAN], at=K - 1)
    row("tiny tile", rnd(), [P_TINY])
    row("tiny range and tile", rnd() * F32(1e-30), [P_TINY, P_B])
    n_edge = len(names)
    for j in range(N_ROWS - n_edge):
        ranges.append(rnd())
        c = rng.integers(0, N_POOL if j % 5 == 0 else N_PLAIN, K).astype(np.int32)  # every 5th: special tiles too
        cand.append(c)
    return np.stack(ranges), np.stack(cand), pool, names


def same_bits_or_nan(a, b):
    """Bit-equal, except that a NaN matches any NaN (sign and payload differ between x86 numpy and the device)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def slices(n):
    """The row slices of the table solved for a call of n rows: the first 67, every chunk of 15 / 16 / 17 (the last
    one moved back to stay inside the table), and for n = 1 every row on its own."""
    if n >= N_ROWS:
        return [(0, N_ROWS)]
    out = [(a, a + n) for a in range(0, N_ROWS - n + 1, n)]
    if out[-1][1] < N_ROWS:
        out.append((N_ROWS - n, N_ROWS))
    return out
