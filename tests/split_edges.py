"""Tables and plain numpy restatements for the thread-split edge tests (test helper, shared by
tests/test_split_edges_cpu.py and tests/test_gpu_split_edges.py; no torch).

The reference's scores are ``domain_embs @ q`` in OpenBLAS's sgemv_t order.  From emb_dim·n_domains = 460,800 up
OpenBLAS splits the columns over its T threads, and each thread's chunk ends in (width mod 4) columns that the 4x2
(kind 1) and 4x1 (kind 2) tail kernels score, in another summation order than the 4-column kernel (kind 0).  The device
restates that in fwav_common.h (make_sgemv_split[_dim], sgemv_kind, sgemv_chunk_start, sgemv16 / sgemv_dim).

The grid (``CASES``): the smallest tables at which that code is live — 28,800 rows of 16 floats, 14,400 of 32 — one
row below, and a few rows above, at thread counts that give chunk widths of every residue mod 4.

The table of a case (``Case``): unit-head rows; the first NQ rows are the queries, each a small perturbation of a
body row (its source: index ≥ NQ, kind 0 under every thread count of the grid); every tail column of the case's T is
then overwritten with the bits of a source, dealt round-robin to the queries (tail column j: the source of query
j mod NQ).  A query's candidate row is then headed by its source and the source's copies — equal bits, so only the
sgemv kernel that scores each decides their order — and then the query itself.  A kernel that scored every column
with kind 0, or with another T's split, ranks them differently (tests/test_split_edges_cpu.py asserts that it does,
per case).
The fewer tail columns a case has, the more queries share a source (COPIES tail columns per source where there are
enough), so that even a single tail column stands in many candidate rows.

The restatements: O.sgemv_scores / O.sgemv_col_kind at width 16, ``sgemv_dim_np`` / ``col_kinds`` at width 32 (both
pinned against numpy's own product under threadpoolctl); candidate rows in (score desc, index asc) order, −1 padded;
the tie list from tie_edges.expected_list."""
import functools

import numpy as np

import tie_edges as TE
from oracle import fractal_oracle as O

F32 = np.float32
THREAD_MIN_MN = 460800  # OpenBLAS: sgemv on one thread while m·n is below this

NQ = 96          # queries: table rows 0 … NQ − 1
COPIES = 3       # tail columns per source where a case has enough of them
K_COVER = 8      # the K of the coverage conditions
K_ALL = (8, 64, 65)
# queries whose whole score row is kept (score-row tests, numpy comparison): these, after the queries a case picks so
# that every tail column's score differs in bits from its kind-0 score in some kept row (Case.full_q)
FULL_Q = (5, 6, 17, 40, 41, 77, 94, 95)
FULL_MIN, FULL_MAX, Q_OFFSET = 8, 16, 5  # kept rows per case; the score-row tests' non-zero q_offset (kept rows ≥ it)
KEEP = 67        # per query, the columns whose score is among the KEEP largest are kept (K ≤ 65 and the (K+1)-th)
# a query = its source plus normal noise of σ = SIGMA·sqrt(8 / head width) per entry, each head normalised and scaled
# by SHRINK.  A head's cosine to its source is then about 0.99, so the source and its copies (norm 1) score about
# 1.98·SHRINK, the query itself 2·SHRINK² (below them: SHRINK < 0.98), and another query of the same source at most
# 2·SHRINK² — never above the source, however the two queries' noise happens to agree.
SIGMA, SHRINK = 0.05, 0.97

T16 = (2, 3, 7, 16, 17, 33, 64)
T32 = (3, 7, 16, 64)
GRID16 = [(28799, 1), (28799, 16)] + [(nd, T) for nd in (28800, 28801, 28802, 28803, 28867) for T in T16] + \
    [(28803, 1)]
# (14414 = 7·2059 + 1: the one "one wider" chunk of width ≡ 0 mod 4 at width 32, which the rest of the grid lacks)
GRID32 = [(14399, 1), (14399, 16)] + [(nd, T) for nd in (14400, 14401, 14402, 14403, 14467) for T in T32] + \
    [(14414, 7)]
CASES = [(16, nd, T) for nd, T in GRID16] + [(32, nd, T) for nd, T in GRID32]
CONTROL = {16: (16, 28800, 16), 32: (32, 14400, 16)}  # no tail column at all
# the cases that also run the fp16 knob paths and the product sequence: per width one with both tail kinds, the control
KNOB_CASES = [(16, 28803, 7), (16, 28867, 33), (16, 28800, 64), CONTROL[16]]
PRODUCT_CASES = [(16, 28803, 7), CONTROL[16], (32, 14403, 7), CONTROL[32]]
SEED = {}  # (width, nd, T) → seed, where the default misses a coverage bar


def case_id(c):
    return f"w{c[0]}-nd{c[1]}-T{c[2]}"


# ------------------------------------------------------------------------------------------------ sgemv order
def col_kinds(nd: int, threads: int, dim: int = 32) -> np.ndarray:
    """fwav_common.h make_sgemv_split_dim + sgemv_kind: which sgemv_t kernel scores each of the nd columns."""
    T = 1 if dim * nd < THREAD_MIN_MN else max(1, int(threads))
    q, r = divmod(nd, T)
    d = np.arange(nd)
    big = d < r * (q + 1)
    w = np.where(big, q + 1, q)
    start = np.where(big, d // (q + 1) * (q + 1), r * (q + 1) + (d - r * (q + 1)) // max(q, 1) * q)
    pos, t = d - start, w & 3
    return np.where(pos < w - t, 0, np.where(((t & 2) != 0) & (pos < w - t + 2), 1, 2)), {int(x) for x in np.unique(w)}


def sgemv_dim_np(E: np.ndarray, q: np.ndarray, kinds: np.ndarray) -> np.ndarray:
    """fwav_common.h sgemv_dim on every row of E (nd, dim), restated in numpy."""
    E, q = np.asarray(E, F32), np.asarray(q, F32)
    nd, dim = E.shape
    P = E * q[None, :]  # separately rounded f32 products
    l0 = np.zeros((nd, 8), F32)
    for b in range(dim // 8):
        sl = slice(8 * b, 8 * b + 8)
        l0 = O.fma_f32(E[:, sl].astype(np.float64) * q[None, sl].astype(np.float64), l0.astype(np.float64))
    fold8 = lambda l: ((l[:, 0] + l[:, 4]) + (l[:, 1] + l[:, 5])) + ((l[:, 2] + l[:, 6]) + (l[:, 3] + l[:, 7]))  # noqa: E731
    l1 = np.zeros((nd, 4), F32)
    l2 = np.zeros((nd, 8), F32)
    for k in range(dim):
        l1[:, k % 4] = l1[:, k % 4] + P[:, k]
        l2[:, k % 8] = l2[:, k % 8] + P[:, k]
    k1 = (l1[:, 0] + l1[:, 1]) + (l1[:, 2] + l1[:, 3])
    return np.where(kinds == 0, fold8(l0), np.where(kinds == 1, k1, fold8(l2))).astype(F32)


def unit_head_rows(rng, n: int, dim: int = 32) -> np.ndarray:
    """n rows of two f32 heads, each normalised in f32 as the reference normalises them."""
    x = rng.normal(0, 1, (n, 2, dim // 2)).astype(F32)
    x = x / np.sqrt((x * x).sum(-1, dtype=F32))[..., None]
    return np.ascontiguousarray(x.reshape(n, dim).astype(F32))


def kinds_of(width: int, nd: int, T: int) -> np.ndarray:
    """The kernel (0, 1, 2) that scores each of the nd columns under T BLAS threads."""
    if width == 16:
        return np.asarray(O.sgemv_col_kind(np.arange(nd), nd, T), np.int8)
    return np.asarray(col_kinds(nd, T, width)[0], np.int8)


def chunk_widths(width: int, nd: int, T: int):
    """(width of the "one wider" chunks or None, width of the regular ones) of the split under T threads."""
    T = 1 if width * nd < THREAD_MIN_MN else max(1, int(T))
    q, r = divmod(nd, T)
    return (q + 1 if r else None), q


def scores(width: int, E: np.ndarray, Q: np.ndarray, kinds) -> np.ndarray:
    """The restated score rows f32[len(Q), len(E)]: E @ q per query, column d by the kernel kinds[d]."""
    kinds = np.asarray(kinds)
    if len(E) == 0:
        return np.zeros((len(Q), 0), F32)
    if width == 16:
        return np.ascontiguousarray(O.sgemv_scores(E, Q, kinds), F32)
    return np.stack([sgemv_dim_np(E, q, kinds) for q in Q])


def top_rows(sel_scores, K: int) -> np.ndarray:
    """Candidate rows in (score desc, index asc) order, −1 padded, from per-query (columns ascending, their scores)."""
    out = np.full((len(sel_scores), K), -1, np.int32)
    for j, (sel, s) in enumerate(sel_scores):
        o = np.lexsort((sel, -s.astype(np.float64)))[:K]
        out[j, :len(o)] = sel[o]
    return out


def keep_top(S: np.ndarray, keep: int):
    """Per score row: (the columns whose score is at least the keep-th largest, ascending; their scores)."""
    out = []
    for row in S:
        th = np.partition(row, len(row) - keep)[len(row) - keep] if len(row) > keep else -np.inf
        sel = np.flatnonzero(row >= th)
        out.append((sel, row[sel].copy()))
    return out


def tie_list(sel_scores, K: int) -> dict:
    """tie_edges.expected_list of every query, from the kept columns: they hold the whole top K + 1 and every column
    that equals the K-th score, in ascending index order, so the list is that of the whole row."""
    out = {}
    for q, (sel, s) in enumerate(sel_scores):
        assert len(sel) > K + 1
        for _, (flag, n, m) in TE.expected_list([s], K, [q]).items():
            out[q] = (flag, n, sel[m].astype(np.int32))
    return out


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """One (width, nd, T): the table, the kinds, the kept part of every query's restated score row (under the case's
    kinds), whole rows for the queries full_q, and the K_COVER rankings under all-kind-0 and under the one-thread split."""

    def __init__(self, width, nd, T, seed=None):
        self.width = self.emb_dim = width
        self.nd, self.T, self.nq, self.max_q, self.q_offset = nd, T, NQ, NQ, 0
        seed = SEED.get((width, nd, T), 0) if seed is None else seed
        rng = np.random.default_rng(1_000_003 * width + 31 * nd + 7_919 * seed)  # not of T: below the threshold one table
        E = unit_head_rows(rng, nd, width)
        kind = kinds_of(width, nd, T)
        tail = np.flatnonzero(kind)
        safe = np.ones(nd, bool)
        safe[:NQ] = False
        for t in sorted({1, 16} | set(T16 if width == 16 else T32)):
            safe &= kinds_of(width, nd, t) == 0
        n_src = int(min(NQ, max(1, -(-len(tail) // COPIES))))
        src = np.sort(rng.choice(np.flatnonzero(safe), n_src, replace=False))
        self.src_of_q = src[np.arange(NQ) % n_src]
        x = E[self.src_of_q] + rng.normal(0, SIGMA * np.sqrt(16.0 / width), (NQ, width)).astype(F32)
        x = x.reshape(NQ, 2, width // 2)
        x = x / np.sqrt((x * x).sum(-1, dtype=F32))[..., None] * F32(SHRINK)
        E[:NQ] = x.reshape(NQ, width).astype(F32)
        assert (np.sqrt((E[:NQ].reshape(NQ, 2, -1).astype(np.float64) ** 2).sum(-1)) <= 1).all()
        srcrows = E[self.src_of_q].copy()
        for j, col in enumerate(tail):
            E[col] = srcrows[j % NQ]
        self.t = self.E = np.ascontiguousarray(E)
        self.kind, self.tail = kind, tail
        self.kind1 = kinds_of(width, nd, 1)
        self.ids = np.arange(NQ, dtype=np.int32)
        self.row_of = {q: q for q in range(NQ)}
        Q = self.E[:NQ]
        S0 = scores(width, self.E, Q, np.zeros(nd, np.int8))
        S = S0.copy()
        S[:, tail] = scores(width, self.E[tail], Q, kind[tail])
        S1 = S0.copy()
        t1 = np.flatnonzero(self.kind1)
        S1[:, t1] = scores(width, self.E[t1], Q, self.kind1[t1])
        self.top = keep_top(S, KEEP)
        differ = S[:, tail].view(np.uint32) != S0[:, tail].view(np.uint32)  # (query, tail column)
        self.full_q = self._pick_full(differ)
        self.full = {q: S[q].copy() for q in self.full_q}
        self.full_bits_differ = differ[list(self.full_q)].any(axis=0)
        self.rows_kind0 = top_rows(keep_top(S0, K_COVER + 1), K_COVER)
        self.rows_one_thread = top_rows(keep_top(S1, K_COVER + 1), K_COVER)
        # per tail column: does some query's score differ in bits between the column's kind and kind 0?
        self.tail_bits_differ = differ.any(axis=0)
        self._rows, self._exp = {}, {}

    @staticmethod
    def _pick_full(differ):
        """Greedily, the queries (≥ Q_OFFSET) in whose rows the most tail columns not yet covered differ in bits from
        their kind-0 score; then FULL_Q's, up to FULL_MIN rows at least.  Chosen from the restatement alone."""
        picked, todo = [], np.ones(differ.shape[1], bool)
        while todo.any() and len(picked) < FULL_MAX:
            gain = (differ[Q_OFFSET:, todo]).sum(axis=1)
            if gain.max() == 0:
                break
            q = Q_OFFSET + int(np.argmax(gain))
            picked.append(q)
            todo &= ~differ[q]
        for q in FULL_Q:
            if len(picked) >= FULL_MIN:
                break
            if q not in picked:
                picked.append(q)
        return tuple(sorted(picked))

    def rows(self, K):
        """The expected candidate rows i32[NQ, K]."""
        if K not in self._rows:
            self._rows[K] = top_rows(self.top, K)
        return self._rows[K]

    def exp(self, K):
        """The expected tie list {query: (flag, count, members)}."""
        if K not in self._exp:
            self._exp[K] = tie_list(self.top, K)
        return self._exp[K]

    def view(self, K):
        """The attributes tests/test_gpu_tie_edges.py's check_search and f16_paths read of a tie_edges.Case."""
        return View(self, K)


class View:
    def __init__(self, c, K):
        self.c, self.K, self.nd, self.emb_dim, self.max_q, self.q_offset = c, K, c.nd, c.width, c.max_q, 0
        self.t, self.ids, self.row_of = c.E, c.ids, c.row_of
        self.dev, self.exp = c.rows(K), c.exp(K)
        # (f16_paths reads only the K-th score of each row: rows[j][dev[j][K − 1]])
        self.rows = [dict(zip(sel.tolist(), s.tolist())) for sel, s in c.top]


@functools.lru_cache(maxsize=None)
def case(width, nd, T):
    return Case(width, nd, T)
