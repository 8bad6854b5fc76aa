"""Inputs and plain numpy restatements for the tie-list and tie-check edge tests (test helper, shared by
tests/test_tie_edges_cpu.py and tests/test_gpu_tie_edges.py; no torch).

Exact ties on demand.  ``table`` builds embedding rows whose entries are multiples of 1/16 with |entry| ≤ 6/16 and at
most five non-zeros per head: every product is a multiple of 1/256 and every partial sum is exact in float32, so the
score row ``t @ t[i]`` is the same in any summation order (any BLAS thread count, the device's sgemv order, the fp16
pre-filter: the fp16 high part is the value itself and the low part zero) and numpy's own product is the exact truth.
Scores then lie on a grid of 1/256, which makes equal scores plentiful: inside the top K, at the K-th place, at 0.

``pool_and_ranges`` draws the pool from a handful of distinct coarse rows, so that equal errors under different
indices are common — which is what makes the order of equal scores matter to the match.

The restatements:
  ``expected_list``    the tie list fwav_sim_topk must write (flag, left-out members of the K-th score's group);
  ``admissible_rows``  the candidate rows numpy may return for a score row (equal scores in any order, the last places
                       any subset of the K-th score's group);
  ``depends_rule``     the rule documented above k_tie_check (fwav_affine.hip), from per-slot errors;
  ``truly_depends``    whether some admissible row gives another match tuple than the device-order row — independent
                       of the rule: the soundness reference."""
import functools
import itertools
import math

import numpy as np

from oracle import fractal_oracle as O

F32 = np.float32
TIE_REC = 9            # int32 per tie record (kTieRec)
MAX_LEFT = TIE_REC - 2  # left-out members a record can carry
MAX_ALL = 5040         # every admissible row is enumerated up to this many
N_RANDOM = 64

ND_ALL = (40, 64, 65, 257, 600)
K_ALL = (1, 2, 17, 32, 63, 64)
MAX_Q = 129
RS_OF_ND = {40: 4, 64: 5, 65: 8, 257: 16, 600: 19}  # the range size each table is paired with in the product sequence
# distinct pool rows and seed per table, tuned until every (nd, K) shape holds every class it can (can_hold below;
# tests/test_tie_edges_cpu.py asserts it)
POOL_DISTINCT = {40: 8, 64: 8, 65: 14, 257: 6, 600: 6}
SEED_OF_ND = {40: 15, 64: 0, 65: 2, 257: 1, 600: 0}


# --------------------------------------------------------------------------------------------------- builders
def table(nd, seed=0, emb_dim=16):
    """The dyadic embedding table: nd rows of two heads of emb_dim/2 columns, 1–5 non-zeros per head drawn from
    {±1 … ±6}/16 (a head's sum of squares is at most 180/256 < 1).  Every 37th row is zero, every 41st row is a copy of
    row 5, every 11th row keeps only its first head and every 13th only its second (their scores against each other
    are exactly 0)."""
    rng = np.random.default_rng(7919 * nd + 31 * emb_dim + seed)
    h = emb_dim // 2
    t = np.zeros((nd, 2, h), F32)
    for i in range(nd):
        for head in range(2):
            nz = rng.integers(1, 6)
            cols = rng.choice(h, nz, replace=False)
            t[i, head, cols] = rng.choice([-1, 1], nz) * rng.integers(1, 7, nz) / 16.0
    t[0::11, 1] = 0
    t[0::13, 0] = 0
    t = t.reshape(nd, emb_dim)
    t[0::37] = 0
    if nd > 5:
        t[41::41] = t[5]
    assert np.array_equal(t * 16, np.round(t * 16)) and np.abs(t).max() <= 6 / 16
    assert ((t.reshape(nd, 2, h).astype(np.float64) ** 2).sum(-1) <= 1).all()
    return np.ascontiguousarray(t)


def overflow_table(nd=600, copies=250, seed=0):
    """``table`` with `copies` rows replaced by one row: its queries' bands overflow the fp16 search's buffer."""
    t = table(nd, seed + 1)
    rng = np.random.default_rng(seed + 5)
    t[rng.choice(np.arange(1, nd), copies, replace=False)] = t[1]
    return t


def queries(t, q_offset=0, max_q=MAX_Q):
    """Local ids of the searchable queries: local i is table row q_offset + i; all-zero rows are not searched."""
    n = min(max_q, len(t) - q_offset)
    return np.nonzero(t[q_offset:q_offset + n].any(axis=1))[0].astype(np.int32)


def score_rows(t, rows):
    """numpy's own score rows (fractal.py:537), one sgemv per query as the reference."""
    return np.stack([t @ t[r] for r in rows]) if len(rows) else np.zeros((0, len(t)), F32)


def pool_and_ranges(nd, nq, rs, seed=0, n_distinct=None):
    """→ (pool f32[nd, rs], ranges f32[nq, rs]) on the grid round(normal·2)/4.  The pool is n_distinct distinct rows
    assigned at random to the domains, independently of the embedding: a constant row, a palindrome, a row and its
    mirror, the rest plain; one domain holds a row with +inf and one a row with NaN.  Every 29th range is
    constant (every candidate then fits equally)."""
    n_distinct = POOL_DISTINCT.get(nd, 10) if n_distinct is None else n_distinct
    assert n_distinct >= 6
    rng = np.random.default_rng(104729 * nd + 1009 * rs + seed)

    def coarse(*shape):
        return (np.round(rng.normal(0, 1, shape) * 2) / 4).astype(F32)

    rows = coarse(n_distinct, rs)
    for i in range(n_distinct):  # no accidentally constant plain row
        if np.all(rows[i] == rows[i, 0]):
            rows[i, 0] += F32(0.25)
    rows[0] = F32(0.25)
    half = rs // 2
    rows[1, rs - half:] = rows[1, :half][::-1]
    rows[3] = rows[2][::-1]
    rows[4, rs // 3] = F32(np.inf)
    rows[5, rs // 2] = F32(np.nan)
    plain = np.r_[0:4, 6:n_distinct]
    pool = rows[rng.choice(plain, nd)]
    bad = rng.choice(nd, 2, replace=False)  # one domain each: most candidate rows of the larger tables hold neither
    pool[bad[0]], pool[bad[1]] = rows[4], rows[5]
    ranges = coarse(nq, rs)
    ranges[28::29] = F32(0.5)
    return np.ascontiguousarray(pool), np.ascontiguousarray(ranges)


# ------------------------------------------------------------------------------------ the list and the rows
def device_order(score_row):
    """Every domain in (score desc, index asc) order."""
    return np.lexsort((np.arange(len(score_row)), -score_row.astype(np.float64)))


def device_row(score_row, K):
    out = np.full(K, -1, np.int32)
    o = device_order(score_row)[:K]
    out[:len(o)] = o
    return out


def expected_list(rows, K, ids=None):
    """{query id: (flag, count, members)} for the score rows whose top K + 1 scores hold exactly equal values:
    flag = 1 for a tie at the K-th place (the K-th and (K+1)-th scores are equal), and then members = the domains
    outside the K with the K-th's score in index order, count = how many; else flag 0, count 0, no members."""
    out = {}
    for j, row in enumerate(rows):
        nd = len(row)
        o = device_order(row)
        s = row[o]
        top = s[:K + 1]
        if not (top[1:] == top[:-1]).any():
            continue
        q = int(j if ids is None else ids[j])
        if nd > K and s[K - 1] == s[K]:
            m = o[K:][s[K:] == s[K - 1]]
            out[q] = (1, len(m), m.astype(np.int32))
        else:
            out[q] = (0, 0, np.zeros(0, np.int32))
    return out


def list_array(exp, max_q, mode="full", order=None):
    """The int32 tie list of `exp` as the search writes it (fwav_tie_list_size(max_q) entries, unused ones −7):
    mode "full" (count and members; −1 above MAX_LEFT), "uncollected" (every count −1) or "reversed" (the members in
    descending index order).  `order`: the records' order (default ascending query id)."""
    t = np.full(1 + TIE_REC * max(max_q, 1), -7, np.int32)
    qs = sorted(exp) if order is None else list(order)
    t[0] = len(qs)
    for j, q in enumerate(qs):
        flag, n, m = exp[q]
        rec = t[1 + TIE_REC * j:1 + TIE_REC * (j + 1)]
        rec[0] = 2 * q + flag
        if flag:
            if mode == "uncollected" or n > MAX_LEFT:
                rec[1] = -1
            else:
                rec[1] = n
                rec[2:2 + n] = m[::-1] if mode == "reversed" else m
    return t


def parse_list(t):
    """→ [(query, flag, count, members)] of a tie list read back from the device."""
    n = int(t[0])
    recs = t[1:1 + TIE_REC * n].reshape(n, TIE_REC)
    return [(int(r[0]) >> 1, int(r[0]) & 1, int(r[1]), r[2:].copy()) for r in recs]


def _structure(score_row, K):
    """(runs above the K-th score: index arrays in device order, the K-th score's whole group, the places m it fills).
    With nd ≤ K every domain is returned and the last run is simply a run (m = its length)."""
    o = device_order(score_row)
    s = score_row[o]
    kk = min(K, len(o))
    kth = s[kk - 1]
    above = o[s > kth]
    sa = s[:len(above)]
    runs, start = [], 0
    for i in range(1, len(sa) + 1):
        if i == len(sa) or sa[i] != sa[start]:
            runs.append(above[start:i])
            start = i
    group = o[s == kth]
    return runs, group, kk - len(above)


def n_admissible(score_row, K):
    runs, group, m = _structure(score_row, K)
    n = math.perm(len(group), m)
    for r in runs:
        n *= math.factorial(len(r))
    return n


def admissible_rows(score_row, K, seed=0):
    """The candidate rows numpy may return for this score row: the scores strictly above the K-th's are fixed, each run
    of equal scores may come in any order, and the last places hold any subset of the K-th score's group in any order.
    → (device-order row, variants i32[n, K], exhaustive).  The variants are every admissible row when there are at
    most MAX_ALL of them (exhaustive = True); else targeted ones — each member of each run first in its run with the
    rest in ascending and in descending index order, each group member forced in and forced out — plus N_RANDOM seeded
    random ones.  Rows are −1 padded when nd < K."""
    runs, group, m = _structure(score_row, K)
    dev = device_row(score_row, K)
    g = len(group)

    def assemble(run_orders, tail):
        row = np.full(K, -1, np.int32)
        parts = list(run_orders) + [tail]
        cat = np.concatenate(parts) if parts else np.zeros(0, np.int64)
        row[:len(cat)] = cat
        return row

    base = [r.copy() for r in runs]
    out = []
    if n_admissible(score_row, K) <= MAX_ALL:
        run_perms = [list(itertools.permutations(r)) for r in runs]
        tails = list(itertools.permutations(group, m))
        for combo in itertools.product(*run_perms):
            for tail in tails:
                out.append(assemble([np.array(c, np.int64) for c in combo], np.array(tail, np.int64)))
        return dev, np.stack(out), True
    for i, r in enumerate(runs):
        for a in range(len(r)):
            rest = np.delete(r, a)
            for rr in (rest, rest[::-1]):
                ro = list(base)
                ro[i] = np.r_[r[a], rr]
                out.append(assemble(ro, group[:m]))
    for a in range(g):
        rest = np.delete(group, a)
        if m >= 1:  # forced in, first of the group's places, the rest ascending and descending
            out.append(assemble(base, np.r_[group[a], rest[:m - 1]]))
            out.append(assemble(base, np.r_[group[a], rest[::-1][:m - 1]]))
            out.append(assemble(base, np.r_[rest[::-1][:m - 1], group[a]]))
        if g > m:   # forced out
            out.append(assemble(base, rest[:m]))
            out.append(assemble(base, rest[::-1][:m]))
    rng = np.random.default_rng(seed + 17 * K + len(score_row))
    for _ in range(N_RANDOM):
        out.append(assemble([rng.permutation(r) for r in runs], rng.permutation(group)[:m]))
    return dev, np.stack(out), False


def is_admissible(row, score_row, K):
    """`row` is one of the rows admissible_rows describes: the same members outside the K-th score's group, each run
    only permuted, the last places distinct members of the group."""
    runs, group, m = _structure(score_row, K)
    kk = min(K, len(score_row))
    row = np.asarray(row)
    if len(row) != K or (row[kk:] != -1).any():
        return False
    p = 0
    for r in runs:
        if sorted(row[p:p + len(r)].tolist()) != sorted(r.tolist()):
            return False
        p += len(r)
    tail = row[p:kk].tolist()
    return len(tail) == m and len(set(tail)) == m and set(tail) <= set(group.tolist())


# ----------------------------------------------------------------------------------------- match tuples
def _tuple_bytes(idx, s, o, sym, err):
    """One match tuple per row as bytes (a NaN compares equal to the same NaN: both come from the same slot values)."""
    m = np.empty(len(idx), O.MATCH_DTYPE)
    m["idx"], m["s"], m["o"], m["sym"], m["err"] = idx, s, o, sym, err
    return m


def slot_table(rng_row, doms, pool):
    """(s, o, err) of every domain of `doms` against one range, both orientations: (2, len(doms)) each.  A slot's
    values depend on its range and tile alone (O.affine_slots), so a candidate row's slots are a gather of these."""
    with np.errstate(all="ignore"):
        s, o, e = O.affine_slots(rng_row[None, :], np.asarray(doms, np.int32)[None, :], pool)
    n = len(doms)
    return s[0].reshape(2, n), o[0].reshape(2, n), e[0].reshape(2, n)


def tuples_of_rows(rng_row, rows, pool, s_clip=16.0):
    """O.affine's match tuple of each candidate row in `rows` (n, K) for one range, as a structured array — computed
    from one slot table of the distinct domains (tests/test_tie_edges_cpu.py checks it against O.affine itself)."""
    rows = np.asarray(rows, np.int32)
    n, K = rows.shape
    doms = np.unique(rows[rows >= 0])
    s, o, e = slot_table(rng_row, doms, pool)
    pos = np.searchsorted(doms, np.where(rows < 0, doms[0] if len(doms) else 0, rows))
    inval = rows < 0
    ev = np.concatenate([np.where(inval, F32(np.inf), e[0][pos]), np.where(inval, F32(np.inf), e[1][pos])], axis=1)
    with np.errstate(all="ignore"):
        j = np.argmin(ev, axis=1)
    ar = np.arange(n)
    orient, slot = j // K, j % K
    p = pos[ar, slot]
    c = abs(F32(s_clip))
    safe = np.where(inval, 0, rows)
    return _tuple_bytes(safe[ar, slot], np.clip(s[orient, p], -c, c).astype(F32), o[orient, p], orient.astype(np.uint8),
                        ev[ar, j])


def truly_depends(score_row, K, rng_row, pool, seed=0):
    """True when some admissible candidate row's match tuple differs bytewise from the device-order row's."""
    dev, var, _ = admissible_rows(score_row, K, seed)
    t = tuples_of_rows(rng_row, np.vstack([dev[None, :], var]), pool)
    return bool((t[1:].tobytes() != t[:1].tobytes() * (len(t) - 1)))


# ------------------------------------------------------------------------------------------------ the rule
def _same(a, b):
    return (np.isnan(a) & np.isnan(b)) | (a == b)


def _first_min(e):
    """The error numpy's argmin picks: the first NaN, else the first minimum."""
    with np.errstate(all="ignore"):
        return e[np.argmin(e)] if len(e) else F32(np.inf)


def depends_rule(score_row, K, cand_row, flag, count, members, rng_row, pool, exact_sets=0):
    """The rule above k_tie_check (fwav_affine.hip), restated: must this listed query be resolved on the host?
    `cand_row` is the emitted row, (flag, count, members) its tie record (count −1: group not collected).
      K > 64, or exact_sets 2: always.  A K-th place tie with exact_sets 1 or an uncollected group: always.
      A K-th place tie otherwise: G = the candidates with the K-th's score plus the recorded members; resolve unless
        every member of G fits strictly worse, in both orientations, than the best candidate outside G (a NaN on
        either side, or nothing outside G, is never strictly worse).
      Then, for every listed query: of the slots attaining the minimum error (the originals; the mirrors only when no
        original does), the first keeps its candidate unless another candidate of the same run of equal scores attains
        it too."""
    if K > 64 or exact_sets >= 2:
        return True
    if flag and (exact_sets or count < 0):
        return True
    cand_row = np.asarray(cand_row)
    valid = cand_row >= 0
    doms = cand_row[valid]
    _, _, e = slot_table(rng_row, doms, pool)
    e0 = np.full(K, np.inf, F32)
    e1 = np.full(K, np.inf, F32)
    e0[valid], e1[valid] = e[0], e[1]
    sc = np.full(K, np.nan, F32)
    sc[valid] = score_row[doms]
    with np.errstate(all="ignore"):
        if flag:
            in_g = valid & (sc == sc[K - 1])
            out = valid & ~in_g
            bo = _first_min(np.r_[e0[out], e1[out]])
            ge = [e0[in_g], e1[in_g]]
            if count > 0:
                _, _, em = slot_table(rng_row, members[:count], pool)
                ge += [em[0], em[1]]
            if not np.all(np.concatenate(ge) > bo):
                return True
        be = _first_min(np.r_[e0, e1])
        att = valid & _same(e0, be)
        if not att.any():
            att = valid & _same(e1, be)
        first = int(np.argmax(att))
        return int((att & (sc == sc[first])).sum()) >= 2


# ------------------------------------------------------------------------------------------- whole cases
class Case:
    """One (table, K) with its pool and ranges: per searchable query the score row, the device-order row, the expected
    tie record, and both decisions.  Built once per argument tuple (``case``)."""

    def __init__(self, nd, K, rs, seed=0, emb_dim=16, q_offset=0, tab=None, decisions=True):
        self.nd, self.K, self.rs, self.q_offset, self.emb_dim = nd, K, rs, q_offset, emb_dim
        self.t = table(nd, seed, emb_dim) if tab is None else tab
        self.ids = queries(self.t, q_offset)
        self.max_q = int(min(MAX_Q, nd - q_offset))
        self.rows = score_rows(self.t, self.ids + q_offset)
        self.dev = np.stack([device_row(r, K) for r in self.rows])
        self.exp = expected_list(self.rows, K, self.ids)
        self.pool, self.ranges = pool_and_ranges(nd, self.max_q, rs, seed)
        self.row_of = {int(q): j for j, q in enumerate(self.ids)}
        self.rule, self.truly = {}, {}
        if decisions:
            for q, (flag, n, m) in self.exp.items():
                j = self.row_of[q]
                cnt = n if n <= MAX_LEFT else -1
                self.rule[q] = depends_rule(self.rows[j], K, self.dev[j], flag, cnt, m, self.ranges[q], self.pool)
                self.truly[q] = truly_depends(self.rows[j], K, self.ranges[q], self.pool) if K <= 64 else None

    def classes(self):
        """Query counts per class of the coverage condition (tests/test_tie_edges_cpu.py)."""
        c = dict.fromkeys(CLASSES, 0)
        for q, (flag, n, m) in self.exp.items():
            j = self.row_of[q]
            rule, truly = self.rule[q], self.truly[q]
            sk = self.rows[j][self.dev[j][:min(self.K, self.nd)]]
            if not flag:
                c["in-K keep" if not rule else "in-K depends" if truly else "in-K conservative"] += 1
                c["left out 0"] += bool(len(sk) >= 2 and sk[-1] == sk[-2])  # the K-th score's run ends at place K
            else:
                if n > MAX_LEFT:
                    c["K-th >7 left out"] += 1
                elif not rule:
                    c["K-th keep"] += 1
                elif truly:
                    c["K-th depends"] += 1
                else:
                    c["K-th conservative"] += 1
                c["left out 1"] += n == 1
                c["left out 7"] += n == MAX_LEFT
                c["left out 8"] += n == MAX_LEFT + 1
                c["K-th score 0"] += bool(sk[-1] == 0)
            s = np.sort(self.rows[j])[::-1]
            c["straddles 63/64"] += bool(len(s) > 64 and self.K >= 64 and s[63] == s[64])
            _, _, e = slot_table(self.ranges[q], np.r_[self.dev[j][self.dev[j] >= 0], m[:MAX_LEFT]].astype(np.int32),
                                 self.pool)
            c["NaN minimum"] += bool(np.isnan(e).any())
        return c


CLASSES = ("in-K keep", "in-K conservative", "in-K depends", "K-th keep", "K-th conservative", "K-th depends", "left out 0", "left out 1",
           "left out 7", "left out 8", "K-th >7 left out", "straddles 63/64", "K-th score 0", "NaN minimum")


@functools.lru_cache(maxsize=None)
def case(nd, K, rs=None, seed=None, emb_dim=16, q_offset=0):
    return Case(nd, K, RS_OF_ND[nd] if rs is None else rs, SEED_OF_ND[nd] if seed is None else seed, emb_dim,
                q_offset)


def can_hold(cls, nd, K):
    """The classes demanded of every (nd, K) shape, from the shape alone.  Equal scores inside the K beyond the copies
    of the query's own row need K ≥ 17; a K-th place tie needs domains left over (nd ≥ K + 8 asks for a few); with
    K = 1 the K-th score's group is the whole row, so nothing lies outside it and the rule always resolves (and any
    other member changes the match); a K-th place tie the rule keeps needs candidate rows free of the NaN and inf
    tiles, one domain each, which rows of more than half the table rarely are (nd ≥ 2K); positions 63 and 64 are the
    K-th and (K+1)-th at K = 64.  The other classes are demanded in total only."""
    if cls in ("in-K keep", "in-K depends"):
        return K >= 17
    if cls == "K-th keep":
        return K >= 2 and nd >= 2 * K and nd >= K + 8
    if cls == "K-th conservative":
        return K >= 2 and nd >= K + 8
    if cls == "K-th depends":
        return nd >= K + 8
    if cls == "straddles 63/64":
        return K == 64 and nd >= 65
    return False
