"""The inputs and restatements of the tie edge tests (tests/tie_edges.py), checked on the CPU before the device is
compared with them (tests/test_gpu_tie_edges.py):

* the dyadic tables' score rows are exact — numpy's ``t @ t[i]`` equals the float64 product bit for bit at any BLAS
  thread count — so ties are the same in every summation order;
* every class of tie the device code distinguishes occurs, often enough, over the GPU test's shapes;
* the restated rule is sound: it resolves every query whose match truly depends on the order of equal scores;
* the admissible-row model describes numpy itself: numpy's own row is admissible, and where the match does not depend
  on the order numpy's row gives the device-order row's tuple."""
import numpy as np
import pytest

import tie_edges as TE
from oracle import fractal_oracle as O

SHAPES = [(nd, K) for nd in TE.ND_ALL for K in TE.K_ALL]
TOTAL_MIN = 8
TOTAL_CLASSES = ("in-K keep", "in-K depends", "K-th keep", "K-th conservative", "K-th depends", "left out 0",
                 "left out 7", "left out 8", "straddles 63/64", "K-th score 0", "NaN minimum")


def _tables():
    for nd in TE.ND_ALL:
        yield f"nd{nd}", TE.table(nd, TE.SEED_OF_ND[nd])
    yield "nd257 wide", TE.table(257, TE.SEED_OF_ND[257], 32)
    yield "overflow", TE.overflow_table()


def test_tables_keep_the_search_contract():
    """Finite rows, entries on the 1/16 grid, both heads of norm ≤ 1, zero rows and copies present."""
    for name, t in _tables():
        h = t.shape[1] // 2
        assert np.isfinite(t).all() and np.array_equal(t * 16, np.round(t * 16)) and np.abs(t).max() <= 6 / 16, name
        for head in (t[:, :h], t[:, h:]):
            assert (head.astype(np.float64) ** 2).sum(1).max() <= 1, name
        assert not t[0].any() and (len(t) <= 41 or name == "overflow" or np.array_equal(t[41], t[5])), name
        assert np.array_equal(t.astype(np.float16).astype(np.float32), t), name  # the fp16 low part is zero


def test_scores_are_exact_in_any_order():
    threadpoolctl = pytest.importorskip("threadpoolctl")
    for name, t in _tables():
        rows = np.arange(min(TE.MAX_Q, len(t)))
        want = t.astype(np.float64) @ t[rows].astype(np.float64).T  # exact: multiples of 1/256 below 2^24/256
        assert np.array_equal(want * 256, np.round(want * 256))
        for T in (1, 2, 5, 16):
            with threadpoolctl.threadpool_limits(T, user_api="blas"):
                got = TE.score_rows(t, rows)
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want.T), (name, T)
        if t.shape[1] == 16:  # ... and in each of the device's three sgemv orders
            for kind in (0, 1, 2):
                got = O.sgemv_scores(t, t[rows], np.full(len(t), kind, np.int8))
                assert np.array_equal(got.astype(np.float64), want.T), (name, kind)


def test_class_coverage():
    """A condition on the inputs, not a measurement: every class holds at least TOTAL_MIN queries over the shape list,
    and every shape holds every class it can (TE.can_hold)."""
    total = dict.fromkeys(TE.CLASSES, 0)
    print("\n%-8s %s" % ("nd,K", " ".join("%7s" % c.replace("left out", "out").replace("K-th ", "K:")[:7]
                                         for c in TE.CLASSES)))
    missing = []
    for nd, K in SHAPES:
        c = TE.case(nd, K).classes()
        print("%-8s %s" % (f"{nd},{K}", " ".join("%7d" % c[k] for k in TE.CLASSES)))
        for k in TE.CLASSES:
            total[k] += c[k]
            if TE.can_hold(k, nd, K) and c[k] == 0:
                missing.append((k, nd, K))
    print("total    %s" % " ".join("%7d" % total[k] for k in TE.CLASSES))
    print("class totals:", total)
    assert not missing, missing
    assert all(total[k] >= TOTAL_MIN for k in TOTAL_CLASSES), total
    # the in-K rule is exact on these inputs: whenever it resolves, some admissible order changes the match
    assert total["in-K conservative"] == 0


@pytest.mark.parametrize("nd", TE.ND_ALL)
def test_rule_is_sound_and_numpy_is_admissible(nd):
    """Per listed query: depends_rule ⊇ truly_depends.  Per query, listed or not: numpy's own row is admissible
    (the same members outside the K-th score's group, runs only permuted), and where the match does not truly depend
    on the order its O.affine tuple is the device-order row's.  The slot-table shortcut behind truly_depends equals
    O.affine on whole candidate rows."""
    for K in TE.K_ALL:
        c = TE.case(nd, K)
        npy = np.stack([O.numpy_topk_row(r, K) for r in c.rows])
        with np.errstate(all="ignore"):
            t_np = TE._tuple_bytes(*O.affine(c.ranges[c.ids], npy, c.pool))
            t_dev = TE._tuple_bytes(*O.affine(c.ranges[c.ids], c.dev, c.pool))
        for j, q in enumerate(c.ids.tolist()):
            assert TE.is_admissible(npy[j], c.rows[j], K), (nd, K, q)
            assert TE.is_admissible(c.dev[j], c.rows[j], K), (nd, K, q)
            if q in c.exp:
                assert c.rule[q] or not c.truly[q], (nd, K, q)
                if not c.truly[q]:
                    assert t_np[j].tobytes() == t_dev[j].tobytes(), (nd, K, q)
            else:
                assert np.array_equal(npy[j], c.dev[j]), (nd, K, q)  # no tie in the top K + 1: one admissible row
                assert TE.n_admissible(c.rows[j], K) == 1
            short = TE.tuples_of_rows(c.ranges[q], np.stack([c.dev[j], npy[j]]), c.pool)
            assert short[0].tobytes() == t_dev[j].tobytes() and short[1].tobytes() == t_np[j].tobytes(), (nd, K, q)


def test_admissible_rows_enumerates_and_targets():
    """A hand-made score row: runs of 2 and 3 above a K-th score group of 4 with 2 places: 2!·3!·P(4,2) = 144 rows,
    all distinct, all admissible, the device-order row among them; a row with too many for enumeration gets every
    member of every run first and every group member both in and out."""
    s = np.array([9, 7, 7, 5, 5, 5, 3, 3, 3, 3, 1], np.float32)[::-1].copy()
    K = 8
    dev, var, full = TE.admissible_rows(s, K)
    assert full and len(var) == 144 == TE.n_admissible(s, K) and len({v.tobytes() for v in var}) == 144
    assert dev.tobytes() in {v.tobytes() for v in var} and all(TE.is_admissible(v, s, K) for v in var)
    assert not TE.is_admissible(np.r_[dev[1], dev[0], dev[2:]].astype(np.int32), s, K)  # 9 and 7 swapped
    big = np.r_[np.full(9, 2.0), np.full(12, 1.0), 0.0].astype(np.float32)
    K = 14
    dev, var, full = TE.admissible_rows(big, K)
    assert not full and all(TE.is_admissible(v, big, K) for v in var)
    assert {int(v[0]) for v in var} == set(range(9))
    grp = set(range(9, 21))
    assert all(any(g in v[9:] for v in var) and any(g not in v[9:] for v in var) for g in grp)
    # nd ≤ K: a full argsort, every run only permuted, −1 padded
    small = np.array([1, 1, 0, 2], np.float32)
    dev, var, full = TE.admissible_rows(small, 6)
    assert full and len(var) == 2 and (var[:, 4:] == -1).all() and dev.tolist() == [3, 0, 1, 2, -1, -1]


def test_expected_list_and_rule_by_hand():
    """Hand-checked records and decisions on a six-domain table."""
    s = np.array([[5, 4, 4, 3, 3, 3]], np.float32)
    assert TE.expected_list(s, 1) == {}
    e = TE.expected_list(s, 2)
    assert e[0][0] == 1 and e[0][1] == 1 and e[0][2].tolist() == [2]
    e = TE.expected_list(s, 3)
    assert e[0][:2] == (0, 0)
    e = TE.expected_list(s, 4, ids=[7])
    assert e[7][0] == 1 and e[7][2].tolist() == [4, 5]
    assert TE.expected_list(s, 6)[0][:2] == (0, 0) and TE.expected_list(s, 9)[0][:2] == (0, 0)
    t = TE.list_array(e, 9)
    assert t[0] == 1 and t[1:5].tolist() == [15, 2, 4, 5] and TE.parse_list(t)[0][:3] == (7, 1, 2)
    assert TE.list_array(e, 9, "reversed")[3:5].tolist() == [5, 4] and TE.list_array(e, 9, "uncollected")[2] == -1
    # pool: domains 1 and 2 (one run) hold the same tile, which fits the range exactly; domain 0 does not
    pool = np.array([[0, 1, 0, 0], [1, 2, 3, 5], [1, 2, 3, 5], [0, 0, 1, 0], [2, 0, 0, 1], [0, 3, 0, 0]], np.float32)
    r = np.array([1, 2, 3, 5], np.float32)
    none = np.zeros(0, np.int32)
    row3 = TE.device_row(s[0], 3)
    assert TE.depends_rule(s[0], 3, row3, 0, 0, none, r, pool) and TE.truly_depends(s[0], 3, r, pool)
    r2 = pool[0] * 2 + 1  # domain 0 alone fits exactly: the run of 1 and 2 cannot change the match
    assert not TE.depends_rule(s[0], 3, row3, 0, 0, none, r2, pool) and not TE.truly_depends(s[0], 3, r2, pool)
    # K = 2: the K-th place group is {1, 2}; with range r the group holds the minimum → resolve, and it truly depends
    row2 = TE.device_row(s[0], 2)
    assert TE.depends_rule(s[0], 2, row2, 1, 1, np.array([2], np.int32), r, pool) and TE.truly_depends(s[0], 2, r, pool)
    assert not TE.depends_rule(s[0], 2, row2, 1, 1, np.array([2], np.int32), r2, pool)
    assert not TE.truly_depends(s[0], 2, r2, pool)
    for mode, flag, cnt in ((0, 1, -1), (1, 1, 1), (2, 0, 0)):  # uncollected group; exact_sets 1 and 2
        assert TE.depends_rule(s[0], 2, row2, flag, cnt, np.array([2], np.int32), r2, pool, exact_sets=mode)
    assert TE.depends_rule(s[0], 65, TE.device_row(s[0], 65), 0, 0, none, r2, pool)
