"""The thread-split edge table (tests/split_edges.py) without a GPU: the restatement against numpy's own product
at every thread count of the grid, and the coverage conditions that keep tests/test_gpu_split_edges.py from passing
vacuously — every tail column stands in some query's top K, its score under its own sgemv kernel differs in bits from
its kind-0 score, and the expected candidate rows differ from those of an all-kind-0 kernel and from those of the
one-thread split."""
import numpy as np
import pytest

import split_edges as SE
from oracle import fractal_oracle as O

IDS = [SE.case_id(c) for c in SE.CASES]
BAR = 3  # candidate rows (of SE.NQ, at K = SE.K_COVER) that must differ from each wrong ranking


def has_tail(c):
    return len(c.tail) > 0


@pytest.mark.parametrize("key", SE.CASES, ids=IDS)
def test_restatement_is_numpys_product(key):
    """``E @ q`` under threadpool_limits(T) equals the restated score row on every column, for the case's kept rows;
    and the kept part of every fourth query's row (what the expected candidates are cut from) is numpy's too."""
    threadpoolctl = pytest.importorskip("threadpoolctl")
    width, nd, T = key
    c = SE.case(*key)
    assert len(c.full_q) >= 8 and min(c.full_q) >= SE.Q_OFFSET
    with threadpoolctl.threadpool_limits(T, user_api="blas"):
        assert O.blas_threads() == T
        for q in c.full_q:
            ref = c.E @ c.E[q]
            bad = np.flatnonzero(ref.view(np.uint32) != c.full[q].view(np.uint32))
            assert bad.size == 0, (key, q, bad[:8], c.kind[bad[:8]])
        for q in range(0, c.nq, 4):
            sel, s = c.top[q]
            ref = c.E @ c.E[q]
            assert np.array_equal(ref[sel].view(np.uint32), s.view(np.uint32)), (key, q)
            assert (np.delete(ref, sel) < s.min()).all(), (key, q)


@pytest.mark.parametrize("key", SE.CASES, ids=IDS)
def test_coverage_of_each_case(key):
    width, nd, T = key
    c = SE.case(*key)
    K = SE.K_COVER
    rows = c.rows(K)
    d0 = int((rows != c.rows_kind0).any(axis=1).sum())
    d1 = int((rows != c.rows_one_thread).any(axis=1).sum())
    in_top = np.isin(c.tail, rows)
    print(f"\n{SE.case_id(key)}: tail columns {len(c.tail)} (kind 1: {int((c.kind == 1).sum())}, kind 2: "
          f"{int((c.kind == 2).sum())}), sources {len(set(c.src_of_q.tolist()))}; in some top {K}: {int(in_top.sum())}; "
          f"bits differ from kind 0: {int(c.tail_bits_differ.sum())} (in the {len(c.full_q)} kept rows: {int(c.full_bits_differ.sum())}); rows of {c.nq} that differ from all-kind-0: {d0}, "
          f"from the one-thread split: {d1}; listed ties at K = {K}: {len(c.exp(K))}")
    # the table's contract: its source and the source's copies head each candidate row, then the query itself
    assert (c.tail >= c.nq).all()  # (no tail column of this grid replaces a query)
    for q in range(c.nq):
        group = {int(c.src_of_q[q])} | {int(col) for j, col in enumerate(c.tail)
                                        if c.src_of_q[j % c.nq] == c.src_of_q[q]}
        assert rows[q, len(group)] == q and set(rows[q, :len(group)].tolist()) == group, (key, q)
    if not has_tail(c):
        assert np.array_equal(rows, c.rows_kind0)
        return
    assert in_top.all(), (key, c.tail[~in_top])
    assert c.tail_bits_differ.all(), (key, c.tail[~c.tail_bits_differ])
    # ... and in one of the whole rows the score-row tests compare
    assert c.full_bits_differ.all(), (key, c.tail[~c.full_bits_differ])
    assert d0 >= BAR, (key, d0)
    if not np.array_equal(c.kind, c.kind1):
        assert d1 >= BAR, (key, d1)


def test_coverage_of_the_grid():
    """Per width: chunk-width residues 0 … 3 among the "one wider" chunks and among the regular ones, kinds 1 and 2,
    and the control without a tail."""
    for width in (16, 32):
        wide, regular, kinds = set(), set(), set()
        for w, nd, T in SE.CASES:
            if w != width:
                continue
            a, b = SE.chunk_widths(w, nd, T)
            if a is not None:
                wide.add(a % 4)
            regular.add(b % 4)
            kinds |= set(np.unique(SE.kinds_of(w, nd, T)).tolist())
        print(f"\nwidth {width}: residues of the wider chunks {sorted(wide)}, of the regular ones {sorted(regular)}, "
              f"kinds {sorted(kinds)}")
        assert wide == {0, 1, 2, 3} and regular == {0, 1, 2, 3} and kinds == {0, 1, 2}, (width, wide, regular, kinds)
        assert SE.CONTROL[width] in SE.CASES and not SE.kinds_of(*SE.CONTROL[width]).any()
    # the subsets that run the knob paths and the product sequence keep a control and, per width, both tail kinds
    for sub in (SE.KNOB_CASES, SE.PRODUCT_CASES):
        assert set(sub) <= set(SE.CASES)
        for width in {k[0] for k in sub}:
            kinds = set()
            for k in sub:
                if k[0] == width:
                    kinds |= set(np.unique(SE.kinds_of(*k)).tolist())
            assert kinds == {0, 1, 2} and SE.CONTROL[width] in sub


@pytest.mark.parametrize("width, nd", [(16, 28799), (32, 14399)])
def test_no_leak_below_the_threshold(width, nd):
    """Below emb_dim·n_domains = 460,800 the expectation ignores T: the table, the kinds and the rows are those of
    one thread."""
    a, b = SE.case(width, nd, 1), SE.case(width, nd, 16)
    assert width * nd < SE.THREAD_MIN_MN <= width * (nd + 1)
    assert np.array_equal(a.E.view(np.uint32), b.E.view(np.uint32)) and np.array_equal(a.kind, b.kind)
    assert np.array_equal(b.kind, b.kind1)
    for K in SE.K_ALL:
        assert np.array_equal(a.rows(K), b.rows(K)) and np.array_equal(b.rows(SE.K_COVER), b.rows_one_thread)
        assert a.exp(K).keys() == b.exp(K).keys()
    assert a.full_q == b.full_q
    for q in a.full_q:
        assert np.array_equal(a.full[q].view(np.uint32), b.full[q].view(np.uint32))
    # ... and one row above it does not: the split of 16 threads is another
    assert not np.array_equal(SE.kinds_of(width, nd + 2, 16), SE.kinds_of(width, nd + 2, 1))
