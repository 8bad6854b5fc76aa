"""Every scoring kernel at every BLAS thread count: the thread-split edge table of tests/split_edges.py through the
C ABI, against the numpy restatements that tests/test_split_edges_cpu.py pins to numpy's own product.

Each case is a table just large enough for OpenBLAS to split ``domain_embs @ q`` over T threads (28,800 rows of 16
floats, 14,400 of 32, and a few more; one row fewer: T must be ignored) whose tail columns — the columns the 4x2 and
4x1 sgemv kernels score — are bit copies of body rows that head some query's candidate row.  The expected candidate
rows therefore differ from those of a kernel that scored every column with the 4-column kernel, took the "whole tile
is kind 0" shortcut once too often, or split by another T (asserted per case on the CPU).

a. score rows: fwav_score_rows, fwav_score_rows_q, fwav_score_rows_dim — whole rows bit-equal to the restatement;
b. search at K = 8 and 64: the f32 kernel, the fp16 search, fwav_sim_topk_q, fwav_sim_topk_dim (and, for a few cases,
   every fp16 knob path of tests/test_gpu_tie_edges.py): candidate rows, order included, and the tie list;
c. K = 65, the large-K route;
d. the product sequence search → fwav_affine → tie check → fwav.ties.resolve_rows at T."""
import contextlib

import numpy as np
import pytest

import oracle_rows
import split_edges as SE
import test_gpu_tie_edges as GT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import ties as fties  # noqa: E402
from fwav._lib import call, debug_library, size_call  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

DEV = torch.device("cuda", 0)
I32 = np.int32
IDS = [SE.case_id(c) for c in SE.CASES]
td, stream = GT.td, GT.stream

_TABLES = {}


def table_of(key):
    if key not in _TABLES:
        _TABLES[key] = GT.Table(SE.case(*key).E)
    return _TABLES[key]


def active_list(c):
    """The queries in no order, with a gap (30 … 39 are not searched)."""
    ids = np.r_[0:30, 40:c.nq].astype(I32)
    return np.random.default_rng(c.nd + c.T).permutation(ids)


def search(key, K, active, kind, knobs=()):
    """One search of the queries `active` with blas_threads = the case's T.  kind: "f32" (emb16 = NULL), "f16", "q"
    (fwav_sim_topk_q, the table as its own query table) or "dim"; knobs: debug-library calls made first.
    → (cand i32[max_q, K], the tie list); untouched entries are −7."""
    c, tab = SE.case(*key), table_of(key)
    nd, mq, T = c.nd, c.max_q, c.T
    act, n_act = td(np.asarray(active, I32)), td(np.array([len(active)], I32))
    cand = torch.full((mq * K,), -7, dtype=torch.int32, device=DEV)
    tl = torch.full((size_call("fwav_tie_list_size", mq),), -7, dtype=torch.int32, device=DEV)
    with (debug_library() if knobs else contextlib.nullcontext()):
        for name, *args in knobs:
            call(name, *args)
        if kind == "dim":
            wk = size_call("fwav_sim_topk_dim_workspace_size", mq, nd, c.width, K)
        else:
            wk = size_call("fwav_sim_topk_workspace_size", mq, nd, K) if (kind != "f32" or K > 64) else 0
        ws = torch.zeros(max(wk, 16), dtype=torch.uint8, device=DEV)
        e16 = None if kind == "f32" else tab.e16.data_ptr()
        if kind == "dim":
            call("fwav_sim_topk_dim", tab.emb.data_ptr(), e16, nd, c.width, act.data_ptr(), n_act.data_ptr(), mq, 0, K, T,
                 cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, stream())
        elif kind == "q":
            call("fwav_sim_topk_q", tab.emb.data_ptr(), e16, nd, tab.emb.data_ptr(), e16, nd, 1, act.data_ptr(),
                 n_act.data_ptr(), mq, 0, K, T, cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, stream())
        else:
            call("fwav_sim_topk", tab.emb.data_ptr(), e16, nd, act.data_ptr(), n_act.data_ptr(), mq, 0, K, T,
                 cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, stream())
        torch.cuda.synchronize()
    return cand.cpu().numpy().reshape(mq, K), tl.cpu().numpy()


def check(key, K, kind, knobs=(), label=None):
    """Candidate rows equal the expectation, order included; rows of unlisted queries untouched; the tie list names
    exactly the expected queries with the expected flag; a record's members are −1 or the true ones (−1 at K > 64)."""
    c = SE.case(*key)
    active = active_list(c)
    cand, tl = search(key, K, active, kind, knobs)
    GT.check_search(c.view(K), active, cand, tl, None, False, (SE.case_id(key), K, label or kind), never=K > 64)


# ------------------------------------------------------------------------------------------------ a. score rows
@pytest.mark.parametrize("key", SE.CASES, ids=IDS)
def test_score_rows(key):
    c, tab = SE.case(*key), table_of(key)
    nd, T = c.nd, c.T
    entries = ("fwav_score_rows", "fwav_score_rows_q") if c.width == 16 else ("fwav_score_rows_dim",)
    for q_offset in (0, SE.Q_OFFSET):
        rows = np.array(c.full_q, I32) - q_offset
        assert (rows >= 0).all()
        r = td(rows)
        for entry in entries:
            S = torch.full((len(rows) * nd,), float("nan"), dtype=torch.float32, device=DEV)
            if entry == "fwav_score_rows":
                call(entry, tab.emb.data_ptr(), nd, r.data_ptr(), len(rows), q_offset, T, S.data_ptr(), stream())
            elif entry == "fwav_score_rows_q":
                call(entry, tab.emb.data_ptr(), nd, tab.emb.data_ptr(), r.data_ptr(), len(rows), q_offset, T,
                     S.data_ptr(), stream())
            else:
                call(entry, tab.emb.data_ptr(), nd, c.width, r.data_ptr(), len(rows), q_offset, T, S.data_ptr(),
                     stream())
            torch.cuda.synchronize()
            S = S.cpu().numpy().reshape(len(rows), nd)
            for j, q in enumerate(c.full_q):
                bad = np.flatnonzero(S[j].view(np.uint32) != c.full[q].view(np.uint32))
                assert bad.size == 0, (SE.case_id(key), entry, q_offset, q, bad[:8], c.kind[bad[:8]])


# ------------------------------------------------------------------------------------------------ b. search
@pytest.mark.parametrize("key", SE.CASES, ids=IDS)
def test_search(key):
    for K in (8, 64):
        for kind in (("f32", "f16", "q") if key[0] == 16 else ("dim",)):
            check(key, K, kind)


@pytest.mark.parametrize("key", SE.KNOB_CASES, ids=[SE.case_id(c) for c in SE.KNOB_CASES])
def test_search_fp16_knob_paths(key):
    """Modes 0/1 × geometries 0–3, the split plans and the forced floors, through the debug library."""
    for K in (8, 64):
        for label, kind, knobs in GT.f16_paths(SE.case(*key).view(K)):
            if knobs:
                check(key, K, kind, knobs, label)


# ------------------------------------------------------------------------------------------------ c. K = 65
@pytest.mark.parametrize("key", SE.CASES, ids=IDS)
def test_large_k(key):
    check(key, 65, "f16" if key[0] == 16 else "dim")


# ------------------------------------------------------------------------------------------------ d. product
@pytest.mark.parametrize("exact_sets", [0, 2])
@pytest.mark.parametrize("key", SE.PRODUCT_CASES, ids=[SE.case_id(c) for c in SE.PRODUCT_CASES])
def test_product_sequence(key, exact_sets):
    """search → fwav_affine → fwav_tie_check[_dim] → fwav.ties.resolve_rows(threads=T).  Width 16: oracle_rows.check_rows
    at T (rows without a tie and resolved rows are the oracle's, order included; every match tuple is O.affine of the
    oracle's row).  Width 32: resolved rows are numpy's ranking of the restated score row, the others the expected
    rows, and every match tuple is O.affine of numpy's row."""
    c, tab = SE.case(*key), table_of(key)
    nd, mq, T, K, rs, W = c.nd, c.max_q, c.T, SE.K_COVER, 8, c.width
    rng = np.random.default_rng(11 + nd)
    ranges_np = rng.normal(0, 0.3, (mq, rs)).astype(np.float32)
    pool_np = rng.normal(0, 0.3, (nd, rs)).astype(np.float32)
    # a copy's tile is its source's, and every other range is an affine image of its source's tile: the source and its
    # copies then attain the minimum error together, and whether numpy's order matters depends on which of them share
    # a score — on the sgemv kernel of each, which the tie check has to restate too
    for j, col in enumerate(c.tail):
        pool_np[col] = pool_np[c.src_of_q[j % c.nq]]
    ranges_np[0::2] = 2 * pool_np[c.src_of_q[0::2]] + np.float32(0.25)
    ranges, pool = td(ranges_np.reshape(-1)), td(pool_np.reshape(-1))
    act, n_act = td(c.ids), td(np.array([mq], I32))
    cand = torch.full((mq * K,), -1, dtype=torch.int32, device=DEV)
    tl = torch.empty(size_call("fwav_tie_list_size", mq), dtype=torch.int32, device=DEV)
    st = stream()
    if W == 16:
        wk = size_call("fwav_sim_topk_workspace_size", mq, nd, K)
        ws = torch.zeros(max(wk, 16), dtype=torch.uint8, device=DEV)
        call("fwav_sim_topk", tab.emb.data_ptr(), tab.e16.data_ptr(), nd, act.data_ptr(), n_act.data_ptr(), mq, 0, K, T,
             cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, st)
    else:
        call("fwav_sim_topk_dim", tab.emb.data_ptr(), tab.e16.data_ptr(), nd, W, act.data_ptr(), n_act.data_ptr(), mq, 0,
             K, T, cand.data_ptr(), tl.data_ptr(), None, 0, st)
    outs = [torch.empty(mq, dtype=dt, device=DEV) for dt in (torch.int32, torch.float32, torch.float32, torch.uint8,
                                                            torch.float32)]
    call("fwav_affine", ranges.data_ptr(), mq, rs, cand.data_ptr(), K, pool.data_ptr(), nd, 16.0,
         *[t.data_ptr() for t in outs], st)
    resolve = torch.empty(mq + 1, dtype=torch.int32, device=DEV)
    if W == 16:
        call("fwav_tie_check", ranges.data_ptr(), mq, rs, cand.data_ptr(), K, pool.data_ptr(), nd, tab.emb.data_ptr(), 0,
             T, tl.data_ptr(), mq, exact_sets, resolve.data_ptr(), st)
    else:
        call("fwav_tie_check_dim", ranges.data_ptr(), mq, rs, cand.data_ptr(), K, pool.data_ptr(), nd,
             tab.emb.data_ptr(), W, 0, T, tl.data_ptr(), mq, exact_sets, resolve.data_ptr(), st)
    n = int(resolve[0].item())
    fties.resolve_rows(resolve[1:1 + n], emb=tab.emb, n_domains=nd, q_offset=0, k=K, threads=T, ranges=ranges,
                       range_size=rs, pool=pool, s_clip=16.0, cand=cand, outs=tuple(outs), stream=st, emb_dim=W)
    torch.cuda.synchronize()
    resolved = resolve[1:1 + n].cpu().tolist()
    cand_np = cand.cpu().numpy().reshape(mq, K)
    outs_np = [t.cpu().numpy() for t in outs]
    listed = set(c.exp(K))
    assert set(resolved) <= listed and len(set(resolved)) == n
    if exact_sets == 2:
        assert set(resolved) == listed
    print(f"\n{SE.case_id(key)} exact_sets {exact_sets}: listed {len(listed)}, resolved {n}")
    if W == 16:
        st_ = oracle_rows.check_rows(c.E, pool_np, ranges_np, cand_np, outs_np, c.ids, K, threads=T, exact=resolved,
                                     label=f"{SE.case_id(key)} exact_sets {exact_sets}")
        assert st_["tied"] == len(listed)
        return
    S = SE.scores(W, c.E, c.E[:mq], c.kind)
    npy = np.stack([O.numpy_topk_row(S[q], K) for q in range(mq)])
    for q in range(mq):
        want = npy[q] if q in resolved else c.rows(K)[q]
        assert np.array_equal(cand_np[q], want), (SE.case_id(key), exact_sets, q, cand_np[q], want)
        if q not in listed:
            assert np.array_equal(npy[q], c.rows(K)[q])
    want = O.affine(ranges_np, npy, pool_np)
    for nm, got, ref in zip(("idx", "s", "o", "sym", "err"), outs_np, want):
        assert np.array_equal(got.view(np.uint8), np.asarray(ref).astype(got.dtype).view(np.uint8)), \
            (SE.case_id(key), exact_sets, nm)
