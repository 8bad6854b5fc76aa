"""The search's tie list (record_tie / tie_flags, fwav_topk_keys.h) and the tie check (k_tie_check, fwav_affine.hip)
against the plain numpy restatements of tests/tie_edges.py, through the C ABI and the debug library's knobs.

Inputs: dyadic embedding tables (entries k/16: every score exact in any order, ties plentiful and the same for numpy,
the f32 kernels and the fp16 pre-filter) of 40, 64, 65, 257 and 600 rows, up to 129 queries, K ∈ {1, 2, 17, 32, 63, 64}
(K = 64: the K-th score in lane 63, the (K+1)-th in the next slot; nd = K, K + 1, < K), pools of a few distinct coarse
rows.  tests/test_tie_edges_cpu.py asserts that every class of tie occurs in them and that the restated rule is sound.

a. every search path: the candidates are the (score desc, index asc) contract, the list holds each expected query once
   with the expected flag, a K-th place record carries −1 or the true left-out members in index order (above 7: −1).
   A −1 must not hide a group that should have been collected: on the fp16 paths (whose final pass sorts a complete
   band: emit with tv == 0 in S16/HL mode, k_merge_pieces) every K-th place record of at most 7 left-out members
   carries them, except for the queries the search itself lists for its exact-mode relaunch (read back from the
   workspace's overflow lists through fwav_debug_sim_topk_layout: exact mode keeps only the top K, so a tied domain
   it dropped leaves the group unknown).  No final band of these tables is near the buffer's 192 entries, but a
   running one can be: a query with one or two non-zeros scores exactly 0 against most of the first chunk, so its
   first compaction, taken while the running K-th score is still 0, keeps more than 192 zeros — a dozen such queries
   of the 600-row table overflow on every path.  The f32 kernel and the wide (_dim) search do not collect today (−1 or the true members are
   both accepted); K > 64 must write −1.
b. fwav_tie_check / _q / _dim fed hand-built lists (no search): the resolve set equals depends_rule exactly and
   contains truly_depends, for the templated (rs 4, 8, 16) and runtime (rs 5, 19) kernels, widths 16 and 32,
   exact_sets 0 / 1 / 2, records with the members, with −1, and with the members reversed.
c. the product sequence search → fwav_affine → tie check → fwav.ties.resolve_rows under each tie_order."""
import contextlib

import numpy as np
import pytest

import affine_edges as AE
import tie_edges as TE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import ties as fties  # noqa: E402
from fwav._lib import call, debug_lib, debug_library, sim_topk_layout, size_call  # noqa: E402
from fwav.stages import TIE_MODES  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

DEV = torch.device("cuda", 0)
I32 = np.int32


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


class Table:
    """An embedding table on the device with its fp16 search tables."""

    def __init__(self, t):
        self.nd, self.dim = t.shape
        self.emb = td(t.reshape(-1))
        if self.dim == 16:
            self.e16 = torch.empty(size_call("fwav_emb16_elems", self.nd), dtype=torch.float16, device=DEV)
            call("fwav_emb16_from_emb", self.emb.data_ptr(), self.nd, self.e16.data_ptr(), stream())
        else:
            self.e16 = torch.empty(size_call("fwav_embh_elems", self.nd, self.dim), dtype=torch.float16, device=DEV)
            call("fwav_embh_from_emb", self.emb.data_ptr(), self.nd, self.dim, self.e16.data_ptr(), stream())
        torch.cuda.synchronize()


_TABLES = {}


def table_of(c):
    key = (c.nd, c.emb_dim, c.t.tobytes())
    if key not in _TABLES:
        _TABLES[key] = Table(c.t)
    return _TABLES[key]


def search(c, active, kind="f16", knobs=(), fill=-7):
    """One search of the local queries `active` of case c.  kind: "f32" (emb16 = NULL), "f16", "q" (fwav_sim_topk_q
    with the table as its own query table) or "dim"; knobs: debug-library calls made first (inside debug_library()).
    → (cand i32[max_q, K], the tie list, the queries the fp16 search listed for its exact-mode relaunch or None)."""
    tab = table_of(c)
    nd, K, mq, T = c.nd, c.K, c.max_q, O.blas_threads()
    act = td(np.asarray(active, I32))
    n_act = td(np.array([len(active)], I32))
    cand = torch.full((mq * K,), fill, dtype=torch.int32, device=DEV)
    tl = torch.full((size_call("fwav_tie_list_size", mq),), -7, dtype=torch.int32, device=DEV)
    exact = None
    with (debug_library() if knobs else contextlib.nullcontext()):
        for name, *args in knobs:
            call(name, *args)
        if kind == "dim":
            wk = size_call("fwav_sim_topk_dim_workspace_size", mq, nd, c.emb_dim, K)
        else:
            wk = size_call("fwav_sim_topk_workspace_size", mq, nd, K) if (kind != "f32" or K > 64) else 0
        ws = torch.zeros(max(wk, 16), dtype=torch.uint8, device=DEV)
        e16 = None if kind == "f32" else tab.e16.data_ptr()
        if kind == "dim":
            call("fwav_sim_topk_dim", tab.emb.data_ptr(), e16, nd, c.emb_dim, act.data_ptr(), n_act.data_ptr(), mq,
                 c.q_offset, K, T, cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, stream())
        elif kind == "q":
            call("fwav_sim_topk_q", tab.emb.data_ptr(), e16, nd, tab.emb.data_ptr(), e16, nd, 1, act.data_ptr(),
                 n_act.data_ptr(), mq, c.q_offset, K, T, cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, stream())
        else:
            call("fwav_sim_topk", tab.emb.data_ptr(), e16, nd, act.data_ptr(), n_act.data_ptr(), mq, c.q_offset, K, T,
                 cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, stream())
        torch.cuda.synchronize()
        if kind in ("f16", "q") and K <= 64:
            # the queries of the exact-mode relaunch: after an S16 first pass the HL relaunch's overflow list, after an
            # HL first pass the first pass's own (fwav_topk.hip launch_topk)
            lay = sim_topk_layout(mq, nd)
            info, blocks = (np.zeros(3, I32), np.zeros(3, np.int64))
            assert debug_lib().fwav_debug_topk_plan_info(mq, nd, info.ctypes.data, blocks.ctypes.data) == 0
            lst, cnt = ("ovf2", "n_ovf2") if info[1] == 0 else ("ovf1", "n_ovf1")
            tail = ws[lay["ovf2"]:lay["miss"]].cpu().numpy()
            base = lay["ovf2"]
            n = int(tail[lay[cnt] - base:lay[cnt] - base + 4].view(I32)[0])
            assert 0 <= n <= mq
            exact = set(tail[lay[lst] - base:lay[lst] - base + 4 * n].view(I32).tolist())
    return cand.cpu().numpy().reshape(mq, K), tl.cpu().numpy(), exact


def check_search(c, active, cand, tl, exact, collects, label, never=False):
    """The contract of one search's outputs; → (K-th place records, with the members, with −1, −1 in exact mode)."""
    active = [int(q) for q in active]
    for q in active:
        assert np.array_equal(cand[q], c.dev[c.row_of[q]]), (label, "cand", q, cand[q], c.dev[c.row_of[q]])
    rest = np.setdiff1d(np.arange(c.max_q), active)
    assert (cand[rest] == -7).all(), (label, "rows of unlisted queries written")
    recs = TE.parse_list(tl)
    want = {q: c.exp[q] for q in active if q in c.exp}
    got = [r[0] for r in recs]
    assert len(set(got)) == len(got), (label, "a query listed twice")
    assert set(got) == set(want), (label, "listed", sorted(set(got) ^ set(want))[:10])
    n_kth = n_full = n_minus = n_exact = 0
    for q, flag, cnt, mem in recs:
        wf, wn, wm = want[q]
        assert flag == wf, (label, "flag", q, flag, wf)
        if never:  # the large-K route writes −1 into every record
            assert cnt == -1, (label, "count", q, cnt)
        if not flag:
            continue
        n_kth += 1
        if cnt == -1:
            n_minus += 1
            in_exact = exact is not None and q in exact
            n_exact += in_exact
            if collects and wn <= TE.MAX_LEFT:
                assert in_exact, (label, "group of", wn, "not collected for query", q)
        else:
            assert not never, (label, "this path never collects", q, cnt)
            assert cnt == wn <= TE.MAX_LEFT, (label, "count", q, cnt, wn)
            assert np.array_equal(mem[:cnt], wm), (label, "members", q, mem, wm)
            n_full += 1
    return np.array([n_kth, n_full, n_minus, n_exact])


def kth_scores(c):
    kk = min(c.K, c.nd)
    return np.array([c.rows[j][c.dev[j][kk - 1]] for j in range(len(c.ids))], np.float64)


def f16_paths(c):
    """(label, kind, knobs) of every fp16 search path."""
    kth = kth_scores(c)
    out = [("f16 auto", "f16", ()), ("f16 _q", "q", ())]
    for mode in (0, 1):
        for geo in (0, 1, 2, 3):
            out.append((f"mode {mode} geometry {geo}", "f16",
                        (("fwav_debug_topk_mode", mode), ("fwav_debug_topk_geometry", geo))))
    for plan in ((1 << 20, 2), (1 << 20, 8), (10, 3), (1 << 20, -1)):
        out.append((f"plan {plan}", "f16", (("fwav_debug_topk_plan", *plan),)))
    for fm in (1, 3):
        for name, v in (("below", -10.0), ("median", float(np.median(kth))), ("above", 10.0)):
            out.append((f"floor {fm} {name}", "f16", (("fwav_debug_topk_floor", fm, v),)))
    return out


def report(title, stats):
    print(f"\n{title}: K-th place records / with members / -1 / -1 in the exact-mode relaunch")
    for label, s in stats.items():
        print(f"  {label:24s} {int(s[0]):6d} {int(s[1]):6d} {int(s[2]):6d} {int(s[3]):6d}")


# ------------------------------------------------------------------------------------ a. the tie list
@pytest.mark.parametrize("nd", TE.ND_ALL)
def test_tie_list_every_search_path(nd):
    stats = {}

    def add(label, s):
        stats[label] = stats.get(label, 0) + s

    for K in TE.K_ALL:
        c = TE.case(nd, K)
        cand, tl, _ = search(c, c.ids, "f32")
        add("f32", check_search(c, c.ids, cand, tl, None, False, (nd, K, "f32")))
        for label, kind, knobs in f16_paths(c):
            cand, tl, exact = search(c, c.ids, kind, knobs)
            add(label, check_search(c, c.ids, cand, tl, exact, True, (nd, K, label)))
    c = TE.Case(nd, 65, TE.RS_OF_ND[nd], TE.SEED_OF_ND[nd], decisions=False)  # the large-K route: nothing collected
    cand, tl, _ = search(c, c.ids, "f16")
    add("K = 65", check_search(c, c.ids, cand, tl, None, False, (nd, 65), never=True))
    report(f"nd = {nd}", stats)


def test_tie_list_q_offset_and_sparse_active_list():
    """Queries 100 … 228 of the 257-row table (q_offset = 100), and a sparse active list in no order: only the listed
    queries' rows are written, and the list names only them."""
    stats = {}
    c = TE.case(257, 32, q_offset=100)
    assert c.q_offset == 100 and c.max_q == 129 and len(c.exp) > 50
    rng = np.random.default_rng(5)
    sparse = rng.permutation(c.ids[::3])
    for label, kind, knobs in [("f32", "f32", ())] + f16_paths(c):
        for name, active in (("offset", c.ids), ("sparse", sparse)):
            cand, tl, exact = search(c, active, kind, knobs)
            s = check_search(c, active, cand, tl, exact, kind != "f32", (label, name))
            stats[f"{label} {name}"] = s
    report("q_offset 100 / sparse", stats)


def test_tie_list_wide_search():
    """fwav_sim_topk_dim at width 32 (two heads of 16): candidates, flags, and −1 or the members for a K-th place
    record (−1 at K = 65)."""
    stats = {}
    for K in TE.K_ALL + (65,):
        c = TE.Case(257, K, 8, TE.SEED_OF_ND[257], emb_dim=32, decisions=False)
        cand, tl, _ = search(c, c.ids, "dim")
        stats[f"K = {K}"] = check_search(c, c.ids, cand, tl, None, False, ("dim", K), never=K > 64)
        assert K == 1 or len(c.exp) > 20
    report("width 32", stats)


def test_tie_list_overflowing_band():
    """600 rows of which 250 are one row: its queries' bands overflow, so the exact-mode relaunch serves them and −1
    is expected there.  Candidates, flags and "the count or −1" still hold on every path."""
    stats = {}
    tab = TE.overflow_table()
    for K in (32, 64):
        c = TE.Case(600, K, 19, 0, tab=tab, decisions=False)
        cand, tl, _ = search(c, c.ids, "f32")
        stats[f"K {K} f32"] = check_search(c, c.ids, cand, tl, None, False, (K, "f32"))
        for label, kind, knobs in f16_paths(c):
            cand, tl, exact = search(c, c.ids, kind, knobs)
            stats[f"K {K} {label}"] = check_search(c, c.ids, cand, tl, exact, True, (K, label))
            # an unsplit first pass holds a query's whole band in one buffer: 250 equal scores do not fit.  (Table
            # pieces — the plans, and the floor's second pass — hold a share each, and their union of 250 fits the merge.)
            copies = [int(q) for q in c.ids if np.array_equal(tab[q], tab[1])]
            assert len(copies) > 20
            if label.startswith(("f16", "mode")):
                assert set(copies) <= exact, (K, label, "the copies' bands did not overflow")
    report("overflowing band", stats)


# ------------------------------------------------------------------------------------ b. the tie check
class Checker:
    """A case's ranges, pool and device-order candidate rows on the device; run(list, exact_sets) → the resolve set."""

    def __init__(self, c, entry="plain"):
        self.c, self.entry = c, entry
        self.tab = table_of(c)
        cand = np.full((c.max_q, c.K), -1, I32)
        cand[c.ids] = c.dev
        self.cand, self.ranges, self.pool = td(cand.reshape(-1)), td(c.ranges.reshape(-1)), td(c.pool.reshape(-1))

    def run(self, lst, exact_sets, max_ties=None):
        c = self.c
        mt = c.max_q if max_ties is None else max_ties
        tl = td(lst)
        res = torch.full((1 + c.max_q,), -9, dtype=torch.int32, device=DEV)
        res[0] = 12345  # the call resets the count
        head = (self.ranges.data_ptr(), c.max_q, c.rs, self.cand.data_ptr(), c.K, self.pool.data_ptr(), c.nd,
                self.tab.emb.data_ptr())
        tail = (c.q_offset, O.blas_threads(), tl.data_ptr(), mt, exact_sets, res.data_ptr(), stream())
        if self.entry == "q":
            call("fwav_tie_check_q", *head, self.tab.emb.data_ptr(), *tail)
        elif self.entry == "dim":
            call("fwav_tie_check_dim", *head, c.emb_dim, *tail)
        else:
            call("fwav_tie_check", *head, *tail)
        torch.cuda.synchronize()
        r = res.cpu().numpy()
        n = int(r[0])
        assert 0 <= n <= c.max_q and (r[1 + n:] == -9).all(), ("resolve written past its count", r[:8])
        rows = r[1:1 + n].tolist()
        assert len(set(rows)) == n, "a row named twice"
        return set(rows)


def want_resolve(c, mode, exact_sets):
    """depends_rule for the list written in `mode` (tie_edges.list_array) under exact_sets."""
    out = set()
    for q, (flag, n, m) in c.exp.items():
        if c.K > 64 or exact_sets >= 2 or (flag and (exact_sets >= 1 or mode == "uncollected" or n > TE.MAX_LEFT)):
            out.add(q)
        elif c.rule[q]:  # (a record with its members: the rule on the errors; the members' order does not matter)
            out.add(q)
    return out


def check_tie_check(c, entry, tally):
    ck = Checker(c, entry)
    rng = np.random.default_rng(c.nd + c.K)
    order = rng.permutation(sorted(c.exp)).tolist()  # the search appends records in no particular order
    truly = {q for q in c.exp if c.truly[q]}
    for mode in ("full", "uncollected", "reversed"):
        lst = TE.list_array(c.exp, c.max_q, mode, order)
        for es in (0, 1, 2):
            got = ck.run(lst, es)
            want = want_resolve(c, mode, es)
            label = (c.nd, c.K, c.rs, c.emb_dim, entry, mode, es)
            assert got <= set(c.exp), (label, "rows not listed were named", sorted(got - set(c.exp))[:10])
            assert truly <= got, (label, "a match that depends on numpy's order is kept", sorted(truly - got)[:10])
            assert got == want, (label, "resolve vs depends_rule", sorted(got ^ want)[:10])
            if mode == "full" and es == 0:
                tally += np.array([len(c.exp), len(got), len(want), len(truly)])
    # max_ties = 0 writes only the count
    assert ck.run(TE.list_array(c.exp, c.max_q), 0, max_ties=0) == set()
    # the restatement of mode "uncollected" itself: the plain rule with count −1
    for q, (flag, n, m) in list(c.exp.items())[:8]:
        j = c.row_of[q]
        assert TE.depends_rule(c.rows[j], c.K, c.dev[j], flag, -1 if flag else 0, m, c.ranges[q], c.pool) == \
            (q in want_resolve(c, "uncollected", 0))


@pytest.mark.parametrize("nd", TE.ND_ALL)
def test_tie_check_equals_the_rule(nd):
    """Each table with its range size (40: 4, 64: 5, 65: 8, 257: 16, 600: 19 — the three templated kernels and the
    runtime one twice), every K, both entry points of width 16; K = 65: every listed row is resolved."""
    tally = np.zeros(4, np.int64)
    for K in TE.K_ALL:
        c = TE.case(nd, K)
        check_tie_check(c, "plain", tally)
        if K in (2, 64):
            check_tie_check(c, "q", tally * 0)
    c = TE.Case(nd, 65, TE.RS_OF_ND[nd], TE.SEED_OF_ND[nd], decisions=False)
    ck = Checker(c)
    for mode in ("full", "uncollected"):
        for es in (0, 1, 2):
            assert ck.run(TE.list_array(c.exp, c.max_q, mode), es) == set(c.exp), (nd, 65, mode, es)
    print(f"\nnd = {nd}, exact_sets 0, records with members: listed {tally[0]}, resolved {tally[1]}, "
          f"depends_rule {tally[2]}, truly_depends {tally[3]}")


@pytest.mark.parametrize("rs", [4, 8, 16, 5, 19])
def test_tie_check_other_range_sizes_and_width_32(rs):
    """The 65-row table at every range size (K = 17 and 64), the 257-row table with q_offset = 100 (range sizes 4 and
    19), and the width-32 table through fwav_tie_check_dim."""
    tally = np.zeros(4, np.int64)
    for K in (17, 64):
        check_tie_check(TE.case(65, K, rs=rs), "plain", tally)
    if rs in (4, 19):
        check_tie_check(TE.case(257, 32, rs=rs, q_offset=100), "q" if rs == 4 else "plain", tally)
    check_tie_check(TE.case(257, 32, rs=rs, emb_dim=32), "dim", tally)
    if rs == 16:
        check_tie_check(TE.case(257, 64, rs=rs, emb_dim=32), "dim", tally)
    print(f"\nrs = {rs}: listed {tally[0]}, resolved {tally[1]}, depends_rule {tally[2]}, truly_depends {tally[3]}")


# ------------------------------------------------------------------------------------ c. the product sequence
def product_sequence(c, tie_order):
    """search (fp16, the product's policy) → fwav_affine → fwav_tie_check → fwav.ties.resolve_rows (exact score rows,
    numpy's ranking, the fix-up kernels) → (cand, the five outputs, the resolved rows)."""
    tab = table_of(c)
    nd, K, mq, rs, T = c.nd, c.K, c.max_q, c.rs, O.blas_threads()
    act, n_act = td(c.ids), td(np.array([len(c.ids)], I32))
    cand = torch.full((mq * K,), -1, dtype=torch.int32, device=DEV)  # rows of unsearched queries: no candidates
    tl = torch.empty(size_call("fwav_tie_list_size", mq), dtype=torch.int32, device=DEV)
    wk = size_call("fwav_sim_topk_workspace_size", mq, nd, K)
    ws = torch.zeros(max(wk, 16), dtype=torch.uint8, device=DEV)
    st = stream()
    call("fwav_sim_topk", tab.emb.data_ptr(), tab.e16.data_ptr(), nd, act.data_ptr(), n_act.data_ptr(), mq, c.q_offset,
         K, T, cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, st)
    ranges, pool = td(c.ranges.reshape(-1)), td(c.pool.reshape(-1))
    outs = [torch.empty(mq, dtype=dt, device=DEV) for dt in (torch.int32, torch.float32, torch.float32, torch.uint8,
                                                            torch.float32)]
    call("fwav_affine", ranges.data_ptr(), mq, rs, cand.data_ptr(), K, pool.data_ptr(), nd, 16.0,
         *[t.data_ptr() for t in outs], st)
    rows = []
    if tie_order != "index":
        resolve = torch.empty(mq + 1, dtype=torch.int32, device=DEV)
        call("fwav_tie_check", ranges.data_ptr(), mq, rs, cand.data_ptr(), K, pool.data_ptr(), nd, tab.emb.data_ptr(),
             c.q_offset, T, tl.data_ptr(), mq, TIE_MODES[tie_order], resolve.data_ptr(), st)
        n = int(resolve[0].item())
        fties.resolve_rows(resolve[1:1 + n], emb=tab.emb, n_domains=nd, q_offset=c.q_offset, k=K, threads=T,
                           ranges=ranges, range_size=rs, pool=pool, s_clip=16.0, cand=cand, outs=tuple(outs), stream=st)
        rows = resolve[1:1 + n].cpu().tolist()
    torch.cuda.synchronize()
    return cand.cpu().numpy().reshape(mq, K), [t.cpu().numpy() for t in outs], rows


@pytest.mark.parametrize("nd", TE.ND_ALL)
def test_product_sequence_every_tie_order(nd):
    """"numpy": every match tuple is O.affine of numpy's own row; "numpy_sets": the candidate sets are numpy's too;
    "numpy_rows": the rows are; "index" (no resolution) differs from numpy's tuples only on rows in truly_depends."""
    n_res = {}
    for K in TE.K_ALL:
        c = TE.case(nd, K)
        npy = np.stack([O.numpy_topk_row(r, K) for r in c.rows])
        with np.errstate(all="ignore"):
            want = [np.asarray(a) for a in O.affine(c.ranges[c.ids], npy, c.pool)]
        for order in ("numpy", "numpy_sets", "numpy_rows", "index"):
            cand, outs, rows = product_sequence(c, order)
            n_res[order] = n_res.get(order, 0) + len(rows)
            diff = [int(q) for j, q in enumerate(c.ids)
                    if not all(AE.same_bits_or_nan(o[q:q + 1], w[j:j + 1].astype(o.dtype)) for o, w in zip(outs, want))]
            if order == "index":
                assert set(diff) <= {q for q in c.exp if c.truly[q]}, (nd, K, order, diff[:10])
                assert np.array_equal(cand[c.ids], c.dev)
                continue
            assert not diff, (nd, K, order, diff[:10])
            assert set(rows) <= set(c.exp)
            if order == "numpy":  # at least what the rule names (a −1 record of the exact-mode relaunch adds to it)
                assert want_resolve(c, "full", 0) <= set(rows), (nd, K, sorted(want_resolve(c, "full", 0) - set(rows)))
            if order in ("numpy_sets", "numpy_rows"):
                for j, q in enumerate(c.ids):
                    assert set(cand[q].tolist()) == set(npy[j].tolist()), (nd, K, order, int(q))
            if order == "numpy_rows":
                assert np.array_equal(cand[c.ids], npy), (nd, K, order)
    print(f"\nnd = {nd}: rows resolved per tie_order {n_res}")
