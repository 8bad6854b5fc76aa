"""compress_audio(query="range") on the device: each range searched with its own embedding (what the reference's
range_candidates_from_embedding computes, fractal.py:337-351) instead of domain row i (quirk Q1).

Expected values come from a numpy restatement built here from the oracle's stages — O.embed for the queries,
O.sgemv_scores + O.sgemv_col_kind for the scores in the reference's sgemv order, (score desc, index asc) for the
device's candidate rows, O.numpy_topk_row on the whole score row wherever the top K + 1 hold an exact tie,
O.zero_query_candidates for an all-zero query, O.affine for the match — and nothing below has a tolerance: embeddings,
candidate rows, tie lists and match tuples are compared bit for bit.  The one inequality is the point of the feature:
the encoder's own fit SNR gains at least 3 dB over the default on the four signals whose CPU restatement gained at
least 8.0 dB."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import api, engine, synth  # noqa: E402
from fwav._lib import call, debug_library, size_call  # noqa: E402
from fwav.fwavio import load_compressed, save_compressed  # noqa: E402
from golden_util import bit_equal, load  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

DEV = torch.device("cuda", 0)
F32 = np.float32
TIE_REC = 9


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# --------------------------------------------------------------------------------------------- the restatement
def restate_top(E, Q, kk, threads, chunk=512):
    """For every query row of Q against the table E: the kk best domains in (score desc, index asc) order and their
    scores in the reference's sgemv order — BLAS scores (within O.SGEMV_GAP of them) pick a superset of every domain
    that can be among the kk best, which is then scored exactly (as O.topk_rows does for queries that are table rows)."""
    E, Q = np.asarray(E, F32), np.asarray(Q, F32)
    nd = len(E)
    kk = min(kk, nd)
    idx = np.zeros((len(Q), kk), np.int64)
    sc = np.zeros((len(Q), kk), F32)
    for a in range(0, len(Q), chunk):
        fast = Q[a:a + chunk] @ E.T
        Tf = -np.partition(-fast, kk - 1, axis=1)[:, kk - 1]
        for j in range(len(fast)):
            sup = np.nonzero(fast[j] >= Tf[j] - O.SGEMV_GAP)[0]
            ex = O.sgemv_scores(E[sup], Q[a + j][None, :], O.sgemv_col_kind(sup, nd, threads))[0]
            o = np.lexsort((sup, -ex))[:kk]
            idx[a + j], sc[a + j] = sup[o], ex[o]
    return idx, sc


def cut_top(idx, sc, K):
    """The device's contract for K from the K + 1 best: (cand i32[n, K] −1-padded, tied bool[n]: an exact tie among
    the top K + 1 scores)."""
    n, kk = idx.shape
    cand = np.full((n, K), -1, np.int32)
    cand[:, :min(K, kk)] = idx[:, :K]
    m = min(K + 1, kk)
    return cand, (sc[:, 1:m] == sc[:, :m - 1]).any(axis=1)


def unit_head_rows(rng, n):
    """n rows of two heads of 8 columns, each of norm just under 1 (the search's error bounds need ≤ 1)."""
    x = rng.standard_normal((n, 2, 8))
    x /= np.sqrt((x ** 2).sum(-1, keepdims=True)) * (1 + 1e-6)
    return x.reshape(n, 16).astype(F32)


def restate_compress(sig, tile, K, thr=1e-4, fast_mode=True, threads=None):
    """compress_audio(query="range") in numpy: the oracle's stages with the queries embedded from the ranges."""
    sig = np.asarray(sig, F32)
    threads = O.blas_threads() if threads is None else threads
    rs, step = O.geometry(tile)
    vm = O.voiced_detection(sig, frame_size=2 * rs, energy_threshold=thr)
    ranges, _ = O.form_ranges(sig, vm, rs)
    pool = O.domain_pool(sig, tile, rs, step)
    E, Q = O.embed(pool), O.embed(ranges)
    nr, nd = len(ranges), len(pool)
    pruned = O.range_energy_pruned(ranges, thr, fast_mode)
    zero = ~pruned & np.all(Q == 0, axis=1)
    cand = np.full((nr, K), -1, np.int32)
    cand[zero] = O.zero_query_candidates(nd, K)
    act = np.nonzero(~pruned & ~zero)[0]
    idx, sc = restate_top(E, Q[act], K + 1, threads)
    c, tied = cut_top(idx, sc, K)
    for j in np.nonzero(tied)[0]:  # numpy's own order among exactly equal scores (fractal.py:537-541)
        c[j] = O.numpy_topk_row(O.reference_row_scores(E, Q[act[j]], threads), K)
    cand[act] = c
    m = O.affine(ranges, cand, pool)
    return dict(rs=rs, step=step, ranges=ranges, pool=pool, emb=E, qemb=Q, pruned=pruned, zero=zero, cand=cand,
                tied=act[tied], m=m, nr=nr, nd=nd)


# ------------------------------------------------------------------------------------------- device harness
def embed_rows(rows, rs, exact=False, want16=True):
    rows = np.ascontiguousarray(rows, F32)
    n = len(rows)
    tab = engine.embed_tables(rs, DEV, "pocketfft" if exact else "matrix")
    r = td(rows.reshape(-1))
    emb = torch.full((max(n, 1) * 16,), 7.0, dtype=torch.float32, device=DEV)
    e16 = torch.full((size_call("fwav_emb16_elems", max(n, 1)),), 3.0, dtype=torch.float16, device=DEV) if want16 else None
    call("fwav_embed_rows_exact" if exact else "fwav_embed_rows", r.data_ptr(), n, rs, tab.data_ptr(), emb.data_ptr(),
         None if e16 is None else e16.data_ptr(), stream())
    torch.cuda.synchronize()
    return emb, e16


def emb16_of(emb, n):
    e16 = torch.full((size_call("fwav_emb16_elems", n),), 5.0, dtype=torch.float16, device=DEV)
    call("fwav_emb16_from_emb", emb.data_ptr(), n, e16.data_ptr(), stream())
    return e16


class Search:
    """One table, one query table and one active list on the device; run(K, …) returns (cand, tied rows)."""

    def __init__(self, E, Q, active):
        self.nd, self.nq = len(E), len(Q)
        self.emb, self.qemb = td(E.reshape(-1)), td(Q.reshape(-1))
        self.emb16, self.qemb16 = emb16_of(self.emb, self.nd), emb16_of(self.qemb, self.nq)
        self.active = td(np.asarray(active, np.int32))
        self.n_active = td(np.array([len(active)], np.int32))
        self.m = int(max(active)) + 1 if len(active) else 1

    def run(self, K, stride=1, f16=True, threads=1, plain=False, debug_entry=False):
        m = self.m
        cand = torch.full((m * K,), -7, dtype=torch.int32, device=DEV)
        ties = torch.zeros(size_call("fwav_tie_list_size", m), dtype=torch.int32, device=DEV)
        wk = size_call("fwav_sim_topk_workspace_size", m, self.nd, K) if f16 else 0
        ws = torch.empty(max(wk, 16), dtype=torch.uint8, device=DEV)
        e16 = self.emb16.data_ptr() if f16 else None
        q16 = self.qemb16.data_ptr() if f16 else None
        if plain:
            call("fwav_sim_topk", self.emb.data_ptr(), e16, self.nd, self.active.data_ptr(), self.n_active.data_ptr(), m,
                 0, K, threads, cand.data_ptr(), ties.data_ptr(), ws.data_ptr(), wk, stream())
        elif debug_entry:
            call("fwav_debug_sim_topk_q", self.emb.data_ptr(), e16, self.nd, self.qemb.data_ptr(), q16, self.nq, stride,
                 self.active.data_ptr(), self.n_active.data_ptr(), m, 0, K, cand.data_ptr(), ws.data_ptr(), wk, 0, None,
                 stream())
        else:
            call("fwav_sim_topk_q", self.emb.data_ptr(), e16, self.nd, self.qemb.data_ptr(), q16, self.nq, stride,
                 self.active.data_ptr(), self.n_active.data_ptr(), m, 0, K, threads, cand.data_ptr(), ties.data_ptr(),
                 ws.data_ptr(), wk, stream())
        torch.cuda.synchronize()
        t = ties.cpu().numpy()
        rows = np.sort(t[1:1 + TIE_REC * int(t[0])].reshape(-1, TIE_REC)[:, 0] >> 1)
        return cand.cpu().numpy().reshape(m, K), rows


# ------------------------------------------------------------------------------------- 1. fwav_embed_rows
ROW_COUNTS = (1, 255, 256, 257, 1000)


def _rows(rng, n, rs):
    x = (rng.standard_normal((n, rs)) * rng.choice([1e-3, 0.1, 1.0], (n, 1))).astype(F32)
    x = np.clip(x, -1.0, 1.0)
    for j, v in enumerate((0.0, 0.25, 1.0, -1.0)):  # all-zero, constant (a zero embedding), ± full scale
        if j < n:
            x[-1 - j] = v
    if n > 8:
        x[3] = np.where(np.arange(rs) % 2 == 0, 1.0, -1.0)
        x[4, 1:] = 0.0
    return x


@pytest.mark.parametrize("rs,exact", [(4, False), (8, False), (16, False), (5, True), (19, True), (32, True),
                                      (8, True)])
def test_embed_rows_equals_the_oracle_bit_for_bit(rs, exact):
    rng = np.random.default_rng(100 + rs)
    for n in ROW_COUNTS:
        rows = _rows(rng, n, rs)
        want = O.embed(rows)
        emb, e16 = embed_rows(rows, rs, exact)
        got = emb.cpu().numpy().reshape(-1, 16)[:n]
        assert bit_equal(got, want), (rs, n, np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0][:5])
        assert np.array_equal(e16.cpu().numpy().view(np.uint16), emb16_of(emb, n).cpu().numpy().view(np.uint16)), (rs, n)
        emb2, _ = embed_rows(rows, rs, exact, want16=False)  # emb16 is optional
        assert bit_equal(emb2.cpu().numpy()[:n * 16], got.reshape(-1))
        if n >= 4:
            # the all-zero row embeds to zero, and so does the constant one wherever its DCT is exactly zero beyond the
            # mean (at other sizes pocketfft's f32 rounding leaves a residue that the head normalises, as the oracle's)
            assert not got[-1].any() and (rs not in (4, 8, 16) or not got[-2].any())
        # every head of a query row has norm ≤ 1, as a pool row's has: the search's bounds δ, δ′ and the centroid
        # bound hold for these queries (as test_embedding_heads_at_most_unit_norm asserts for the table)
        e = got.astype(np.float64)
        for head in (e[:, :8], e[:, 8:]):
            assert np.sqrt((head ** 2).sum(1)).max() <= 1 + 1e-6


def test_embed_rows_is_the_pool_rows_embedding():
    """The same kernel on other rows: embedding the pool rows as caller rows gives the table fwav_pool_embed built."""
    sig = synth.noise(0.5, 44100, seed=3)
    for tile, embedding in ((2048, "matrix"), (5000, "pocketfft"), (8192, "matrix")):
        r = engine.compress_device(td(sig), tile, 8, keep_intermediates=True, embedding=embedding)
        rs = r.range_size
        emb, _ = embed_rows(r.pool.cpu().numpy().reshape(-1, rs), rs, exact=embedding == "pocketfft")
        assert bit_equal(emb.cpu().numpy(), r.emb.cpu().numpy()), tile


# ------------------------------------------------------------------------------- 2. the pointer swap is complete
@pytest.mark.parametrize("case,K", [("noise2048", 64), ("sweep", 32), ("tone", 32)])
def test_query_table_equal_to_the_domain_table_is_the_plain_search(case, K):
    g = load(case)
    E = g["emb"]
    nd = len(E)
    nq = min(g["p"]["n_ranges"], nd)
    active = np.nonzero(~O.range_energy_pruned(g["ranges"][:nq], g["p"]["thr"]) & E[:nq].any(axis=1))[0]
    s = Search(E, E, active)
    for f16 in (True, False):
        want, wt = s.run(K, f16=f16, plain=True)
        got, gt = s.run(K, stride=1, f16=f16)
        assert np.array_equal(got, want) and np.array_equal(gt, wt), (case, f16)
    assert len(active) > 100


# ----------------------------------------------------------------------------------------- 3. unrelated queries
def _tie_table(rng, n):
    """≈ 60,000 unit-head rows with exact duplicates, one-ulp near-duplicates and one cluster of 400 copies of a row
    (more than the band's 192 entries within the margin: the hi/lo and exact-mode relaunches serve its queries)."""
    E = unit_head_rows(rng, n)
    src = rng.integers(0, n, 3000)
    dst = rng.integers(0, n, 3000)
    E[dst[:1500]] = E[src[:1500]]
    near = E[src[1500:]].copy()
    col = rng.integers(0, 16, 1500)
    near[np.arange(1500), col] = np.nextafter(near[np.arange(1500), col], F32(0))  # one ulp towards zero: norm ≤ 1
    E[dst[1500:]] = near
    E[rng.choice(n, 400, replace=False)] = E[17]
    return E


def _queries(rng, E, nq):
    Q = unit_head_rows(rng, nq)
    if nq >= 33:
        Q[5] = E[17] if len(E) > 17 else Q[5]  # a query whose best scores are exact ties where the table has copies
        Q[9] = 0.0                              # all-zero queries take the zero_cand row and are not searched
        Q[nq - 2] = 0.0
    return Q


def _active_by_prune(Q, nd, K, rs=4):
    """fwav_prune_q on ranges of which every 7th is silent: the active list (with gaps), the candidate rows it wrote."""
    nq = len(Q)
    ranges = np.full((nq, rs), 0.5, F32)
    ranges[::7] = 0.0
    if nq == 1:
        ranges[:] = 0.5
    zc = td(O.zero_query_candidates(nd, K))
    cand = torch.full((nq * K,), -9, dtype=torch.int32, device=DEV)
    active = torch.full((nq,), -1, dtype=torch.int32, device=DEV)
    n_active = torch.zeros(1, dtype=torch.int32, device=DEV)
    rt, qt = td(ranges.reshape(-1)), td(Q.reshape(-1))
    call("fwav_prune_q", rt.data_ptr(), nq, 0, rs, float(F32(0.75e-4)), 1, qt.data_ptr(), nq, nd, K, zc.data_ptr(), cand.data_ptr(), active.data_ptr(), n_active.data_ptr(), stream())
    torch.cuda.synchronize()
    na = int(n_active.item())
    silent = ~ranges.any(axis=1)
    zero = ~silent & ~Q.any(axis=1)
    want = np.nonzero(~silent & ~zero)[0]
    got = np.sort(active.cpu().numpy()[:na])
    assert np.array_equal(got, want)
    c = cand.cpu().numpy().reshape(nq, K)
    assert (c[silent] == -1).all() and (c[zero] == O.zero_query_candidates(nd, K)).all()
    assert (c[want] == -9).all()  # searchable rows are left to the search
    return active.cpu().numpy()[:na]


KNOBS = [(geo, sets, mode, floor) for (geo, sets) in ((0, -1), (1, -1), (2, 2), (2, 4), (3, -1)) for mode in (0, 1)
         for floor in (0, 2)]


@pytest.mark.parametrize("nd", [40, 77, 255, 257, 2049, 60_000])
def test_unrelated_queries_every_geometry_equals_f32_equals_numpy(nd):
    rng = np.random.default_rng(nd)
    E = _tie_table(rng, nd) if nd >= 60_000 else unit_head_rows(rng, nd)
    for nq in (1, 33, 275, 2100):
        Q = _queries(rng, E, nq)
        active = _active_by_prune(Q, nd, 32)
        if len(active) == 0:
            continue
        s = Search(E, Q, active)
        rows = np.sort(active)
        idx, sc = restate_top(E, Q[rows], 65, 1)
        for K in (1, 32, 64):
            c, tied = cut_top(idx, sc, K)
            ref, rt = s.run(K, stride=1, f16=False)  # the all-f32 kernel with a query table
            assert np.array_equal(ref[rows], c), (nd, nq, K)
            assert np.array_equal(rt, rows[tied]), (nd, nq, K)
            if K > nd:
                assert (ref[rows][:, nd:] == -1).all() and (ref[rows][:, :nd] >= 0).all()
            for stride in (0, 1, 4):
                got, gt = s.run(K, stride=stride)  # the product's own policy
                assert np.array_equal(got[rows], c) and np.array_equal(gt, rt), (nd, nq, K, stride)
                for geo, sets, mode, floor in KNOBS:
                    with debug_library():
                        call("fwav_debug_topk_geometry", geo)
                        call("fwav_debug_topk_cent_sets", sets)
                        call("fwav_debug_topk_mode", mode)
                        call("fwav_debug_topk_floor", floor, 0.0)
                        got, gt = s.run(K, stride=stride)
                    assert np.array_equal(got[rows], c), (nd, nq, K, stride, geo, sets, mode, floor)
                    assert np.array_equal(gt, rt), (nd, nq, K, stride, geo, sets, mode, floor)
            with debug_library():  # the debug entry point itself (no tie list)
                call("fwav_debug_topk_geometry", 2)
                got, _ = s.run(K, stride=4, debug_entry=True)
            assert np.array_equal(got[rows], c), (nd, nq, K)
        if nd >= 60_000 and nq >= 275:
            assert tied.any()  # the table's copies do tie


def test_blas_thread_split_reaches_the_query_table_search():
    """Scores in the sgemv order of blas_threads: a table large enough for OpenBLAS to split (16·nd ≥ 460,800), where
    the split's tail columns take other kernels."""
    rng = np.random.default_rng(5)
    nd, nq, K = 30_011, 300, 32
    E, Q = unit_head_rows(rng, nd), unit_head_rows(rng, nq)
    s = Search(E, Q, np.arange(nq))
    for threads in (1, 7):
        idx, sc = restate_top(E, Q, K + 1, threads)
        c, tied = cut_top(idx, sc, K)
        for f16 in (False, True):
            got, gt = s.run(K, stride=4, f16=f16, threads=threads)
            assert np.array_equal(got, c) and np.array_equal(gt, np.nonzero(tied)[0]), (threads, f16)


# -------------------------------------------------------------------------------------------------- 4. pipeline
PIPE = {
    "tone": (lambda: (synth.tone(), 128, 32, {})),
    "sweep": (lambda: (synth.sweep(0.25, 16000), 1024, 32, {})),
    "speech1024": (lambda: (synth.speech_like(0.5, 44100), 1024, 32, {})),
    "speech2048": (lambda: (synth.speech_like(0.5, 44100), 2048, 64, {})),
    "speech4096": (lambda: (synth.speech_like(0.5, 44100), 4096, 32, {})),
    "more_ranges_than_domains": (lambda: (synth.noise(1100 / 44100, 44100, seed=2)[:1100], 1024, 32, {})),
    "slow_mode": (lambda: (synth.speech_like(0.25, 44100, seed=4, floor=False), 2048, 32, dict(fast_mode=False))),
    "pocketfft5000": (lambda: (synth.speech_like(0.5, 44100, seed=1), 5000, 32, dict(embedding="pocketfft"))),
}
_RESTATED: dict = {}


def _pipe(name):
    if name not in _RESTATED:
        sig, tile, K, kw = PIPE[name]()
        _RESTATED[name] = (sig, tile, K, kw, restate_compress(sig, tile, K, fast_mode=kw.get("fast_mode", True)))
    return _RESTATED[name]


def _assert_tuple(matches, ref, what):
    for got, want, nm in zip((matches.idx, matches.s, matches.o, matches.sym, matches.err), ref["m"],
                             ("idx", "s", "o", "sym", "err")):
        assert bit_equal(np.asarray(got), want), (what, nm, np.nonzero(np.asarray(got) != want)[0][:5])


@pytest.mark.parametrize("name", list(PIPE))
def test_pipeline_equals_the_restatement_tuple_for_tuple(name, tmp_path):
    sig, tile, K, kw, ref = _pipe(name)
    out = api.compress_audio(sig, 44100, 2, tile_size=tile, top_k=K, query="range", **kw)
    matches, domains, nr, rs, tile_o, step, thr, orig = out
    assert (nr, rs, step, orig) == (ref["nr"], ref["rs"], ref["step"], len(sig)) and bit_equal(domains, ref["pool"])
    _assert_tuple(matches, ref, name)
    if name == "more_ranges_than_domains":
        assert (nr, len(domains)) == (275, 77)
        with pytest.raises(ValueError, match="mmap length"):  # the default keeps quirk Q9
            api.compress_audio(sig, 44100, 2, tile_size=tile, top_k=K)
    if name == "slow_mode":
        assert ref["zero"].any() and not ref["pruned"].any()  # masked ranges are constant: the zero_cand row
    # the intermediates: the query table is the oracle's embedding of the ranges, the domain table is untouched
    r = engine.compress_device(td(sig), tile, K, keep_intermediates=True, query="range", **kw)
    torch.cuda.synchronize()
    assert bit_equal(r.qemb.cpu().numpy().reshape(-1, 16), ref["qemb"]) and bit_equal(r.emb.cpu().numpy().reshape(-1, 16),
                                                                                     ref["emb"])
    assert np.array_equal(np.sort(r.ties.cpu().numpy()[1:1 + TIE_REC * r.n_ties].reshape(-1, TIE_REC)[:, 0] >> 1),
                          ref["tied"])
    # every other tie order and the all-f32 search agree wherever numpy's order cannot matter, "numpy_rows" everywhere
    r2 = engine.compress_device(td(sig), tile, K, keep_intermediates=True, query="range", tie_order="numpy_rows",
                                search="f32", **kw)
    torch.cuda.synchronize()
    assert np.array_equal(r2.cand.cpu().numpy().reshape(-1, K), ref["cand"])
    # save / load / decode round trip, and the compact set composes
    path = str(tmp_path / "q.fwav")
    save_compressed(path, matches, domains, rs, 44100, 2, tile, step, thr, orig)
    lm, ld, lnr, lrs, *_ = load_compressed(path)
    assert (lnr, lrs) == (nr, rs) and bit_equal(ld, domains) and bit_equal(lm.err, matches.err)
    for d in (0.0, 1e-6):
        want, it, _ = O.decode(*ref["m"][:4], ref["pool"], nr, rs, original_len=orig, s_damping=d)
        got, info = api.decompress_audio(lm, ld, lnr, lrs, original_len=orig, s_damping=d, return_info=True)
        assert bit_equal(got, want) and info["iterations"] == it, (name, d)
    cm, cd, *rest = api.compress_audio(sig, 44100, 2, tile_size=tile, top_k=K, query="range", compact=True, **kw)
    assert rest[0] == nr and len(cd) == len(np.unique(ref["m"][0])) and bit_equal(cd[cm.idx], ref["pool"][ref["m"][0]])
    assert bit_equal(api.decompress_audio(cm, cd, nr, rs, original_len=orig), O.decode(
        *ref["m"][:4], ref["pool"], nr, rs, original_len=orig)[0])


def test_sub_blocks_shards_and_deferred_ties_agree():
    """The same slicing and tie machinery drives the _q entry points: sliced searches, a shard and a deferred
    resolution return the whole call's tuples."""
    sig, tile, K, kw, ref = _pipe("speech1024")
    t = td(sig)
    for opts in (dict(sub_blocks=3), dict(defer_ties=True), dict(sub_blocks=2, defer_ties=True)):
        r = engine.compress_device(t, tile, K, query="range", **opts).wait()
        torch.cuda.synchronize()
        for got, want in zip((r.idx, r.s, r.o, r.sym, r.err), ref["m"]):
            assert bit_equal(got.cpu().numpy(), want), opts
    lo, hi = 1000, 3001
    r = engine.compress_device(t, tile, K, query="range", shard=(lo, hi))
    torch.cuda.synchronize()
    for got, want in zip((r.idx, r.s, r.o, r.sym, r.err), ref["m"]):
        assert bit_equal(got.cpu().numpy(), want[lo:hi])


# ----------------------------------------------------------------------------------- 5. the point of the feature
def fit_snr(ranges, err):
    ok = np.isfinite(err)
    return 10 * np.log10((ranges[ok].astype(np.float64) ** 2).sum() / (err[ok].astype(np.float64) ** 2).sum())


@pytest.mark.parametrize("name", ["speech2048", "speech1024", "sweep1024", "noise2048"])
def test_fit_snr_gains_at_least_3_db(name):
    """Rows 1, 2, 4 and 5 of the issue's table (K = 32): the smallest gain of the CPU restatement there is 8.0 dB."""
    sig, tile = {"speech2048": (lambda: synth.speech_like(1.5, 44100), 2048),
                 "speech1024": (lambda: synth.speech_like(1.5, 44100), 1024),
                 "sweep1024": (lambda: synth.sweep(1.0, 16000), 1024),
                 "noise2048": (lambda: synth.noise(1.0, 44100), 2048)}[name]
    sig = sig()
    snr = {}
    for q in ("domain_row", "range"):
        r = engine.compress_device(td(sig), tile, 32, keep_intermediates=True, query=q)
        torch.cuda.synchronize()
        snr[q] = fit_snr(r.ranges.cpu().numpy().reshape(-1, r.range_size), r.err.cpu().numpy())
    print(f"{name}: fit SNR domain_row {snr['domain_row']:.2f} dB, range {snr['range']:.2f} dB")
    assert snr["range"] >= snr["domain_row"] + 3.0, snr


# ---------------------------------------------------------------------------------- 6. the default is untouched
def _arrays(m):
    return tuple(np.asarray(getattr(m, f)) for f in ("idx", "s", "o", "sym", "err"))


def test_default_is_domain_row():
    sig = synth.noise(0.5, 44100, seed=7)  # the golden smoke signal
    a = api.compress_audio(sig, 44100, 2, tile_size=2048, top_k=64)
    b = api.compress_audio(sig, 44100, 2, tile_size=2048, top_k=64, query="domain_row")
    for x, y in zip(_arrays(a[0]), _arrays(b[0])):
        assert bit_equal(x, y)
    assert bit_equal(a[1], b[1]) and a[2:] == b[2:]
    ref = O.compress(sig, 2048, 64)
    for x, nm in zip(_arrays(a[0]), ("idx", "s", "o", "sym", "err")):
        assert bit_equal(x, ref[nm]), nm  # still the reference's Q1 matches
    c = api.compress_audio(sig, 44100, 2, tile_size=2048, top_k=64, query="range")
    assert not np.array_equal(np.asarray(c[0].idx), ref["idx"])  # ... which the option does change
