"""compress_audio(emb_dim=32) on the device, against the reference's own outputs (tests/golden/embdim32_*.npz, made by
tests/golden/make_embdim32.py) and against numpy on this host: the wide embedding, the exact score rows, the wide
search (fwav_topk_wide.hip for K ≤ 64, fwav_topk_large.hip above) with its tie list, and the whole pipeline through
the Python API, the torch-free host and the CLI."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, bit_equal, load

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import api, engine, ties  # noqa: E402
from fwav._lib import call, size_call  # noqa: E402
from fwav.fwavio import save_compressed, write_wav  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

F32 = np.float32
D = 32
CASES = ("t1024", "t2048", "t4096", "periodic2048")
TIE_REC = 9


def dev():
    return torch.device("cuda", 0)


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def stream():
    return torch.cuda.current_stream().cuda_stream


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def fixture(case):
    g = dict(np.load(os.path.join(GOLDEN, f"embdim32_{case}.npz")))
    g["p"] = json.loads(str(g.pop("params")))
    return g


# ------------------------------------------------------------------------------------------------ embedding
def pool_embed_dim(sig_np, tile, rs, step):
    """fwav_pool_embed_dim → (pool f32[nd, rs], emb f32[nd, 32], embh f16[...], the device emb tensor)."""
    sig = td(sig_np)
    n = sig.numel()
    nd = (n - tile) // step + 1
    tab = engine.embed_tables(rs, dev(), "matrix", D)
    pool = torch.empty(nd * rs, dtype=torch.float32, device=dev())
    emb = torch.empty(nd * D, dtype=torch.float32, device=dev())
    embh = torch.empty(size_call("fwav_embh_elems", nd, D), dtype=torch.float16, device=dev())
    wsn = size_call("fwav_pool_workspace_size", n, tile, rs, step)
    ws = torch.empty(max(wsn, 16), dtype=torch.uint8, device=dev())
    call("fwav_pool_embed_dim", sig.data_ptr(), n, tile, rs, step, D, tab.data_ptr(), pool.data_ptr(), emb.data_ptr(),
         embh.data_ptr(), ws.data_ptr(), wsn, stream())
    torch.cuda.synchronize()
    return pool.cpu().numpy().reshape(nd, rs), emb.cpu().numpy().reshape(nd, D), embh.cpu().numpy(), emb


def embh_layout(emb):
    """The wide search's table of rows emb f32[nd, 32] (fwav_pool_embed.hip store_embh), in numpy."""
    nd = len(emb)
    nc = -(-nd // 256)
    full = np.zeros((nc * 256, D), np.float16)
    full[:nd] = emb.astype(np.float16)
    return np.ascontiguousarray(full.reshape(nc, 256, D // 8, 8).transpose(0, 2, 1, 3)).reshape(-1)


@pytest.mark.parametrize("case", CASES[:3])
def test_embedding_bit_exact(case):
    """Range sizes 4, 8 and 16: every row of the wide embedding is the reference's, bit for bit; the fp16 table is
    f16(emb) in the search's layout, rows past nd zero, and fwav_embh_from_emb writes the same table."""
    g = fixture(case)
    p = g["p"]
    pool, emb, embh, emb_dev = pool_embed_dim(g["signal"], p["tile"], p["rs"], p["step"])
    assert emb.shape == (p["n_domains"], D)
    sub_ok = bit_equal(emb[g["emb_rows"]], g["emb_sub"])
    bad = np.flatnonzero((emb[g["emb_rows"]].view(np.uint32) != g["emb_sub"].view(np.uint32)).any(1))
    assert sub_ok, (case, g["emb_rows"][bad[:5]], emb[g["emb_rows"][bad[:1]]], g["emb_sub"][bad[:1]])
    assert sha(emb) == str(g["emb_sha256"])
    assert bit_equal(pool, O.domain_pool(g["signal"], p["tile"], p["rs"], p["step"]))
    want = embh_layout(emb)
    assert np.array_equal(embh.view(np.uint16), want.view(np.uint16))
    again = torch.full_like(td(embh), 7.0)
    call("fwav_embh_from_emb", emb_dev.data_ptr(), len(emb), D, again.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy().view(np.uint16), want.view(np.uint16))
    # the layout the issue states: [tonal: min(16, rs − 1), zero-padded to 16][transient: min(16, rs)][zeros to 32]
    rs = p["rs"]
    assert not emb[:, min(16, rs - 1):16].any() and not emb[:, 16 + min(16, rs):].any()
    assert np.abs(emb[:, :min(16, rs - 1)]).max() > 0.1 and np.abs(emb[:, 16:16 + min(16, rs)]).max() > 0.1


def test_embedding_matrix_route_rs19():
    """Tile 5000 (range size 19, the f64 matrix DCT): the bars of tests/test_gpu_generic_rs.py's test_embedding, on 16
    columns per head.  Tonal columns within 2⁻²² of the f64 embedding of the pool (rows whose f64 un-normalised norm
    lies in (0, 1e-6) left out, at most 1 % of them, and finite); transient columns within 2⁻²³ of the reference's
    arithmetic (oracle.embed: f64 until one final rounding)."""
    import scipy.fftpack
    g = load("t5000")
    p = g["p"]
    pool, emb, embh, _ = pool_embed_dim(g["signal"], p["tile"], p["rs"], p["step"])
    assert bit_equal(pool, g["pool"]) and p["rs"] == 19
    v = scipy.fftpack.dct(pool.astype(np.float64), norm="ortho", axis=-1) * np.linspace(1.0, 2.0, 19)
    e = v[:, 1:17].copy()
    nrm = np.sqrt((e * e).sum(1))
    ok = nrm > 1e-8
    e[ok] /= nrm[ok, None]
    out = (nrm > 0) & (nrm < 1e-6)
    assert out.mean() <= 0.01
    d_ton = np.abs(emb[:, :16].astype(np.float64) - e)[~out].max()
    ref = O.embed(pool, emb_dim=D)
    d_tr = np.abs(emb[:, 16:].astype(np.float64) - ref[:, 16:].astype(np.float64)).max()
    print(f"rs 19, emb_dim 32: tonal max |d| vs f64 {d_ton:.3e} (bar {2.0 ** -22:.3e}), transient vs reference "
          f"arithmetic {d_tr:.3e} (bar {2.0 ** -23:.3e})")
    assert np.isfinite(emb).all() and np.abs(emb).max() <= 1 + 2.0 ** -22
    assert d_ton <= 2.0 ** -22
    assert d_tr <= 2.0 ** -23
    assert np.array_equal(embh.view(np.uint16), embh_layout(emb).view(np.uint16))


# ------------------------------------------------------------------------------------------------ tables
def unit_heads(x):
    x = np.asarray(x, F32).reshape(len(x), 2, D // 2)
    n = np.sqrt((x * x).sum(-1, dtype=F32))
    n = np.where(n > 0, n, F32(1))
    return np.ascontiguousarray((x / n[..., None]).reshape(len(x), D).astype(F32))


@functools.lru_cache(maxsize=None)
def table(kind, nd):
    rng = np.random.default_rng(1000 + nd)
    if kind == "random":
        return unit_heads(rng.normal(0, 1, (nd, D)))
    if kind == "near":  # one base row plus 1e-4 perturbations: nearly every domain lies inside the pre-filter's band
        base = rng.normal(0, 1, (1, D))
        return unit_heads(base + 1e-4 * rng.normal(0, 1, (nd, D)))
    if kind == "zeros":  # zero tonal heads, zero transient heads and all-zero rows (rows 0, 6, 12, … are queries too)
        t = unit_heads(rng.normal(0, 1, (nd, D)))
        t[0::3, :16] = 0
        t[1::5, 16:] = 0
        t[0::6] = 0
        return t
    if kind == "dups":  # every row duplicated many times over: exact ties in every score row
        base = unit_heads(rng.normal(0, 1, (max(3, nd // 9), D)))
        return np.ascontiguousarray(base[rng.integers(0, len(base), nd)])
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def table_on_device(kind, nd):
    """(emb tensor, embh tensor, numpy's score rows of queries 0 … min(129, nd) − 1 with this host's thread count, each
    row's domains in (score desc, index asc) order)."""
    t = table(kind, nd)
    emb = td(t.reshape(-1))
    embh = torch.empty(size_call("fwav_embh_elems", nd, D), dtype=torch.float16, device=dev())
    call("fwav_embh_from_emb", emb.data_ptr(), nd, D, embh.data_ptr(), stream())
    rows = np.stack([t @ t[i] for i in range(min(129, nd))])  # numpy's own sgemv, one call per query as the reference
    orders = [np.lexsort((np.arange(nd), -r.astype(np.float64))) for r in rows]
    return emb, embh, rows, orders


def contract_topk(row, k, order=None):
    """(score desc, index asc), −1 padded: what fwav_sim_topk_dim emits."""
    order = (np.lexsort((np.arange(len(row)), -row.astype(np.float64))) if order is None else order)[:k]
    out = np.full(k, -1, np.int32)
    out[:len(order)] = order
    return out


def expected_ties(rows, k):
    """{query: K-th place tie?} for the queries whose top K + 1 scores hold exactly equal values."""
    out = {}
    for i, row in enumerate(rows):
        top = np.sort(row)[::-1][:k + 1]
        eq = top[1:] == top[:-1]
        if eq.any():
            out[i] = bool(len(top) > k and eq[k - 1])
    return out


def run_search(kind, nd, nq, k, threads):
    emb, embh = table_on_device(kind, nd)[:2]
    active = td(np.arange(nq, dtype=np.int32))
    n_active = td(np.array([nq], np.int32))
    cand = torch.full((nq * k,), -7, dtype=torch.int32, device=dev())
    tl = torch.full((size_call("fwav_tie_list_size", nq),), -7, dtype=torch.int32, device=dev())
    wk = size_call("fwav_sim_topk_dim_workspace_size", nq, nd, D, k)
    ws = torch.empty(max(wk, 16), dtype=torch.uint8, device=dev())
    call("fwav_sim_topk_dim", emb.data_ptr(), embh.data_ptr(), nd, D, active.data_ptr(), n_active.data_ptr(), nq, 0, k,
         threads, cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, stream())
    torch.cuda.synchronize()
    return cand.cpu().numpy().reshape(nq, k), tl.cpu().numpy()


@pytest.mark.parametrize("k", [1, 32, 64, 100])
@pytest.mark.parametrize("nq", [1, 31, 33, 129])
@pytest.mark.parametrize("nd", [40, 255, 256, 257, 14401])
@pytest.mark.parametrize("kind", ["random", "near", "zeros", "dups"])
def test_search(kind, nd, nq, k):
    """fwav_sim_topk_dim = the top K of numpy's exact score rows in (score desc, index asc) order for every query,
    −1 padded when nd < K; where a row's top K + 1 holds no exact tie that is numpy_topk_row itself.  The tie list
    names exactly the queries (and K-th place flags) numpy's rows show.  nd = 40 cannot give more than 40 queries
    (a query is a domain row): nq is cut to 40 there.  K = 100 takes the large-K route."""
    T = O.blas_threads()
    nq = min(nq, nd)
    _, _, rows, orders = table_on_device(kind, nd)
    cand, tl = run_search(kind, nd, nq, k, T)
    want_ties = expected_ties(rows[:nq], k)
    for i in range(nq):
        assert np.array_equal(cand[i], contract_topk(rows[i], k, orders[i])), (kind, nd, nq, k, i)
        if i not in want_ties:
            assert np.array_equal(cand[i], O.numpy_topk_row(rows[i], k)), (kind, nd, nq, k, i)
    got = {int(tl[1 + TIE_REC * j]) >> 1: bool(tl[1 + TIE_REC * j] & 1) for j in range(int(tl[0]))}
    assert int(tl[0]) == len(got)
    assert got == want_ties, (kind, nd, nq, k, sorted(set(got) ^ set(want_ties))[:10])
    if kind == "random":
        assert not want_ties
    if kind == "dups" and nd > 40:
        assert want_ties


def test_search_skips_unlisted_queries_and_reads_n_active_on_device():
    """Only the queries in active[0 .. *n_active) are searched (their rows written, the others untouched), whatever
    max_q says; q_offset shifts the query rows."""
    nd, k, T = 257, 32, O.blas_threads()
    emb, embh = table_on_device("random", nd)[:2]
    t = table("random", nd)
    act = np.array([5, 0, 9], np.int32)
    active = td(np.r_[act, np.full(30, 1, np.int32)])
    n_active = td(np.array([3], np.int32))
    cand = torch.full((33 * k,), -7, dtype=torch.int32, device=dev())
    call("fwav_sim_topk_dim", emb.data_ptr(), embh.data_ptr(), nd, D, active.data_ptr(), n_active.data_ptr(), 33, 100, k,
         T, cand.data_ptr(), None, None, 0, stream())
    torch.cuda.synchronize()
    c = cand.cpu().numpy().reshape(33, k)
    for i in range(33):
        if i in act:
            assert np.array_equal(c[i], contract_topk(t @ t[100 + i], k)), i
        else:
            assert (c[i] == -7).all(), i


@pytest.mark.parametrize("nd", [14399, 14401])
def test_score_rows(nd):
    """fwav_score_rows_dim = numpy's ``emb @ q`` with this host's OpenBLAS thread count, on both sides of the threading
    threshold 32·nd = 460,800."""
    T = O.blas_threads()
    emb, _, rows = table_on_device("random", nd)[:3]
    t = table("random", nd)
    pick = np.array([0, 1, 77, 128, nd - 1], np.int32)
    S = torch.empty(len(pick) * nd, dtype=torch.float32, device=dev())
    call("fwav_score_rows_dim", emb.data_ptr(), nd, D, td(pick).data_ptr(), len(pick), 0, T, S.data_ptr(), stream())
    torch.cuda.synchronize()
    S = S.cpu().numpy().reshape(len(pick), nd)
    for j, r in enumerate(pick):
        ref = rows[r] if r < len(rows) else t @ t[r]
        bad = np.flatnonzero(S[j].view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, (nd, T, int(r), bad[:8])


def test_tie_rows_resolved_with_numpys_order():
    """The duplicated-rows table through the tie path on 32-wide rows: fwav_sim_topk_dim → fwav_affine →
    fwav_tie_check_dim(exact_sets = 2, every listed query) → fwav.ties.resolve_rows(emb_dim=32): every candidate row is
    then numpy's own (numpy_topk_row of numpy's score row), tied rows included."""
    nd, nq, k, rs, T = 257, 129, 32, 8, O.blas_threads()
    emb, embh, rows = table_on_device("dups", nd)[:3]
    rng = np.random.default_rng(3)
    ranges = td(rng.normal(0, 0.3, nq * rs).astype(F32))
    pool = td(rng.normal(0, 0.3, nd * rs).astype(F32))
    active = td(np.arange(nq, dtype=np.int32))
    n_active = td(np.array([nq], np.int32))
    cand = torch.empty(nq * k, dtype=torch.int32, device=dev())
    tl = torch.empty(size_call("fwav_tie_list_size", nq), dtype=torch.int32, device=dev())
    st = stream()
    call("fwav_sim_topk_dim", emb.data_ptr(), embh.data_ptr(), nd, D, active.data_ptr(), n_active.data_ptr(), nq, 0, k,
         T, cand.data_ptr(), tl.data_ptr(), None, 0, st)
    outs = [torch.empty(nq, dtype=dt, device=dev()) for dt in (torch.int32, torch.float32, torch.float32, torch.uint8,
                                                                torch.float32)]
    call("fwav_affine", ranges.data_ptr(), nq, rs, cand.data_ptr(), k, pool.data_ptr(), nd, 16.0,
         *[t.data_ptr() for t in outs], st)
    resolve = torch.empty(nq + 1, dtype=torch.int32, device=dev())
    call("fwav_tie_check_dim", ranges.data_ptr(), nq, rs, cand.data_ptr(), k, pool.data_ptr(), nd, emb.data_ptr(), D, 0,
         T, tl.data_ptr(), nq, 2, resolve.data_ptr(), st)
    n_res = int(resolve[0].item())
    want = expected_ties(rows, k)
    assert n_res == len(want) > 0
    assert sorted(resolve[1:1 + n_res].cpu().tolist()) == sorted(want)
    ties.resolve_rows(resolve[1:1 + n_res], emb=emb, n_domains=nd, q_offset=0, k=k, threads=T, ranges=ranges,
                      range_size=rs, pool=pool, s_clip=16.0, cand=cand, outs=tuple(outs), stream=st, emb_dim=D)
    torch.cuda.synchronize()
    c = cand.cpu().numpy().reshape(nq, k)
    for i in range(nq):
        assert np.array_equal(c[i], O.numpy_topk_row(rows[i], k)), i
    # the match tuples of the re-ranked rows are the oracle's for those candidate rows
    idx, s, o, sym, err = O.affine(ranges.cpu().numpy().reshape(nq, rs), c, pool.cpu().numpy().reshape(nd, rs))
    for t, ref in zip(outs, (idx, s, o, sym, err)):
        assert bit_equal(t.cpu().numpy(), np.asarray(ref).astype(t.cpu().numpy().dtype))


# ------------------------------------------------------------------------------------------------ end to end
def fixture_tuples(g):
    return g["m_idx"], g["m_s"], g["m_o"], g["m_sym"], g["m_err"]


@functools.lru_cache(maxsize=None)
def compressed(case):
    g = fixture(case)
    p = g["p"]
    return api.compress_audio(g["signal"], p["framerate"], p["sampwidth"], tile_size=p["tile"], emb_dim=32, top_k=p["K"])


@pytest.mark.parametrize("case", CASES)
def test_compress_audio_emb_dim_32(case):
    """compress_audio(emb_dim=32, top_k=32) returns the reference's match tuples, the periodic signal (exact ties in
    every row) included, and decompress_audio of them is bit-equal to the oracle's decode of the fixture's tuples."""
    g = fixture(case)
    p = g["p"]
    matches, domains, n_ranges, rs, tile, step, thr, orig = compressed(case)
    assert (n_ranges, rs, tile, step, orig) == (p["n_ranges"], p["rs"], p["tile"], p["step"], p["original_len"])
    assert domains.shape == (p["n_domains"], rs)
    got = (matches.idx, matches.s, matches.o, matches.sym, matches.err)
    for nm, a, b in zip(("idx", "s", "o", "sym", "err"), got, fixture_tuples(g)):
        bad = np.flatnonzero(np.asarray(a) != np.asarray(b)) if nm in ("idx", "sym") else \
            np.flatnonzero(np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32))
        assert bad.size == 0, (case, nm, bad.size, bad[:8])
    rec = api.decompress_audio(matches, domains, n_ranges, rs, original_len=orig)
    want, _, _ = O.decode(g["m_idx"], g["m_s"], g["m_o"], g["m_sym"], O.domain_pool(g["signal"], tile, rs, step),
                          n_ranges, rs, original_len=orig)
    assert bit_equal(rec, want)


def test_numpy_rows_mode_gives_the_references_candidate_rows():
    """tie_order="numpy_rows" on the periodic signal: every candidate row, order included, is cpu_worker's."""
    g = fixture("periodic2048")
    p = g["p"]
    res = engine.compress_device(td(g["signal"]), p["tile"], p["K"], emb_dim=32, tie_order="numpy_rows",
                                 keep_intermediates=True)
    torch.cuda.synchronize()
    cand = res.cand.cpu().numpy().reshape(p["n_ranges"], p["K"])
    assert res.n_ties > 0 and res.n_resolved == res.n_ties
    assert np.array_equal(cand[g["cand_rows"]], g["cand_sub"])
    assert sha(cand) == str(g["cand_sha256"])
    assert res.emb.numel() == p["n_domains"] * D


@pytest.mark.parametrize("case", ["t2048", "t1024"])
def test_candidates_are_the_references(case):
    """The candidate rows of the default mode on a signal without a K-th place tie: cpu_worker's, bit for bit."""
    g = fixture(case)
    p = g["p"]
    res = engine.compress_device(td(g["signal"]), p["tile"], p["K"], emb_dim=32, tie_order="numpy_sets",
                                 keep_intermediates=True)
    torch.cuda.synchronize()
    cand = res.cand.cpu().numpy().reshape(p["n_ranges"], p["K"])
    same = np.array([set(a) == set(b) for a, b in zip(cand[g["cand_rows"]], g["cand_sub"])])
    assert same.all(), np.flatnonzero(~same)[:8]


def test_sub_block_and_deferred_paths():
    """The sliced search (sub_blocks) and the deferred tie resolution on 32-wide rows give the one-launch outputs."""
    g = fixture("periodic2048")
    p = g["p"]
    x = td(g["signal"])
    one = engine.compress_device(x, p["tile"], p["K"], emb_dim=32)
    sl = engine.compress_device(x, p["tile"], p["K"], emb_dim=32, sub_blocks=3)
    df = engine.compress_device(x, p["tile"], p["K"], emb_dim=32, defer_ties=True).wait()
    torch.cuda.synchronize()
    for other in (sl, df):
        for nm in ("idx", "s", "o", "sym", "err"):
            assert bit_equal(getattr(one, nm).cpu().numpy(), getattr(other, nm).cpu().numpy()), nm
    for nm, ref in zip(("idx", "s", "o", "sym", "err"), fixture_tuples(g)):
        assert bit_equal(getattr(one, nm).cpu().numpy(), ref), nm


def test_torch_free_host():
    """fwav.hipctypes.compress(emb_dim=32): the same tuples through HIP buffers and numpy alone."""
    from fwav import hipctypes
    for case in ("t4096", "periodic2048"):
        g = fixture(case)
        p = g["p"]
        r = hipctypes.compress(g["signal"], p["tile"], p["K"], energy_thresh=p["thr"], emb_dim=32)
        assert r["emb"].shape == (p["n_domains"], D)
        for nm, ref in zip(("idx", "s", "o", "sym", "err"), fixture_tuples(g)):
            assert bit_equal(r[nm], ref), (case, nm)


def test_cli_emb_dim(tmp_path):
    """``compress --emb-dim 32`` writes the .fwav whose bytes are save_compressed of the fixture's tuples."""
    from fwav.cli import main
    g = fixture("t2048")
    p = g["p"]
    wav = tmp_path / "a.wav"
    write_wav(str(wav), g["signal"], p["framerate"], p["sampwidth"])
    r = main(["compress", str(wav), str(tmp_path / "out"), "--tile", str(p["tile"]), "--emb-dim", "32"])
    assert "error" not in r, r
    from fwav.matches import MatchList
    ref = tmp_path / "ref.fwav"
    save_compressed(str(ref), MatchList(*fixture_tuples(g)), O.domain_pool(g["signal"], p["tile"], p["rs"], p["step"]),
                    p["rs"], p["framerate"], p["sampwidth"], p["tile"], p["step"], p["thr"], p["original_len"])
    assert open(r["output"], "rb").read() == open(ref, "rb").read()


def test_width_16_unchanged():
    """compress_audio(emb_dim=16) and compress_audio() return identical outputs: the oracle's 16-wide ones, which at
    range size 16 (where the wide rows hold coefficients the 16-wide ones drop) are not the 32-wide ones."""
    g = fixture("t4096")
    p = g["p"]
    a = api.compress_audio(g["signal"], p["framerate"], p["sampwidth"], tile_size=p["tile"], top_k=p["K"])
    b = api.compress_audio(g["signal"], p["framerate"], p["sampwidth"], tile_size=p["tile"], top_k=p["K"], emb_dim=16)
    for nm in ("idx", "s", "o", "sym", "err"):
        assert bit_equal(getattr(a[0], nm), getattr(b[0], nm)), nm
    assert bit_equal(a[1], b[1]) and a[2:] == b[2:]
    ref = O.compress(g["signal"], p["tile"], p["K"])
    assert bit_equal(a[0].idx, ref["idx"]) and bit_equal(a[0].err, ref["err"])
    assert not np.array_equal(a[0].idx, compressed("t4096")[0].idx)
