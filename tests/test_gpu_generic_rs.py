"""Every compress stage at range sizes other than 4, 8 and 16 — the runtime-sized branch of each kernel (k_embed<0>,
k_prune<0>, k_affine_any, k_tie_check<0> / pair_errors<0>, k_domain_pool, k_block_means<0>) — against the
reference's own outputs: tests/golden t8192 (rs 32, step 8), t5000 (rs 19, step 4, block 263) and t1300 (rs 5, step 1,
block 260), made by tests/golden/make_golden.py.  One test per stage, each fed the REFERENCE's inputs from the fixture,
so that a failure names its kernel.

Bars.  Voiced mask, ranges, pool, prune, search (on the reference's embedding), affine, decode: bit-exact.  The
embedding is not bit-exact at these sizes (an f64 matrix DCT instead of scipy's f32 pocketfft sequence), so it has two
bars of its own, neither taken from the code under test (test_embedding).  End to end the device is compared with the
oracle run on the DEVICE's embedding; how many tuples also equal the reference's is printed, not asserted.

Also here: k_tie_check<0> and the numpy tie fix-up on a periodic signal (exact ties in every query's top K + 1), and
the voiced detection's carry across more than 1024 blocks of 1024 frames."""
import functools

import numpy as np
import pytest

from golden_util import GENERIC_CASES, bit_equal, load, same_sets

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import engine, ties  # noqa: E402
from fwav._lib import call, size_call  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

F32 = np.float32
NAMES = ("idx", "s", "o", "sym", "err")


def dev():
    return torch.device("cuda", 0)


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def golden(case):
    return load(case)


def voiced_ranges(sig, rs, thr):
    """fwav_voiced_ranges → (ranges f32[nr, rs], mask u8[n])."""
    n = len(sig)
    frame = 2 * rs
    nr = -(-n // rs)
    x = td(sig)
    wsn = size_call("fwav_voiced_workspace_size", n, frame)
    ws = torch.empty(wsn, dtype=torch.uint8, device=dev())
    ranges = torch.empty(nr * rs, dtype=torch.float32, device=dev())
    mask = torch.empty(n, dtype=torch.uint8, device=dev())
    call("fwav_voiced_ranges", x.data_ptr(), n, rs, frame, 5, float(F32(thr)), float(F32(thr * 0.5)),
         ranges.data_ptr(), nr, mask.data_ptr(), ws.data_ptr(), wsn, stream())
    torch.cuda.synchronize()
    return ranges.cpu().numpy().reshape(nr, rs), mask.cpu().numpy()


@pytest.mark.parametrize("case", GENERIC_CASES)
def test_voiced_and_ranges(case):
    g = golden(case)
    p = g["p"]
    assert 2 * p["rs"] in (64, 38, 10)
    ranges, mask = voiced_ranges(g["signal"], p["rs"], p["thr"])
    assert np.array_equal(mask, g["voiced"])
    assert bit_equal(ranges, g["ranges"])
    assert p["original_len"] % p["rs"] != 0  # ragged: the last range is reflect-padded


@functools.lru_cache(maxsize=None)
def device_pool_embed(case):
    """fwav_pool_embed on the case's signal → (pool f32[nd, rs], emb f32[nd, 16], emb16 f16[...]), computed once."""
    g = golden(case)
    p = g["p"]
    tile, rs, step = p["tile"], p["rs"], p["step"]
    sig = td(g["signal"])
    n = sig.numel()
    nd = (n - tile) // step + 1
    assert nd == p["n_domains"]
    tab = engine.embed_tables(rs, dev())
    pool = torch.empty(nd * rs, dtype=torch.float32, device=dev())
    emb = torch.empty(nd * 16, dtype=torch.float32, device=dev())
    emb16 = torch.empty(size_call("fwav_emb16_elems", nd), dtype=torch.float16, device=dev())
    wsn = size_call("fwav_pool_workspace_size", n, tile, rs, step)
    ws = torch.empty(max(wsn, 16), dtype=torch.uint8, device=dev())
    call("fwav_pool_embed", sig.data_ptr(), n, tile, rs, step, tab.data_ptr(), pool.data_ptr(), emb.data_ptr(),
         emb16.data_ptr(), ws.data_ptr(), wsn, stream())
    torch.cuda.synchronize()
    return pool.cpu().numpy().reshape(nd, rs), emb.cpu().numpy().reshape(nd, 16), emb16.cpu().numpy()


@pytest.mark.parametrize("case", GENERIC_CASES)
def test_pool(case):
    """t5000: k_domain_pool (block 263 — more than one 128-element pairwise leaf — does not divide by step 4, and the 3
    samples tile % rs leaves over are dropped); t8192: k_block_means<256>; t1300: k_block_means<0>, block 260."""
    g = golden(case)
    p = g["p"]
    bl = p["tile"] // p["rs"]
    assert (bl, bl % p["step"] != 0, p["tile"] - bl * p["rs"]) == {"t8192": (256, False, 0), "t5000": (263, True, 3),
                                                                     "t1300": (260, False, 0)}[case]
    pool, _, _ = device_pool_embed(case)
    assert bit_equal(pool, g["pool"])


def f64_tonal(pool):
    """The exactly rounded tonal head (fractal.py:178-208 in f64): → (head f64[nd, 8], un-normalised norm f64[nd])."""
    import scipy.fftpack
    nd, rs = pool.shape
    v = scipy.fftpack.dct(pool.astype(np.float64), norm="ortho", axis=-1) * np.linspace(1.0, 2.0, rs)
    take = min(8, rs - 1)
    e = np.zeros((nd, 8))
    e[:, :take] = v[:, 1:1 + take]
    nrm = np.sqrt((e * e).sum(1))
    ok = nrm > 1e-8
    e[ok] /= nrm[ok, None]
    return e, nrm


@pytest.mark.parametrize("case", GENERIC_CASES)
def test_embedding(case):
    """k_embed<0>.  (1) Tonal columns 0-7 against the f64 embedding of the reference's pool: |Δ| ≤ 2⁻²² (three f32
    roundings — the cast of the f64 DCT, the sdot-order norm, the divide — on values of magnitude ≤ 1).  Rows whose f64
    un-normalised tonal norm lies in (0, 1e-6) are left out (near the 1e-8 switch the two sides may normalise
    differently; their share must stay ≤ 1 %) but must be finite with magnitude ≤ 1 + 2⁻²².  (2) Transient columns
    8-15 against the reference's: |Δ| ≤ 2⁻²³ (both sides f64 until one final rounding).  emb16 is the fp16 table of
    the device's own embedding."""
    g = golden(case)
    _, emb, emb16 = device_pool_embed(case)
    ref, nrm = f64_tonal(g["pool"])
    out = (nrm > 0) & (nrm < 1e-6)
    share = out.mean()
    d_ref = np.abs(emb[:, :8].astype(np.float64) - ref)
    d_gold = np.abs(emb[:, :8].astype(np.float64) - g["emb"][:, :8].astype(np.float64)).max()
    d_tr = np.abs(emb[:, 8:].astype(np.float64) - g["emb"][:, 8:].astype(np.float64))
    tr_equal = (emb[:, 8:].view(np.uint32) == g["emb"][:, 8:].view(np.uint32)).all(axis=1).mean()
    print(f"{case}: tonal max |device - f64| = {d_ref[~out].max():.3e} (bar {2.0 ** -22:.3e}), tonal max |device - "
          f"reference| = {d_gold:.3e}, left out {int(out.sum())}/{len(out)} rows, transient max |device - reference| "
          f"= {d_tr.max():.3e}, transient rows bit-equal {100 * tr_equal:.2f} %")
    assert share <= 0.01, (int(out.sum()), len(out))
    assert np.isfinite(emb).all()
    assert np.abs(emb[out]).max(initial=0.0) <= 1 + 2.0 ** -22
    assert d_ref[~out].max() <= 2.0 ** -22
    assert d_tr.max() <= 2.0 ** -23
    # the fp16 pre-filter's error bound assumes heads of norm ≤ 1 (the bar of
    # test_oracle_golden.test_embedding_heads_at_most_unit_norm, here on the device's rows)
    for head in (emb[:, :8].astype(np.float64), emb[:, 8:].astype(np.float64)):
        assert np.sqrt((head ** 2).sum(1)).max() <= 1 + 1e-6
    e16 =torch.empty(size_call("fwav_emb16_elems", len(emb)), dtype=torch.float16, device=dev())
    e = td(emb.reshape(-1))
    call("fwav_emb16_from_emb", e.data_ptr(), len(emb), e16.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(e16.cpu().numpy().view(np.uint16), emb16.view(np.uint16))


def prune(ranges, emb, K, thr, q_offset=0, fast_mode=1, zero_cand="numpy"):
    """fwav_prune → (cand i32[n, K] with −7 where the kernel wrote nothing, active i32[n_active] as written, n_active)."""
    n, rs = ranges.shape
    nd = len(emb)
    r, e = td(ranges.reshape(-1)), td(emb.reshape(-1))
    zc = td(engine.zero_query_candidates(nd, K)) if zero_cand == "numpy" else None
    cand = torch.full((n * K,), -7, dtype=torch.int32, device=dev())
    active = torch.full((n,), -7, dtype=torch.int32, device=dev())
    n_active = torch.full((1,), -7, dtype=torch.int32, device=dev())
    call("fwav_prune", r.data_ptr(), n, q_offset, rs, float(F32(thr)), fast_mode, e.data_ptr(), nd, K,
         None if zc is None else zc.data_ptr(), cand.data_ptr(), active.data_ptr(), n_active.data_ptr(), stream())
    torch.cuda.synchronize()
    na = int(n_active.item())
    return cand.cpu().numpy().reshape(n, K), active.cpu().numpy(), na


@pytest.mark.parametrize("case", GENERIC_CASES)
def test_prune(case):
    """k_prune<0> on the reference's ranges and embedding: the pruned rows are the reference's all-(−1) rows; `active`
    holds exactly the others (all-zero query embeddings aside, which take numpy's zero-score row)."""
    g = golden(case)
    p = g["p"]
    for K in p["Ks"]:
        gold = g[f"cand_{K}"]
        nr = len(gold)
        cand, active, na = prune(g["ranges"], g["emb"], K, p["thr"] * 0.75)
        pruned = gold[:, 0] < 0
        zero = ~pruned & np.all(g["emb"][:nr] == 0, axis=1)
        assert np.array_equal((cand == -1).all(axis=1), pruned)
        assert (cand[zero] == engine.zero_query_candidates(len(g["emb"]), K)).all()
        assert (cand[~pruned & ~zero] == -7).all()  # searchable rows: left to fwav_sim_topk
        assert na == int((~pruned & ~zero).sum())
        assert np.array_equal(np.sort(active[:na]), np.nonzero(~pruned & ~zero)[0])
        assert (active[na:] == -7).all()
        print(f"{case} K={K}: {int(pruned.sum())}/{nr} pruned, {int(zero.sum())} zero queries, {na} active")


@pytest.mark.parametrize("rs", [5, 19, 32])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_prune_synthetic(rs, n):
    """k_prune<0> against numpy's own np.mean(r ** 2) < thr (fractal.py:602): a row whose mean square equals the
    threshold exactly is kept; fast_mode = 0 prunes nothing; an all-zero query embedding takes zero_cand, or
    0 .. K−1 (−1 past n_domains) when zero_cand is NULL; q_offset > 0; row counts around the 64-lane waves."""
    rng = np.random.default_rng(100 * rs + n)
    K, q_offset, thr = 8, 3, F32(0.25)
    ranges = rng.normal(0, 0.5, (n, rs)).astype(F32)  # mean square ≈ thr: about half pruned
    ranges[0] = 0.5                                   # mean(r²) = 0.25 = thr exactly: not < thr
    if n > 7:
        ranges[5] = 1.0
        ranges[7] = 0.5
        ranges[7, rs // 2] = np.nextafter(F32(0.5), F32(0))
    nd = q_offset + n + 2  # n = 1: 6 domains < K, so the NULL zero_cand row is −1 padded
    emb = rng.normal(0, 0.3, (nd, 16)).astype(F32)
    if n > 7:
        emb[q_offset + 5] = 0   # the query row of range 5 (kept: mean square 1)
        emb[5] = 1              # not a query row here: q_offset must be applied
    else:
        emb[q_offset] = 0
    want = np.array([np.mean(r ** 2) < thr for r in ranges])
    assert not want[0] and (n <= 7 or not want[5])
    zq = np.all(emb[q_offset:q_offset + n] == 0, axis=1)
    for fast in (1, 0):
        pr = want if fast else np.zeros(n, bool)
        for zc in ("numpy", None):
            cand, active, na = prune(ranges, emb, K, thr, q_offset=q_offset, fast_mode=fast, zero_cand=zc)
            assert np.array_equal((cand == -1).all(axis=1), pr), (fast, zc)
            zrow = engine.zero_query_candidates(nd, K) if zc else np.where(np.arange(K) < nd, np.arange(K), -1)
            assert (~pr & zq).sum() == 1 and (cand[~pr & zq] == zrow).all(), (fast, zc)
            act = ~pr & ~zq
            assert (cand[act] == -7).all()
            assert na == int(act.sum()) and np.array_equal(np.sort(active[:na]), np.nonzero(act)[0]), (fast, zc)


def solve(ranges, cand, pool, s_clip=16.0):
    nr, rs = ranges.shape
    K = cand.shape[1]
    out = [torch.empty(nr, dtype=dt, device=dev()) for dt in
           (torch.int32, torch.float32, torch.float32, torch.uint8, torch.float32)]
    r, c, pl = td(ranges.reshape(-1)), td(cand.reshape(-1)), td(pool.reshape(-1))
    call("fwav_affine", r.data_ptr(), nr, rs, c.data_ptr(), K, pl.data_ptr(), len(pool), s_clip,
         *[t.data_ptr() for t in out], stream())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("case", GENERIC_CASES)
def test_affine(case):
    """k_affine_any at rs 32, 19 (K = 64 and 17) and 5 on the reference's ranges, candidates and pool."""
    g = golden(case)
    for K in g["p"]["Ks"]:
        got = solve(g["ranges"], g[f"cand_{K}"], g["pool"])
        for nm, a in zip(NAMES, got):
            assert bit_equal(a, g[f"m_{nm}_{K}"]), f"{case} K={K} {nm}"


@pytest.mark.parametrize("case", GENERIC_CASES)
def test_search_on_reference_embedding(case):
    """fwav_emb16_from_emb(the reference's embedding) → fwav_prune → fwav_sim_topk(blas_threads = 8) → fwav_affine →
    fwav_tie_check(exact_sets = 1) → the numpy fix-up of the rows it lists (the product's sequence, fed the reference's
    arrays): the reference's candidate set for every row, its order wherever the row's scores are distinct (the rule of
    test_gpu_parity.test_candidates_and_matches), and its match tuples."""
    g = golden(case)
    p = g["p"]
    rs, nd = p["rs"], p["n_domains"]
    emb, pool, ranges = td(g["emb"].reshape(-1)), td(g["pool"].reshape(-1)), td(g["ranges"].reshape(-1))
    emb16 = torch.empty(size_call("fwav_emb16_elems", nd), dtype=torch.float16, device=dev())
    call("fwav_emb16_from_emb", emb.data_ptr(), nd, emb16.data_ptr(), stream())
    for K in p["Ks"]:
        gold = g[f"cand_{K}"]
        nr = len(gold)
        zc = td(engine.zero_query_candidates(nd, K))
        cand = torch.full((nr * K,), -7, dtype=torch.int32, device=dev())
        active = torch.empty(nr, dtype=torch.int32, device=dev())
        n_active = torch.zeros(1, dtype=torch.int32, device=dev())
        call("fwav_prune", ranges.data_ptr(), nr, 0, rs, float(F32(p["thr"] * 0.75)), 1, emb.data_ptr(), nd, K,
             zc.data_ptr(), cand.data_ptr(), active.data_ptr(), n_active.data_ptr(), stream())
        wk = size_call("fwav_sim_topk_workspace_size", nr, nd, K)
        ws = torch.empty(max(wk, 16), dtype=torch.uint8, device=dev())
        tl = torch.empty(size_call("fwav_tie_list_size", nr), dtype=torch.int32, device=dev())
        call("fwav_sim_topk", emb.data_ptr(), emb16.data_ptr(), nd, active.data_ptr(), n_active.data_ptr(), nr, 0, K, 8,
             cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, stream())
        outs = tuple(torch.empty(nr, dtype=dt, device=dev()) for dt in
                     (torch.int32, torch.float32, torch.float32, torch.uint8, torch.float32))
        call("fwav_affine", ranges.data_ptr(), nr, rs, cand.data_ptr(), K, pool.data_ptr(), nd, 16.0,
             *[t.data_ptr() for t in outs], stream())
        resolve = torch.empty(nr + 1, dtype=torch.int32, device=dev())
        call("fwav_tie_check", ranges.data_ptr(), nr, rs, cand.data_ptr(), K, pool.data_ptr(), nd, emb.data_ptr(), 0, 8,
             tl.data_ptr(), nr, 1, resolve.data_ptr(), stream())
        n_ties, n_res = int(tl[0].item()), int(resolve[0].item())
        if n_res:
            ties.resolve_rows(resolve[1:1 + n_res], emb=emb, n_domains=nd, q_offset=0, k=K, threads=8, ranges=ranges,
                              range_size=rs, pool=pool, s_clip=16.0, cand=cand, outs=outs, stream=stream())
        torch.cuda.synchronize()
        c = cand.cpu().numpy().reshape(nr, K)
        bad = np.nonzero(~same_sets(c, gold))[0]
        assert len(bad) == 0, f"{case} K={K}: candidate sets differ on rows {bad[:10]}"
        distinct = 0
        for i in range(nr):
            cg = gold[i][gold[i] >= 0]
            if len(cg) == 0:
                continue
            sc = O.sgemv_scores(g["emb"][cg], g["emb"][i][None, :], O.sgemv_col_kind(cg, nd, 8))[0]
            if len(np.unique(sc)) == len(sc):
                distinct += 1
                assert np.array_equal(c[i], gold[i]), f"{case} K={K} row {i}"
        for nm, t in zip(NAMES, outs):
            assert bit_equal(t.cpu().numpy(), g[f"m_{nm}_{K}"]), f"{case} K={K} {nm}"
        print(f"{case} K={K}: {n_ties} rows with exact ties, {n_res} re-ranked by numpy; {distinct} rows with distinct "
              f"scores in the reference's order")


@pytest.mark.parametrize("case", GENERIC_CASES)
def test_decode(case):
    from fwav.api import decompress_audio
    from fwav.matches import MatchList
    g = golden(case)
    p = g["p"]
    for K in p["Ks"]:
        m = MatchList(g[f"m_idx_{K}"], g[f"m_s_{K}"], g[f"m_o_{K}"], g[f"m_sym_{K}"], g[f"m_err_{K}"])
        nr = len(m)
        d, info = decompress_audio(m, g["pool"], nr, p["rs"], original_len=p["original_len"], return_info=True)
        assert bit_equal(d, g[f"dec_{K}"])
        assert info["iterations"] == int(g[f"dec_iters_{K}"])
        d = decompress_audio(m, g["pool"], nr, p["rs"], iterations=50, convergence_eps=0.0,
                             original_len=p["original_len"])
        assert bit_equal(d, g[f"dec50_{K}"])
        d, info = decompress_audio(m, g["pool"], nr, p["rs"], iterations=12, convergence_eps=0.0, s_damping=0.3,
                                   original_len=p["original_len"], return_info=True)
        assert bit_equal(d, g[f"decd_{K}"])
        assert info["iterations"] == int(g[f"decd_iters_{K}"])
        np.testing.assert_allclose(info["deltas"], g[f"decd_deltas_{K}"], rtol=1e-5)


def self_consistent(sig, tile, K, thr=1e-4, label=""):
    """engine.compress_device against the oracle run on the DEVICE's embedding (the way tests/test_gpu_oracle_rows.py
    calls it): every match tuple equals O.affine(ranges, O.topk_candidates(device emb), pool) bit for bit.  → (result,
    the oracle's candidate rows, the device's tuples on the host)."""
    r = engine.compress_device(td(sig), tile, K, energy_thresh=thr, keep_intermediates=True)
    torch.cuda.synchronize()
    rs = r.range_size
    ranges = r.ranges.cpu().numpy().reshape(-1, rs)
    pool = r.pool.cpu().numpy().reshape(-1, rs)
    emb = r.emb.cpu().numpy().reshape(-1, 16)
    pruned = O.range_energy_pruned(ranges, thr)
    ocand, _, _ = O.topk_candidates(emb, len(ranges), K, pruned, threads=ties.blas_threads())
    want = O.affine(ranges, ocand, pool)
    got = [getattr(r, nm).cpu().numpy() for nm in NAMES]
    for nm, a, b in zip(NAMES, got, want):
        bad = np.nonzero(np.asarray(a).view(np.uint8).reshape(len(a), -1)
                         != np.asarray(b).view(np.uint8).reshape(len(a), -1))[0]
        assert len(bad) == 0, f"{label} K={K} {nm}: rows {np.unique(bad)[:10]} differ from the oracle on the device's embedding"
    return r, ocand, got


@pytest.mark.parametrize("case", GENERIC_CASES)
def test_end_to_end_self_consistent(case):
    g = golden(case)
    p = g["p"]
    for K in p["Ks"]:
        r, ocand, got = self_consistent(g["signal"], p["tile"], K, p["thr"], case)
        rs = p["rs"]
        assert bit_equal(r.ranges.cpu().numpy().reshape(-1, rs), g["ranges"])
        assert bit_equal(r.pool.cpu().numpy().reshape(-1, rs), g["pool"])
        same = np.ones(len(got[0]), bool)
        for nm, a in zip(NAMES, got):
            same &= (a.view(np.uint8).reshape(len(a), -1) == g[f"m_{nm}_{K}"].view(np.uint8).reshape(len(a), -1)).all(1)
        sets = same_sets(r.cand.cpu().numpy().reshape(-1, K), g[f"cand_{K}"])
        print(f"{case} K={K}: {int(same.sum())}/{len(same)} tuples and {int(sets.sum())}/{len(sets)} candidate sets "
              f"equal the reference's; {r.n_ties} rows with exact ties, {r.n_resolved} re-ranked by numpy")


@pytest.mark.parametrize("n,tile", [(6_000, 1300), (40_000, 8192)])
def test_ties_at_a_runtime_range_size(n, tile):
    """k_tie_check<0> / pair_errors<0> and the numpy fix-up at rs 5 and 32: a periodic signal (period 96) gives every
    query exact ties in its top 33; the tuples still equal the oracle's on the device's embedding, and some rows had
    to be re-ranked with numpy's order."""
    from test_gpu_parity import _periodic
    sig = _periodic(n)
    K = 32
    r, ocand, _ = self_consistent(sig, tile, K, label=f"periodic tile {tile}")
    emb = r.emb.cpu().numpy().reshape(-1, 16)
    assert not np.all(emb == 0, axis=1).any()
    assert r.range_size == max(4, tile // 256) and r.range_size not in (4, 8, 16)
    searched = ocand[:, 0] >= 0
    assert searched.any() and r.n_ties == int(searched.sum())  # every searched query has exact ties in its top K + 1
    assert r.n_resolved > 0
    print(f"periodic tile {tile}: {r.n_ranges} ranges, {r.n_ties} with exact ties, {r.n_resolved} re-ranked by numpy")


def test_voiced_carry_beyond_1024_blocks():
    """k_voiced_carry scans the per-block last decisive frames 1024 blocks at a time: a signal of 1027 blocks of 1024
    frames (rs 4, frame 8) makes it loop a second time with a running state.  Frames sit between lo and hi (they keep
    the state) except a burst at the start (voiced), a zero dip in block 1025 (unvoiced) and a burst in block 1026
    (voiced again) — so the state of blocks 1024 .. 1026 comes out of the first pass's carry."""
    rs, frame, thr = 4, 8, 1e-4
    nf = 1027 * 1024 + 5
    rng = np.random.default_rng(8)
    amp = np.full(nf, np.sqrt(7.5e-5))
    amp[:40] = 0.05
    amp[1024 * 1025 + 7:1024 * 1025 + 31] = 0.0
    amp[1024 * 1026 + 500:1024 * 1026 + 521] = 0.05
    sig = (np.repeat(amp, frame) * rng.choice([-1.0, 1.0], nf * frame)).astype(F32)
    vm = O.voiced_detection(sig, frame, thr)
    flips = np.nonzero(np.diff(vm[::frame].astype(np.int8)))[0]
    assert flips.tolist() == [1049605, 1051121, 1051651]
    want, _ = O.form_ranges(sig, vm, rs)
    ranges, mask = voiced_ranges(sig, rs, thr)
    assert np.array_equal(mask, vm)
    assert bit_equal(ranges, want)
