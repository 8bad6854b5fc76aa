"""compress_audio(candidates="all") on the device: fwav_affine_all against fwav_affine_fit on the candidate row
0 … n_domains − 1 and against the numpy restatement (tests/fit_all.py), then the pipeline.

Bar: the five outputs bit for bit — every value by its raw bits, except that a NaN matches any NaN
(AE.same_bits_or_nan, the bar of every affine test here).  Which NaN an invalid sum carries, its sign and payload,
follows the operand order the compiler picks for each commutative add: it differs between x86 numpy and the device,
and on the overflowing edge tile between fwav_affine_all and fwav_affine_fit too (measured: the NaN positions agree
on every row, ten rows of the rs 4 table differ in the NaN's bits), as it may between fwav_affine_fit's own kernels.
The one tolerance is the round trip's 0.05 dB (tests/test_gpu_fit_clipped.py: the README's
observed 0.01 dB on eight cells, with room for a ninth)."""
import numpy as np
import pytest

import affine_edges as AE
import fit_all as FA
import fit_clipped as FC

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import api, engine, synth  # noqa: E402
from fwav._lib import call, size_call  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

DEV = torch.device("cuda", 0)
F32 = np.float32
NAMES = FA.NAMES
OUT_DTYPES = (torch.int32, torch.float32, torch.float32, torch.uint8, torch.float32)
GUARD, GUARD_BYTES = 0xA5, 4096


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def solve_all(ranges, pool, fit, s_clip=16.0, active=None, n_active=None, outs=None, ws=None):
    """fwav_affine_all on device tensors → the five outputs as numpy arrays (``outs`` / ``ws``: the caller's)."""
    n, rs = ranges.shape
    nd = len(pool)
    r, p = td(ranges.reshape(-1)), td(pool.reshape(-1))
    if outs is None:
        outs = [torch.empty(n, dtype=dt, device=DEV) for dt in OUT_DTYPES]
    wn = size_call("fwav_affine_all_workspace_size", n, nd, rs)
    if ws is None:
        ws = torch.empty(max(wn, 16), dtype=torch.uint8, device=DEV)
    call("fwav_affine_all", r.data_ptr(), n, rs, None if active is None else active.data_ptr(),
         None if n_active is None else n_active.data_ptr(), n, p.data_ptr(), nd, float(s_clip),
         *[t.data_ptr() for t in outs], fit, ws.data_ptr(), wn, stream())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def solve_fit(ranges, pool, fit, s_clip=16.0):
    """fwav_affine_fit with K = n_domains and the candidate row 0 … n_domains − 1 for every range."""
    n, rs = ranges.shape
    nd = len(pool)
    r, p = td(ranges.reshape(-1)), td(pool.reshape(-1))
    cand = torch.arange(nd, dtype=torch.int32, device=DEV).repeat(n)
    outs = [torch.empty(n, dtype=dt, device=DEV) for dt in OUT_DTYPES]
    call("fwav_affine_fit", r.data_ptr(), n, rs, cand.data_ptr(), nd, p.data_ptr(), nd, float(s_clip),
         *[t.data_ptr() for t in outs], fit, stream())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def assert_restated(got, want, what, rows=None):
    for nm, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w).astype(np.asarray(g).dtype)
        if rows is not None:
            g, w = g[rows], w[rows]
        bad = [i for i in range(len(g)) if not AE.same_bits_or_nan(g[i:i + 1], w[i:i + 1])]
        assert not bad, (what, nm, [(i, g[i], w[i]) for i in bad[:5]])


# ------------------------------------------------------------------------------------- 1. against the existing kernel
@pytest.mark.parametrize("fit", (0, 1), ids=FA.FIT_NAMES)
@pytest.mark.parametrize("rs", (4, 8, 16, 5, 19, 32))
def test_equals_affine_fit_on_every_domain(rs, fit):
    """n_domains around the LDS tile T and the 64-lane dispatch of fwav_affine_fit, n_ranges around the workgroup's
    256: each call equals fwav_affine_fit(K = n_domains, cand = arange) and the restatement."""
    T = size_call("fwav_affine_all_tile_rows", rs)
    cap = size_call("fwav_topk_max_k")
    nds = sorted({min(nd, cap) for nd in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 4096)})
    rng = np.random.default_rng(100 * rs + fit)
    ranges = rng.normal(0, 0.3, (257, rs)).astype(F32)
    pool = rng.normal(0, 0.3, (max(nds), rs)).astype(F32)
    for nd in nds:
        want = FA.affine_all(ranges, pool[:nd], fit)  # once per table: rows are independent
        for n in (1, 255, 256, 257):
            got = solve_all(ranges[:n], pool[:nd], fit)
            assert_restated(got, solve_fit(ranges[:n], pool[:nd], fit), (rs, fit, nd, n))
            assert_restated(got, [w[:n] for w in want], (rs, fit, nd, n))


# ------------------------------------------------------------------------------------------------------ 2. edge rows
def edge_inputs(rs):
    """tests/affine_edges.build's pool and ranges with fit_clipped.twin_rows' patch (two indices holding bit-identical
    tiles, a twin pair of palindromes) and its ranges appended."""
    ranges, _, pool, _ = AE.build(rs, 1)
    tr, _, patch = FC.twin_rows(rs, 1)
    pool = pool.copy()
    for dst, src in patch.items():
        pool[dst] = pool[src]
    return np.concatenate([ranges, tr]), pool


@pytest.mark.parametrize("fit", (0, 1), ids=FA.FIT_NAMES)
@pytest.mark.parametrize("rs", (4, 8, 16, 5, 19))
def test_edge_tiles_with_every_domain_a_candidate(rs, fit):
    """The whole pool (its NaN tile then wins every row: the first NaN error), and its prefixes that end before the
    NaN, the inf and the overflowing tile, so that the constant tile (den = 1e-12), the mirror pair, the palindromes
    and the twins decide rows too; s_clip 16 and one that binds."""
    ranges, pool = edge_inputs(rs)
    for nd in (AE.P_BIG, AE.P_INF, AE.P_NAN, AE.N_POOL):
        for sc in (16.0, 0.5):
            got = solve_all(ranges, pool[:nd], fit, sc)
            assert_restated(got, solve_fit(ranges, pool[:nd], fit, sc), (rs, fit, nd, sc))
            assert_restated(got, FA.affine_all(ranges, pool[:nd], fit, sc), (rs, fit, nd, sc))
    assert np.isnan(got[4]).all()  # the last call held the NaN tile


# --------------------------------------------------------------------------------------------------- 3. domain split
@pytest.mark.parametrize("fit", (0, 1), ids=FA.FIT_NAMES)
@pytest.mark.parametrize("rs", (8, 19))
def test_domain_split_merges_in_the_same_order(rs, fit):
    n, nd = 8, 70000
    assert size_call("fwav_affine_all_slices", n, nd, rs) > 1  # the merge kernel runs
    rng = np.random.default_rng(7 + rs)
    pool = rng.normal(0, 0.3, (nd, rs)).astype(F32)
    ranges = rng.normal(0, 0.3, (n, rs)).astype(F32)
    h = rs // 2
    pool[9, rs - h:] = pool[9, :h][::-1]          # a palindrome …
    pool[nd - 2] = pool[9]                        # … and its twin in the last slice
    pool[nd - 3] = pool[5]                        # a plain row's twin in the last slice
    ranges[0] = F32(1.5) * pool[5] + F32(0.25)    # fits rows 5 and nd − 3 alike: the smaller index
    ranges[1] = F32(-0.75) * pool[9] + F32(0.5)   # fits four slots alike: row 9, unmirrored
    ranges[2] = F32(np.nan)                       # every error NaN: the first slot
    ranges[3] = F32(2.0) * pool[nd - 1][::-1]     # the winner is the last row, mirrored
    got = solve_all(ranges, pool, fit)
    assert_restated(got, FA.affine_all(ranges, pool, fit), (rs, fit))
    idx, _, _, sym, err = got
    assert (idx[0], sym[0]) == (5, 0) and (idx[1], sym[1]) == (9, 0) and (idx[3], sym[3]) == (nd - 1, 1)
    assert (idx[2], sym[2]) == (0, 0) and np.isnan(err[2])


# ------------------------------------------------------------------------------- 4. active list and buffer guards
@pytest.mark.parametrize("fit", (0, 1), ids=FA.FIT_NAMES)
@pytest.mark.parametrize("rs,nd", [(8, 300), (8, 3000), (19, 1000)])
def test_active_list_and_guards(rs, nd, fit):
    """Every third row, descending, with fewer listed than max_q: listed rows are right, every other row and the
    4 KiB after each output and after a workspace of exactly fwav_affine_all_workspace_size bytes keep the pattern."""
    n = 100
    rng = np.random.default_rng(rs + nd)
    ranges = rng.normal(0, 0.3, (n, rs)).astype(F32)
    pool = rng.normal(0, 0.3, (nd, rs)).astype(F32)
    listed = np.arange(n - 1, -1, -3, dtype=np.int32)
    act = np.full(n, 1, np.int32)              # (row 1 is not listed: an entry past *n_active must not be read as one)
    act[:len(listed)] = listed
    assert 1 not in listed and len(listed) < n
    wn = size_call("fwav_affine_all_workspace_size", n, nd, rs)
    assert (wn > 0) == (nd > 300)              # both the direct store and the split launch are covered
    bufs = [torch.full((n * torch.empty(0, dtype=dt).element_size() + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=DEV)
            for dt in OUT_DTYPES]
    outs = [b[:n * torch.empty(0, dtype=dt).element_size()].view(dt) for b, dt in zip(bufs, OUT_DTYPES)]
    ws = torch.full((wn + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=DEV)
    got = solve_all(ranges, pool, fit, active=td(act), n_active=td(np.array([len(listed)], np.int32)), outs=outs, ws=ws)
    want = FA.affine_all(ranges[listed], pool, fit)
    assert_restated([g[listed] for g in got], want, (rs, nd, fit))
    others = np.setdiff1d(np.arange(n), listed)
    for nm, g, b in zip(NAMES, got, bufs):
        assert np.all(raw(g[others]) == GUARD), nm
        assert np.all(b[-GUARD_BYTES:].cpu().numpy() == GUARD), nm
    assert np.all(ws[wn:].cpu().numpy() == GUARD)


# -------------------------------------------------------------------------------------------------------- 5. pipeline
TILE, SR = 1024, 16000
_SIG: dict = {}


def signal(silent=False):
    if silent not in _SIG:
        s = synth.speech_like(0.25, SR)
        _SIG[silent] = np.concatenate([np.zeros(600, F32), s]) if silent else s
    return _SIG[silent]


def arrays(m):
    return tuple(np.asarray(getattr(m, f)) for f in NAMES)


_OUT: dict = {}


def compressed(fit, **kw):
    key = (fit, tuple(sorted(kw.items())))
    if key not in _OUT:
        _OUT[key] = api.compress_audio(signal(), SR, 2, tile_size=TILE, fit=FA.FIT_NAMES[fit], **kw)
    return _OUT[key]


@pytest.mark.parametrize("silent", (False, True), ids=("speech", "silence+speech"))
@pytest.mark.parametrize("fit", (0, 1), ids=FA.FIT_NAMES)
def test_pipeline_equals_the_restatement(fit, silent):
    sig = signal(silent)
    c = FA.restate_compress_all(sig, TILE, fit)
    out = (compressed(fit, candidates="all") if not silent else
           api.compress_audio(sig, SR, 2, tile_size=TILE, fit=FA.FIT_NAMES[fit], candidates="all"))
    matches, domains, nr, rs, _, step, _, orig = out
    assert (nr, rs, step, orig) == (len(c["ranges"]), c["rs"], c["step"], len(sig))
    assert np.array_equal(domains.view(np.uint32), c["pool"].view(np.uint32))
    assert c["pruned"].any() and not c["pruned"].all()
    assert_restated(arrays(matches), c["m"], ("kept", fit, silent), rows=~c["pruned"])
    assert_restated(arrays(matches), c["m"], ("pruned", fit, silent), rows=c["pruned"])


@pytest.mark.parametrize("fit", (0, 1), ids=FA.FIT_NAMES)
def test_compact_and_shard_compose(fit):
    full = compressed(fit, candidates="all")
    cm, cd, nr, rs, *_ = compressed(fit, candidates="all", compact=True)
    assert len(cd) == len(np.unique(np.asarray(full[0].idx))) < len(full[1])
    a = api.decompress_audio(full[0], full[1], nr, rs, s_damping=1e-6)
    b = api.decompress_audio(cm, cd, nr, rs, s_damping=1e-6)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    lo, hi = 130, 777
    r = engine.compress_device(td(signal()), TILE, 32, fit=FA.FIT_NAMES[fit], candidates="all", shard=(lo, hi))
    torch.cuda.synchronize()
    assert r.cand is None and (r.n_ties, r.n_resolved) == (0, 0) and tuple(r.shard) == (lo, hi)
    assert_restated([getattr(r, nm).cpu().numpy() for nm in NAMES], [w[lo:hi] for w in arrays(full[0])], ("shard", fit))


def test_round_trip_decodes_to_the_fit_and_beats_the_embedding_path(tmp_path):
    """Save, load, decompress_audio(s_damping=1e-6) with fit="clipped": over the searched ranges the decoded SNR against
    the voiced-masked ranges is within 0.05 dB of the fit SNR 10·log10(Σ‖r‖² / Σ err²), and at least the figure of
    candidates="embedding" in the same call."""
    c = FA.restate_compress_all(signal(), TILE, 1)
    over = ~c["pruned"]
    r = c["ranges"].astype(np.float64)[over]

    def decoded_snr(out, name):
        matches, domains, nr, rs, tile, step, thr, orig = out
        path = str(tmp_path / f"{name}.fwav")
        api.save_compressed(path, matches, domains, rs, SR, 2, tile, step, thr, orig)
        lm, ld, lnr, lrs, *_ = api.load_compressed(path)
        rec = api.decompress_audio(lm, ld, lnr, lrs, s_damping=1e-6).reshape(lnr, lrs)
        noise = ((rec.astype(np.float64)[over] - r) ** 2).sum()
        return 10 * np.log10((r ** 2).sum() / noise), FC.snr_db(c["ranges"], np.asarray(matches.err), over)

    dec_all, fit_all = decoded_snr(compressed(1, candidates="all"), "all")
    dec_emb, fit_emb = decoded_snr(compressed(1), "embedding")
    print(f"candidates=all: fit {fit_all:.3f} dB, decoded {dec_all:.3f} dB; embedding: fit {fit_emb:.3f} dB, decoded "
          f"{dec_emb:.3f} dB")
    assert abs(dec_all - fit_all) <= 0.05, (fit_all, dec_all)
    assert dec_all >= dec_emb, (dec_all, dec_emb)


# ------------------------------------------------------------------------------------------------- 6. default untouched
def test_default_is_still_the_oracles():
    sig = signal()
    ref = O.compress(sig, TILE, 32)
    matches, domains, nr, rs, *_ = api.compress_audio(sig, SR, 2, tile_size=TILE)
    assert (nr, rs) == (len(ref["ranges"]), ref["rs"])
    assert np.array_equal(domains.view(np.uint32), ref["pool"].view(np.uint32))
    for nm, g in zip(NAMES, arrays(matches)):
        assert np.array_equal(raw(g), raw(np.asarray(ref[nm]).astype(g.dtype))), nm
