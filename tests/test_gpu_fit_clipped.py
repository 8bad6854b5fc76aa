"""compress_audio(fit="clipped") on the device: fwav_affine_fit called directly over its three dispatch paths on the
affine edge table, then the whole pipeline, against the numpy restatement of tests/fit_clipped.py.

Bar: every output bit-equal to the restatement, except that a NaN matches any NaN (AE.same_bits_or_nan).  The one
tolerance is the round trip's: the decoded SNR over the searched ranges lies within 0.05 dB of the SNR the stored err
promises — s_damping = 1e-6 perturbs s by about 1e-6 of the signal, against noise of at least 1e-3 of it (SNR ≤ 60 dB),
which is under 0.01 dB."""
import os

import numpy as np
import pytest

import affine_edges as AE
import fit_clipped as FC
import tie_edges as TE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import api, engine, hipctypes, stages, ties as fties  # noqa: E402
from fwav._lib import call, size_call  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

DEV = torch.device("cuda", 0)
F32 = np.float32
NAMES = ("idx", "s", "o", "sym", "err")
OUT_DTYPES = (torch.int32, torch.float32, torch.float32, torch.uint8, torch.float32)


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ------------------------------------------------------------------------------------ 1. fwav_affine_fit directly
class Solver:
    """The table on the device once; solve(a, b, s_clip, fit) runs the entry point on rows [a, b) alone."""

    def __init__(self, ranges, cand, pool):
        self.rs, self.K, self.nd = ranges.shape[1], cand.shape[1], len(pool)
        self.ranges, self.cand, self.pool = td(ranges.reshape(-1)), td(cand.reshape(-1)), td(pool.reshape(-1))

    def solve(self, a, b, s_clip=16.0, fit=1):
        n = b - a
        out = [torch.empty(n, dtype=dt, device=DEV) for dt in OUT_DTYPES]
        args = (self.ranges[a * self.rs:].data_ptr(), n, self.rs, self.cand[a * self.K:].data_ptr(), self.K,
                self.pool.data_ptr(), self.nd, float(s_clip), *[t.data_ptr() for t in out])
        if fit is None:
            call("fwav_affine", *args, stream())
        else:
            call("fwav_affine_fit", *args, fit, stream())
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]


def edge_table(rs, K):
    """tests/affine_edges.build's table with the twin rows of tests/fit_clipped.py appended (two indices holding
    bit-identical tiles, in both slot orders)."""
    ranges, cand, pool, names = AE.build(rs, K)
    tr, tc, patch = FC.twin_rows(rs, K)
    pool = pool.copy()
    for dst, src in patch.items():
        pool[dst] = pool[src]
    label = names + ["random"] * (AE.N_ROWS - len(names)) + ["twin"] * len(tr)
    return np.concatenate([ranges, tr]), np.concatenate([cand, tc]), pool, label


S_CLIPS = (16.0, 0.5, 0.0, -16.0)


@pytest.mark.parametrize("rs", (4, 8, 16, 5, 19))
def test_affine_fit_sweep_against_the_restatement(rs):
    """rs × K ∈ {1, 2, 63, 64, 65, 129} × rows ∈ {1, 15, 16, 17, 67}: every slice of the table solved on its own equals
    the same rows of the restatement on the whole table; s_clip 16, 0.5, 0 and −16 on the whole-table call."""
    for K in AE.K_ALL:
        ranges, cand, pool, label = edge_table(rs, K)
        n_all = len(ranges)
        want = {sc: FC.affine_clipped(ranges, cand, pool, sc) for sc in S_CLIPS}
        sv = Solver(ranges, cand, pool)
        calls = [(0, n_all, sc) for sc in S_CLIPS]
        calls += [(a, a + 1, 16.0) for a in range(AE.N_ROWS, n_all)]  # every twin row on its own
        for n in AE.ROWS_ALL:
            for a, b in AE.slices(n):
                if n == 1 and label[a] == "random" and a >= label.index("random") + 3:
                    continue  # single-row calls: every edge row and three random ones
                calls.append((a, b, 16.0))
        for a, b, sc in calls:
            got = sv.solve(a, b, sc)
            for nm, g, w in zip(NAMES, got, want[sc]):
                w = np.asarray(w)[a:b]
                bad = [i for i in range(b - a) if not AE.same_bits_or_nan(g[i:i + 1], w[i:i + 1])]
                assert not bad, (f"rs={rs} K={K} rows [{a}, {b}) s_clip={sc} {nm}: "
                                 f"{[(a + i, label[a + i], g[i], w[i]) for i in bad[:5]]}")
        # s_clip 0: every valid slot ties, the lowest valid domain wins; twins: the lower index in either slot order
        idx0 = want[0.0][0]
        assert idx0[0] == 0 and label[0] == "all -1"
        if K >= 2:
            t0 = AE.N_ROWS
            assert want[16.0][0][t0] == want[16.0][0][t0 + 1] == 7 and want[16.0][0][t0 + 2] == 7


@pytest.mark.parametrize("rs,K", [(8, 64), (16, 2), (4, 65), (19, 17), (5, 129)])
def test_fit_0_is_fwav_affine(rs, K):
    ranges, cand, pool, _ = edge_table(rs, K)
    sv = Solver(ranges, cand, pool)
    for sc in (16.0, 0.5):
        a, b = sv.solve(0, len(ranges), sc, fit=None), sv.solve(0, len(ranges), sc, fit=0)
        with np.errstate(all="ignore"):
            ref = O.affine(ranges, cand, pool, s_clip=sc)
        for nm, x, y, w in zip(NAMES, a, b, ref):
            assert AE.same_bits_or_nan(x, y) and AE.same_bits_or_nan(y, np.asarray(w).astype(y.dtype)), (rs, K, sc, nm)


def test_torch_free_affine_batch():
    ranges, cand, pool, _ = edge_table(8, 17)
    got = hipctypes.affine_batch(ranges, cand, pool, s_clip=0.5, fit="clipped")
    for nm, g, w in zip(NAMES, got, FC.affine_clipped(ranges, cand, pool, 0.5)):
        assert AE.same_bits_or_nan(g, w), nm


# -------------------------------------------------------------------------------------------------- 2. pipelines
PIPES = [("speech", 2048, "domain_row"), ("speech", 2048, "range"), ("speech", 1024, "domain_row"),
         ("speech", 1024, "range"), ("sweep", 1024, "domain_row"), ("sweep", 1024, "range")]
ROUND_TRIPS = PIPES + [("noise", 2048, "domain_row"), ("noise", 2048, "range")]  # the eight rows of the CPU table
_DEVICE: dict = {}


def compressed(name, tile, query):
    """api.compress_audio(fit="clipped") of one restated case, once."""
    key = (name, tile, query)
    if key not in _DEVICE:
        c = FC.restated(name, tile, query)
        _DEVICE[key] = api.compress_audio(c["sig"], 44100, 2, tile_size=tile, top_k=32, query=query, fit="clipped")
    return _DEVICE[key]


def assert_tuples(got5, want5, what):
    for nm, g, w in zip(NAMES, got5, want5):
        g, w = np.asarray(g), np.asarray(w)
        assert AE.same_bits_or_nan(g, w.astype(g.dtype)), (what, nm, np.nonzero(g != w)[0][:5])


def arrays(m):
    return tuple(np.asarray(getattr(m, f)) for f in NAMES)


@pytest.mark.parametrize("name,tile,query", PIPES)
def test_pipeline_equals_the_restatement_tuple_for_tuple(name, tile, query):
    c = FC.restated(name, tile, query)
    matches, domains, nr, rs, _, step, _, orig = compressed(name, tile, query)
    assert (nr, rs, step, orig) == (c["nr"], c["rs"], c["step"], len(c["sig"]))
    assert np.array_equal(domains.view(np.uint32), c["pool"].view(np.uint32))
    assert_tuples(arrays(matches), c["mc"], (name, tile, query))
    # the option changes matches here, and the default is still the reference's
    if (name, tile, query) != ("speech", 2048, "domain_row"):
        assert not np.array_equal(c["mc"][0], c["m"][0])
    if query == "domain_row":
        ref = api.compress_audio(c["sig"], 44100, 2, tile_size=tile, top_k=32, fit="reference")
        assert_tuples(arrays(ref[0]), c["m"], (name, tile, "default"))


@pytest.mark.parametrize("name,tile,query", ROUND_TRIPS)
def test_round_trip_decodes_to_the_stored_error(name, tile, query):
    """decompress_audio(s_damping=1e-6) of the clipped set, over the searched ranges: its SNR is the one the stored
    err promises, 10·log10(Σ‖r‖² / Σ err²), within 0.05 dB."""
    c = FC.restated(name, tile, query)
    matches, domains, nr, rs, *_ = compressed(name, tile, query)
    rec = api.decompress_audio(matches, domains, nr, rs, s_damping=1e-6).reshape(nr, rs)
    err = np.asarray(matches.err)
    over = np.isfinite(err)
    r = c["ranges"].astype(np.float64)[over]
    noise = ((rec.astype(np.float64)[over] - r) ** 2).sum()
    decoded = 10 * np.log10((r ** 2).sum() / noise)
    promised = FC.snr_db(c["ranges"], err, over)
    print(f"{name} tile {tile} {query}: promised {promised:.3f} dB, decoded {decoded:.3f} dB")
    assert abs(decoded - promised) <= 0.05, (promised, decoded)


def test_k_100():
    """K > 64: the one-wave-per-range kernel (k_affine<RS, clipped>) and every listed tie resolved on the host."""
    c = FC.restated("speech", 2048, "domain_row", K=100)
    out = api.compress_audio(c["sig"], 44100, 2, tile_size=2048, top_k=100, fit="clipped")
    assert_tuples(arrays(out[0]), c["mc"], "K=100")


def test_compact_composes():
    c = FC.restated("speech", 1024, "range")
    cm, cd, nr, rs, *_ = api.compress_audio(c["sig"], 44100, 2, tile_size=1024, top_k=32, query="range", fit="clipped",
                                            compact=True)
    idx, s, o, sym, err = c["mc"]
    assert len(cd) == len(np.unique(idx)) and np.array_equal(cd[np.asarray(cm.idx)].view(np.uint32),
                                                             c["pool"][idx].view(np.uint32))
    assert_tuples(arrays(cm)[1:], (s, o, sym, err), "compact")


def test_emb_dim_32():
    """The stage sits after the search: with 32-wide rows the clipped tuples are the restated selection over the
    device's candidate rows, whose sets tie_order="numpy_sets" makes the reference's (tests/test_gpu_embdim.py); the
    default tie order gives the same tuples, because under the clipped fit it ranks the same rows."""
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "embdim32_t2048.npz")))
    sig = g["signal"]
    r = engine.compress_device(td(sig), 2048, 32, emb_dim=32, fit="clipped", tie_order="numpy_sets",
                               keep_intermediates=True)
    torch.cuda.synchronize()
    rs = r.range_size
    ranges = r.ranges.cpu().numpy().reshape(-1, rs)
    cand = r.cand.cpu().numpy().reshape(r.n_ranges, 32)
    pool = r.pool.cpu().numpy().reshape(-1, rs)
    want = FC.chunked(FC.affine_clipped, ranges, cand, pool)
    assert_tuples([getattr(r, nm).cpu().numpy() for nm in NAMES], want, "emb_dim=32")
    out = api.compress_audio(sig, 44100, 2, tile_size=2048, top_k=32, emb_dim=32, fit="clipped")
    assert_tuples(arrays(out[0]), want, "emb_dim=32 api")


def test_shard_sub_blocks_and_deferred_ties_agree():
    c = FC.restated("speech", 1024, "range")
    t = td(c["sig"])
    for opts in (dict(sub_blocks=3), dict(defer_ties=True), dict(sub_blocks=2, defer_ties=True)):
        r = engine.compress_device(t, 1024, 32, query="range", fit="clipped", **opts).wait()
        torch.cuda.synchronize()
        assert_tuples([getattr(r, nm).cpu().numpy() for nm in NAMES], c["mc"], opts)
    lo, hi = 1000, 3001
    r = engine.compress_device(t, 1024, 32, query="range", fit="clipped", shard=(lo, hi))
    torch.cuda.synchronize()
    assert_tuples([getattr(r, nm).cpu().numpy() for nm in NAMES], [w[lo:hi] for w in c["mc"]], "shard")


def test_torch_free_host_equals_the_engine():
    c = FC.restated("speech", 2048, "domain_row")
    h = hipctypes.compress(c["sig"], 2048, 32, fit="clipped")
    assert_tuples([h[nm] for nm in NAMES], c["mc"], "hipctypes")
    assert_tuples([h[nm] for nm in NAMES], arrays(compressed("speech", 2048, "domain_row")[0]), "hipctypes vs engine")


# ------------------------------------------------------------------------------------ 3. ties at the K-th place
def clipped_sequence(c, tie_order):
    """The product sequence of tests/test_gpu_tie_edges.py in the clipped mode: search → fwav_affine_fit → fwav_tie_check
    in stages.tie_mode(tie_order, "clipped") → fwav.ties.resolve_rows(fit="clipped")."""
    from test_gpu_tie_edges import table_of
    tab = table_of(c)
    nd, K, mq, rs, T = c.nd, c.K, c.max_q, c.rs, O.blas_threads()
    act, n_act = td(c.ids), td(np.array([len(c.ids)], np.int32))
    cand = torch.full((mq * K,), -1, dtype=torch.int32, device=DEV)
    tl = torch.empty(size_call("fwav_tie_list_size", mq), dtype=torch.int32, device=DEV)
    wk = size_call("fwav_sim_topk_workspace_size", mq, nd, K)
    ws = torch.zeros(max(wk, 16), dtype=torch.uint8, device=DEV)
    st = stream()
    call("fwav_sim_topk", tab.emb.data_ptr(), tab.e16.data_ptr(), nd, act.data_ptr(), n_act.data_ptr(), mq, c.q_offset,
         K, T, cand.data_ptr(), tl.data_ptr(), ws.data_ptr(), wk, st)
    ranges, pool = td(c.ranges.reshape(-1)), td(c.pool.reshape(-1))
    outs = [torch.empty(mq, dtype=dt, device=DEV) for dt in OUT_DTYPES]
    stages.affine(ranges.data_ptr(), mq, rs, cand.data_ptr(), K, pool.data_ptr(), nd, 16.0,
                  [t.data_ptr() for t in outs], st, fit="clipped")
    resolve = torch.empty(mq + 1, dtype=torch.int32, device=DEV)
    stages.tie_check(ranges.data_ptr(), mq, rs, cand.data_ptr(), K, pool.data_ptr(), nd, tab.emb.data_ptr(), c.q_offset,
                     T, tl.data_ptr(), mq, stages.tie_mode(tie_order, "clipped"), resolve.data_ptr(), st)
    n = int(resolve[0].item())
    fties.resolve_rows(resolve[1:1 + n], emb=tab.emb, n_domains=nd, q_offset=c.q_offset, k=K, threads=T, ranges=ranges,
                       range_size=rs, pool=pool, s_clip=16.0, cand=cand, outs=tuple(outs), stream=st, fit="clipped")
    torch.cuda.synchronize()
    return cand.cpu().numpy().reshape(mq, K), [t.cpu().numpy() for t in outs], resolve[1:1 + n].cpu().tolist()


@pytest.mark.parametrize("nd,K", [(65, 2), (65, 17), (257, 32), (257, 64)])
def test_kth_place_ties_numpy_equals_numpy_sets(nd, K):
    """Exact score ties at the K-th place (tests/tie_edges.py's dyadic tables): under the clipped fit "numpy" resolves
    what "numpy_sets" resolves, the candidate sets are numpy's, and every tuple is the restated selection over numpy's
    own row."""
    c = TE.Case(nd, K, TE.RS_OF_ND[nd], TE.SEED_OF_ND[nd], decisions=False)
    kth = {q for q, (flag, n, m) in c.exp.items() if flag}
    assert kth
    npy = np.stack([O.numpy_topk_row(r, K) for r in c.rows])
    want = FC.affine_clipped(c.ranges[c.ids], npy, c.pool)
    res = {order: clipped_sequence(c, order) for order in ("numpy", "numpy_sets")}
    for order, (cand, outs, rows) in res.items():
        assert kth <= set(rows), (order, sorted(kth - set(rows))[:5])
        assert_tuples([o[c.ids] for o in outs], want, (nd, K, order))
        for j, q in enumerate(c.ids):
            assert set(cand[q].tolist()) == set(npy[j].tolist()), (order, int(q))
    assert sorted(res["numpy"][2]) == sorted(res["numpy_sets"][2])
    for a, b in zip(res["numpy"][1], res["numpy_sets"][1]):
        assert AE.same_bits_or_nan(a, b)
