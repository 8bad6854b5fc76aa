"""emb_dim = 32 without a GPU: the arithmetic orders the wide embedding and search rely on, pinned against numpy on
this host; the fp16 pre-filter's error bound δ through the search's own helpers (compiled for the host); the argument
checks of every *_dim entry point; the Python layers' validation of emb_dim."""
import ctypes

import numpy as np
import pytest

from oracle import fractal_oracle as O
from split_edges import THREAD_MIN_MN, col_kinds, sgemv_dim_np, unit_head_rows  # noqa: F401

F32 = np.float32
D = 32


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from fwav import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ sgemv order
def test_sgemv_order_pinned_against_numpy():
    """The restatement of sgemv_dim and of the thread split equals numpy's ``A @ q`` bit for bit at D = 32: one thread
    and this host's count, nd on both sides of D·nd = 460,800, chunk widths of every residue mod 4."""
    threadpoolctl = pytest.importorskip("threadpoolctl")
    host = O.blas_threads()
    rng = np.random.default_rng(5)
    widths = {1: set(), host: set()}
    for T in sorted({1, host}):
        with threadpoolctl.threadpool_limits(T, user_api="blas"):
            assert O.blas_threads() == T
            for nd in (14396, 14397, 14398, 14399, 14401, 14402, 14403, 14404, 14401 + 4 * T + 1, 14401 + 4 * T + 2):
                A = unit_head_rows(rng, nd)
                q = A[rng.integers(nd)]
                kinds, w = col_kinds(nd, T)
                widths[T] |= {x % 4 for x in w}
                ref = A @ q
                got = sgemv_dim_np(A, q, kinds)
                bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
                assert bad.size == 0, (T, nd, bad[:8], kinds[bad[:8]])
    for T, res in widths.items():
        assert res == {0, 1, 2, 3}, (T, res)


def test_kernel_helper_is_the_pinned_order(lib):
    """The search's own sgemv_dim<32> (compiled for the host behind fwav_debug_score_dim) gives the restatement's value
    for each of the three kernels, so the device scores are numpy's."""
    L = lib.product_lib()
    rng = np.random.default_rng(6)
    A = unit_head_rows(rng, 600)
    q = A[17].copy()
    out = np.zeros(3, F32)
    for kind in (0, 1, 2):
        want = sgemv_dim_np(A, q, np.full(len(A), kind))
        for i in range(len(A)):
            assert L.fwav_debug_score_dim(A[i].ctypes.data, q.ctypes.data, D, kind, out.ctypes.data) == 0
            assert out[0].view(np.uint32) == want[i].view(np.uint32), (kind, i)


# ------------------------------------------------------------------------------------------------ ddot order
def ddot16(x: np.ndarray) -> np.float64:
    """fwav_pool_embed.hip ddot_self at 16 values: four lanes l[i % 4] += x_i·x_i (product and add rounded
    separately), folded (l0 + l2) + (l1 + l3)."""
    l = np.zeros(4)
    for i in range(16):
        l[i % 4] = l[i % 4] + x[i] * x[i]
    return (l[0] + l[2]) + (l[1] + l[3])


def test_ddot_order_of_16_values_pinned_against_numpy():
    rng = np.random.default_rng(7)
    for i in range(2000):
        x = rng.normal(0, 1, 16) * 10.0 ** rng.integers(-6, 3)
        assert ddot16(x) == np.dot(x, x), i


# ------------------------------------------------------------------------------------------------ fp16 bound
def _fill_unit(vals) -> np.ndarray:
    """A head of 16 values: ``vals`` first, the rest equal and such that the head's norm is 1."""
    vals = np.asarray(vals, np.float64)
    rest = 16 - len(vals)
    out = np.empty(16)
    out[:len(vals)] = vals
    if rest:
        out[len(vals):] = np.sqrt(max(0.0, 1.0 - (vals ** 2).sum()) / rest)
    return out


def adversarial_rows() -> np.ndarray:
    u = 2.0 ** -11
    e = 2.0 ** -23
    heads = []
    for j in (0, 3, 15):  # all mass in one element
        h = np.zeros(16)
        h[j] = 1.0 if j else -1.0
        heads.append(h)
    # as many elements as a unit norm allows just below / above an fp16 rounding midpoint, where the relative error of
    # a product is the largest there is (15 of 0.25·(1 + u), 3 of 0.5·(1 + u), …), the rest of the head filling the norm
    for m in (1 + u - e, 1 + u + e):
        heads.append(_fill_unit([0.25 * m] * 15))
        heads.append(_fill_unit([0.5 * m] * 3))
        heads.append(_fill_unit([0.5 * m, 0.5 * m, 0.5 * m, 0.25 * m, 0.25 * m, 0.25 * m]))
        heads.append(_fill_unit([0.125 * (m + 2 * u)] * 15))
        heads.append(_fill_unit([0.6 * m]))
        heads.append(_fill_unit([0.6 * m] + [0.0] * 14))
        heads.append(_fill_unit([0.25 * (2 - m + u / 2)] * 15))  # just beside the midpoint below 0.25
    # values at fp16's subnormal edge beside the large ones
    for tiny in (2.0 ** -14, 2.0 ** -14 * (1 - u), 2.0 ** -15 * 1.5, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -26,
                 1.5 * 2.0 ** -24):
        heads.append(_fill_unit([tiny] * 15))
        heads.append(_fill_unit([tiny] * 8 + [0.25 * (1 + u - e)] * 7))
    heads.append(np.zeros(16))  # a zero head
    heads = np.array(heads)
    rows = []
    # both heads alike, d and q with equal signs (Σ d_k q_k = Σ|d_k q_k| = 2: nothing cancels) or sign patterns
    signs = (np.ones(D), np.where(np.arange(D) % 2 == 0, 1.0, -1.0), np.where(np.arange(D) % 3 == 0, -1.0, 1.0), -np.ones(D))
    for i, h in enumerate(heads):
        for sg in signs:
            rows.append(np.concatenate([h, heads[(i + 1) % len(heads)] if i % 4 == 3 else h]) * sg)
    return np.ascontiguousarray(np.array(rows).astype(F32))


def test_fp16_prefilter_bound(lib):
    """|fp16 dot in f32 − sgemv_dim| < δ on random and adversarial unit-norm-head rows, for each sgemv kernel, through
    the search's own helpers; δ itself is the kernel's constant (out[2])."""
    L = lib.product_lib()
    rng = np.random.default_rng(8)
    adv = adversarial_rows()
    head_norm = np.sqrt((adv.reshape(-1, 2, 16).astype(np.float64) ** 2).sum(-1))
    assert head_norm.max() <= 1 + 2.0 ** -22  # the bound's premise: heads of f32 norm 1 (or zero)
    rnd = unit_head_rows(rng, 300)
    out = np.zeros(3, F32)
    worst = 0.0
    pairs = [(d, q) for d in adv for q in adv] + [(rnd[i], rnd[(7 * i + 1) % 300]) for i in range(300)] + \
            [(rnd[i], rnd[i]) for i in range(300)] + [(rnd[i], -rnd[i]) for i in range(100)]
    for d, q in pairs:
        d, q = np.ascontiguousarray(d), np.ascontiguousarray(q)
        for kind in (0, 1, 2):
            assert L.fwav_debug_score_dim(d.ctypes.data, q.ctypes.data, D, kind, out.ctypes.data) == 0
            delta = float(out[2])
            err = abs(float(out[1]) - float(out[0]))
            worst = max(worst, err)
            assert err < delta, (err, delta, kind, d, q)
    assert 1.96311e-3 < delta <= float(F32(2.0e-3))  # above the derived bound, not above the 16-wide δ
    print(f"largest |fp16 score - exact score| over {len(pairs)} pairs x 3 kernels: {worst:.6e} (delta {delta:.3e})")
    assert worst > 1.5e-3  # the adversarial rows do come close to the bound: the test is not vacuous


# ------------------------------------------------------------------------------------------------ argument checks
def test_dim_entry_points_reject_bad_arguments(lib):
    """Every *_dim entry point: FWAV_ERR_ARG for emb_dim 16, 31 and 64 and for null pointers (0 from the size calls),
    before any HIP call — no GPU here."""
    L = lib.product_lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    ERR = -1
    for dim in (16, 31, 64):
        assert L.fwav_embh_elems(1000, dim) == 0
        assert L.fwav_embed_tables_dim_size(8, dim) == 0
        assert L.fwav_sim_topk_dim_workspace_size(10, 1000, dim, 100) == 0
        assert L.fwav_embed_tables_dim(8, dim, p) == ERR
        assert L.fwav_embh_from_emb(p, 10, dim, p, None) == ERR
        assert L.fwav_pool_embed_dim(p, 4096, 2048, 8, 2, dim, p, p, p, p, p, 4096, None) == ERR
        assert L.fwav_prune_dim(p, 4, 0, 8, 1e-4, 1, p, 10, dim, 8, None, p, p, p, None) == ERR
        assert L.fwav_sim_topk_dim(p, p, 10, dim, p, p, 4, 0, 8, 1, p, None, p, 4096, None) == ERR
        assert L.fwav_score_rows_dim(p, 10, dim, p, 1, 0, 1, p, None) == ERR
        assert L.fwav_tie_check_dim(p, 4, 8, p, 8, p, 10, p, dim, 0, 1, p, 4, 0, p, None) == ERR
        assert L.fwav_debug_score_dim(p, p, dim, 0, p) == ERR
        assert b"32" in L.fwav_last_error()
    assert L.fwav_embh_elems(1000, 32) == 1024 * 32 and L.fwav_embh_elems(256, 32) == 256 * 32
    assert L.fwav_embed_tables_dim_size(19, 32) == 32 * 19
    assert L.fwav_sim_topk_dim_workspace_size(10, 1000, 32, 64) == 0
    assert L.fwav_sim_topk_dim_workspace_size(10, 1000, 32, 65) == 10 * 1000 * 4
    assert L.fwav_embed_tables_dim(8, 32, None) == ERR
    assert L.fwav_embh_from_emb(None, 10, 32, p, None) == ERR and L.fwav_embh_from_emb(p, 10, 32, None, None) == ERR
    assert L.fwav_pool_embed_dim(None, 4096, 2048, 8, 2, 32, p, p, p, p, p, 4096, None) == ERR
    assert L.fwav_pool_embed_dim(p, 4096, 2048, 8, 2, 32, None, p, p, p, p, 4096, None) == ERR
    assert L.fwav_pool_embed_dim(p, 4096, 2048, 8, 2, 32, p, p, None, p, p, 4096, None) == ERR
    assert L.fwav_prune_dim(None, 4, 0, 8, 1e-4, 1, p, 10, 32, 8, None, p, p, p, None) == ERR
    assert L.fwav_prune_dim(p, 4, 0, 8, 1e-4, 1, None, 10, 32, 8, None, p, p, p, None) == ERR
    assert L.fwav_sim_topk_dim(None, p, 10, 32, p, p, 4, 0, 8, 1, p, None, p, 4096, None) == ERR
    assert L.fwav_sim_topk_dim(p, None, 10, 32, p, p, 4, 0, 8, 1, p, None, p, 4096, None) == ERR  # K <= 64: table
    assert L.fwav_sim_topk_dim(p, p, 10, 32, None, p, 4, 0, 8, 1, p, None, p, 4096, None) == ERR
    assert L.fwav_sim_topk_dim(p, p, 10, 32, p, p, 4, 0, 8, 1, None, None, p, 4096, None) == ERR
    assert L.fwav_sim_topk_dim(p, p, 10, 32, p, p, 4, 0, 0, 1, p, None, p, 4096, None) == -3  # FWAV_ERR_K
    assert L.fwav_sim_topk_dim(p, None, 10, 32, p, p, 4, 0, 100, 1, p, None, None, 0, None) == -5  # workspace
    assert L.fwav_score_rows_dim(None, 10, 32, p, 1, 0, 1, p, None) == ERR
    assert L.fwav_score_rows_dim(p, 10, 32, p, 1, 0, 0, p, None) == ERR
    assert L.fwav_tie_check_dim(None, 4, 8, p, 8, p, 10, p, 32, 0, 1, p, 4, 0, p, None) == ERR
    assert L.fwav_tie_check_dim(p, 4, 8, p, 8, p, 10, None, 32, 0, 1, p, 4, 0, p, None) == ERR
    assert L.fwav_debug_score_dim(None, p, 32, 0, p) == ERR and L.fwav_debug_score_dim(p, p, 32, 3, p) == ERR
    assert L.fwav_abi_version() == 5


def test_embed_tables_dim_are_the_dct_rows(lib):
    """fwav_embed_tables_dim: 16 tonal rows (DCT rows 1 … min(16, rs − 1), weighted) and 16 transient rows (DCT of the
    weighted difference), zero rows where a range size has fewer coefficients — against scipy, as the 16-wide test."""
    import scipy.fftpack
    L = lib.product_lib()
    for rs in (4, 8, 16, 19, 32):
        n = L.fwav_embed_tables_dim_size(rs, 32)
        tab = np.zeros(n)
        assert L.fwav_embed_tables_dim(rs, 32, tab.ctypes.data) == 0
        w = np.linspace(1.0, 2.0, rs)
        C = scipy.fftpack.dct(np.eye(rs), norm="ortho", axis=0)  # C[k, i]
        take, tk = min(16, rs - 1), min(16, rs)
        tonal = tab[:16 * rs].reshape(16, rs)
        trans = tab[16 * rs:32 * rs].reshape(16, rs)
        assert np.allclose(tonal[:take], C[1:1 + take] * w[1:1 + take, None], atol=1e-14)
        assert np.allclose(trans[:tk], C[:tk] * w[None, :], atol=1e-14)
        assert not tonal[take:].any() and not trans[tk:].any()


# ------------------------------------------------------------------------------------------------ Python layers
def test_emb_dim_validation():
    """16 and 32 pass; any other width is NotImplementedError naming both; pocketfft with 32 is ValueError — in every
    layer, before a device is touched."""
    from fwav import api, cli, dist, engine, hipctypes
    assert engine.check_emb_dim(16) == 16 and engine.check_emb_dim(32) == 32
    sig = np.zeros(4096, F32)
    for call in (lambda d, e: engine.check_emb_dim(d, e),
                 lambda d, e: api.compress_audio(sig, 44100, 4, tile_size=2048, emb_dim=d, embedding=e),
                 lambda d, e: hipctypes.compress(sig, 2048, 8, emb_dim=d, embedding=e),
                 lambda d, e: dist.compress_sharded_start(None, 2048, 8, emb_dim=d, embedding=e)):
        for bad in (8, 24, 64, 0):
            with pytest.raises(NotImplementedError, match="16 and 32"):
                call(bad, "matrix")
        with pytest.raises(ValueError, match="pocketfft.*emb_dim=32"):
            call(32, "pocketfft")
    with pytest.raises(ValueError, match="default compute"):
        dist.compress_sharded_start(None, 2048, 8, compute=lambda *a: None, emb_dim=32)
    with pytest.raises(SystemExit):
        cli.main(["compress", "in.wav", "out", "--emb-dim", "24"])
    r = api.process_file_compress("/nonexistent/in.wav", emb_dim=24)
    assert "error" in r
