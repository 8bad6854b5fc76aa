"""The exact embedding (embedding="pocketfft": fwav_pool_embed_exact, k_embed_exact) at range sizes other than 4, 8 and
16: bit for bit the reference's embedding (fractal.py:154-208: scipy's f32 and f64 pocketfft DCTs, numpy's norms), and
through it the reference's candidate sets and match tuples end to end.

Bars: everything here is bit-equality — against the goldens t8192 (rs 32), t5000 (rs 19), t1300 (rs 5), and against a
host restatement of the two heads with scipy and numpy themselves on synthetic rows at sixteen range sizes that cover
every pass kind of the plan (radix 4, 2, 3, 5, the generic pass with ido = 1 and ido > 1, mixed plans)."""
import functools

import numpy as np
import pytest

from golden_util import GENERIC_CASES, bit_equal, load, same_sets

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import engine  # noqa: E402
from fwav._lib import call, size_call  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

F32 = np.float32
NAMES = ("idx", "s", "o", "sym", "err")
ND = 333  # not a multiple of the kernel's 64-thread groups nor of the fp16 tables' 256-row chunks


def dev():
    return torch.device("cuda", 0)


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def golden(case):
    return load(case)


def pool_embed_exact(sig, tile, rs, step):
    """fwav_pool_embed_exact → (pool f32[nd, rs], emb f32[nd, 16], emb16 u16[...], fwav_emb16_from_emb(emb) u16[...])."""
    x = td(np.asarray(sig, F32))
    n = x.numel()
    nd = (n - tile) // step + 1
    tab = engine.embed_tables(rs, dev(), "pocketfft")
    pool = torch.full((nd * rs,), np.nan, dtype=torch.float32, device=dev())
    emb = torch.full((nd * 16,), np.nan, dtype=torch.float32, device=dev())
    n16 = size_call("fwav_emb16_elems", nd)
    emb16 = torch.full((n16,), np.nan, dtype=torch.float16, device=dev())
    want16 = torch.full((n16,), np.nan, dtype=torch.float16, device=dev())
    wsn = size_call("fwav_pool_workspace_size", n, tile, rs, step)
    ws = torch.empty(max(wsn, 16), dtype=torch.uint8, device=dev())
    call("fwav_pool_embed_exact", x.data_ptr(), n, tile, rs, step, tab.data_ptr(), pool.data_ptr(), emb.data_ptr(),
         emb16.data_ptr(), ws.data_ptr(), wsn, stream())
    call("fwav_emb16_from_emb", emb.data_ptr(), nd, want16.data_ptr(), stream())
    torch.cuda.synchronize()
    return (pool.cpu().numpy().reshape(nd, rs), emb.cpu().numpy().reshape(nd, 16),
            emb16.cpu().numpy().view(np.uint16), want16.cpu().numpy().view(np.uint16))


def diff_rows(a, b):
    """Rows on which two float32 tables differ in any bit."""
    return np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0]


@pytest.mark.parametrize("case", GENERIC_CASES)
def test_goldens(case):
    """The reference's own embedding, all 16 columns of every row, its pool, and the fp16 tables of that embedding."""
    g = golden(case)
    p = g["p"]
    pool, emb, emb16, want16 = pool_embed_exact(g["signal"], p["tile"], p["rs"], p["step"])
    assert len(emb) == p["n_domains"]
    assert bit_equal(pool, g["pool"])
    bad = diff_rows(emb, g["emb"])
    assert len(bad) == 0, f"{case}: {len(bad)}/{len(emb)} embedding rows differ from the reference's, first {bad[:8]}"
    assert np.array_equal(emb16, want16)


def reference_embedding(pool):
    """multi_head_embedding (fractal.py:166-175) restated row by row with scipy's DCT and numpy's own norm: the tonal
    head of tile_embedding (:178-208) and the transient head of transient_embedding (:154-164)."""
    import scipy.fftpack
    nd, rs = pool.shape
    w = np.linspace(1.0, 2.0, rs)
    ton = scipy.fftpack.dct(pool, norm="ortho", axis=-1)
    assert ton.dtype == F32
    ton = ton * w
    dif = np.diff(pool, axis=-1, prepend=pool[:, :1])
    assert dif.dtype == F32
    tra = scipy.fftpack.dct(dif * w, norm="ortho", axis=-1)
    assert tra.dtype == np.float64
    take, tk = min(8, rs - 1), min(8, rs)
    out = np.zeros((nd, 16), F32)
    for d in range(nd):
        e = np.zeros(8, F32)
        e[:take] = ton[d, 1:1 + take].astype(F32)
        nrm = np.linalg.norm(e)
        if nrm > 1e-8:
            e = e / nrm
        v = tra[d, :tk]
        nrm = np.linalg.norm(v)
        if nrm > 1e-8:
            v = v / nrm
        out[d, :8] = e
        out[d, 8:8 + tk] = v.astype(F32)
    return out


def synthetic_signal(rs, bl, step, seed):
    """A signal of exactly ND domains (tile = rs·bl) whose pool holds, besides noise rows of scales 1e-3 … 1e2, one
    whole domain each of: zeros, a constant, 1e3 + noise·1e-3, and noise at 1e-30 (each segment starts on a domain
    boundary and is one tile long, so one pool row lies wholly inside it)."""
    rng = np.random.default_rng(seed)
    tile = rs * bl
    n = tile + (ND - 1) * step
    assert 4 * tile + 4 * step <= n, (rs, bl, step)
    sig = rng.standard_normal(n) * np.repeat(rng.choice([1e-3, 0.1, 1.0, 1e2], -(-n // 16)), 16)[:n]
    gap = (n - 4 * tile) // 4 // step * step
    for j, kind in enumerate(("zero", "const", "dc", "tiny")):
        a = j * (tile + gap) // step * step
        seg = {"zero": np.zeros(tile), "const": np.full(tile, 0.37), "dc": 1e3 + rng.standard_normal(tile) * 1e-3,
               "tiny": rng.standard_normal(tile) * 1e-30}[kind]
        sig[a:a + tile] = seg
    return sig.astype(F32), tile


#: every pass kind and mixed plans: 5, 7, 19 (one factor: radix 5, generic), 6 = 2·3, 9 = 3·3, 10 = 2·5, 12 = 4·3,
#: 14 = 2·7, 20 = 4·5, 25 = 5·5, 32 = 2·4·4, 36 = 4·3·3, 45 = 3·3·5, 48 = 4·4·3, 49 = 7·7 (generic, ido > 1), 64 = 4·4·4
SYNTH_RS = [5, 6, 7, 9, 10, 12, 14, 19, 20, 25, 32, 36, 45, 48, 49, 64]


@pytest.mark.parametrize("layout", ["block_means", "domain_pool"])
@pytest.mark.parametrize("rs", SYNTH_RS)
def test_synthetic_rows(rs, layout):
    """Every column of every one of 333 rows against the host restatement, on both pool layouts: a step that divides
    the block (block means read with stride block/step: 2 wherever the four special domains fit into 333 domains
    then, i.e. 6·rs ≤ 332, else 1) and one that does not (k_domain_pool's rows).  The rows include all-zero rows,
    constant rows (whose tonal norm is rounding noise next to the 1e-8 switch: both sides must take the same branch),
    1e3 + noise·1e-3, the 1e-30 scale, and at rs 5 and 6 fewer than 8 tonal coefficients."""
    if layout == "block_means":
        step = 4
        bl = 2 * step if 6 * rs + 8 <= ND - 1 else step
    else:
        bl, step = 3, 2
    assert (bl % step == 0) == (layout == "block_means")
    sig, tile = synthetic_signal(rs, bl, step, 1000 * rs + bl)
    ref_pool = O.domain_pool(sig, tile, rs, step)
    assert ref_pool.shape == (ND, rs)
    rows = {"zero": (ref_pool == 0).all(axis=1),
            "const": (ref_pool == ref_pool[:, :1]).all(axis=1) & (ref_pool[:, 0] != 0),
            "dc": (ref_pool > 900).all(axis=1) & (ref_pool != ref_pool[:, :1]).any(axis=1),
            "tiny": (np.abs(ref_pool) < 1e-28).all(axis=1) & (ref_pool != 0).any(axis=1)}
    assert all(m.any() for m in rows.values()), {k: int(m.sum()) for k, m in rows.items()}
    pool, emb, emb16, want16 = pool_embed_exact(sig, tile, rs, step)
    assert bit_equal(pool, ref_pool)
    want = reference_embedding(ref_pool)
    bad = diff_rows(emb, want)
    kinds = {k: int(m[bad].sum()) for k, m in rows.items()}
    assert len(bad) == 0, f"rs {rs} {layout}: {len(bad)}/{ND} rows differ, first {bad[:8]}, special rows among them {kinds}"
    assert (emb[rows["zero"]] == 0).all()
    if rs < 9:
        assert (want[:, rs - 1:8] == 0).all() and (want[:, 8 + min(8, rs):] == 0).all()
    assert np.array_equal(emb16, want16)


def compress(case, K, **kw):
    g = golden(case)
    p = g["p"]
    r = engine.compress_device(td(g["signal"]), p["tile"], K, p["thr"], blas_threads=8, tie_order="numpy_sets",
                               keep_intermediates=True, **kw)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("case", GENERIC_CASES)
def test_end_to_end_is_the_reference(case):
    """compress_device(embedding="pocketfft") on the golden signals: every match tuple and every candidate set is the
    reference's (690/690 at tile 8192, where the matrix embedding gives 688 tuples and 682 sets)."""
    g = golden(case)
    p = g["p"]
    for K in p["Ks"]:
        r = compress(case, K, embedding="pocketfft")
        assert bit_equal(r.emb.cpu().numpy().reshape(-1, 16), g["emb"])
        for nm in NAMES:
            got = getattr(r, nm).cpu().numpy()
            assert bit_equal(got, g[f"m_{nm}_{K}"]), f"{case} K={K} {nm}"
        sets = same_sets(r.cand.cpu().numpy().reshape(-1, K), g[f"cand_{K}"])
        assert sets.all(), f"{case} K={K}: {int(sets.sum())}/{len(sets)} candidate sets equal the reference's"


def test_end_to_end_torch_free_binding():
    """The same call through fwav.hipctypes.compress (numpy and HIP buffers only) on t5000."""
    from fwav import hipctypes
    g = golden("t5000")
    p = g["p"]
    for K in p["Ks"]:
        r = hipctypes.compress(g["signal"], p["tile"], K, energy_thresh=p["thr"], tie_order="numpy_sets", threads=8,
                               embedding="pocketfft")
        assert r is not None and r["n_ranges"] == p["n_ranges"]
        assert bit_equal(r["pool"], g["pool"]) and bit_equal(r["emb"], g["emb"])
        for nm in NAMES:
            assert bit_equal(r[nm], g[f"m_{nm}_{K}"]), (K, nm)
        assert same_sets(r["cand"], g[f"cand_{K}"]).all()
    pool, emb = hipctypes.pool_embed(g["signal"], p["tile"], p["rs"], p["step"], embedding="pocketfft")
    assert bit_equal(pool, g["pool"]) and bit_equal(emb, g["emb"])


@pytest.mark.parametrize("case", ["noise2048", "noise4096"])
def test_range_sizes_8_and_16_are_the_default_path(case):
    """At range sizes 8 and 16 embedding="pocketfft" routes to the existing kernels: the same bytes as the default."""
    g = golden(case)
    p = g["p"]
    assert p["rs"] == {"noise2048": 8, "noise4096": 16}[case]
    K = p["Ks"][0]
    a, b = compress(case, K), compress(case, K, embedding="pocketfft")
    for nm in ("pool", "emb", "cand") + NAMES:
        x, y = getattr(a, nm).cpu().numpy(), getattr(b, nm).cpu().numpy()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), nm
    assert bit_equal(b.emb.cpu().numpy().reshape(-1, 16), g["emb"])


def test_errors():
    """No silent fall-back: "pocketfft" at a range size without an exact plan (tile 13056 → rs 51, where pocketfft
    itself may leave its factorised plan) is a ValueError that names the range size; so is an unknown mode."""
    sig = td(np.zeros(20000, F32))
    assert not size_call("fwav_embed_exact_supported", 51)
    with pytest.raises(ValueError, match="51"):
        engine.compress_device(sig, 13056, 8, embedding="pocketfft")
    with pytest.raises(ValueError, match="65"):
        engine.compress_device(sig, 16640, 8, embedding="pocketfft")
    with pytest.raises(ValueError, match="embedding"):
        engine.compress_device(sig, 8192, 8, embedding="scipy")
    with pytest.raises(ValueError, match="51"):
        engine.embed_tables(51, dev(), "pocketfft")
    from fwav import hipctypes
    with pytest.raises(ValueError, match="51"):
        hipctypes.compress(np.ones(20000, F32), 13056, 8, embedding="pocketfft")
    with pytest.raises(ValueError, match="embedding"):
        hipctypes.compress(np.ones(20000, F32), 8192, 8, embedding="scipy")
    # the C ABI refuses it too, before any launch
    p = sig.data_ptr()
    rc = __import__("fwav")._lib.lib().fwav_pool_embed_exact(p, 20000, 13056, 51, 204, p, p, p, None, p, 1 << 20, None)
    assert rc == -1
