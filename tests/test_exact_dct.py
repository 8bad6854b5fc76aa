"""The exact embedding's DCT and tables on the host (no GPU): fwav_dct_plan.h — pocketfft's general real-FFT plan
inside the T_dcst23 wrapper, the code k_embed_exact runs — against scipy.fftpack.dct(x, norm='ortho') bit for bit at
every supported length, and the fwav_embed_tables_exact contract."""
import numpy as np
import pytest

#: the lengths the exact path must support: every n from 4 to 49, then those up to 64 at which pocketfft still takes
#: its factorised plan ((largest prime factor)² ≤ n)
REQUIRED = list(range(4, 50)) + [50, 54, 56, 60, 63, 64]
ROWS = 500


@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    from fwav import _lib
    return _lib.lib()


def supported(L):
    return [n for n in range(0, 130) if L.fwav_embed_exact_supported(n)]


def test_required_lengths_are_supported(L):
    sup = supported(L)
    assert set(REQUIRED) <= set(sup)
    assert all(4 <= n <= 64 for n in sup)
    assert not L.fwav_embed_exact_supported(-3)


def rows_for(n, T, seed):
    """test_dct_is_scipy_bitexact's distribution (scales 1e-30 … 1e4, occasional zeros) plus rows with a large DC
    offset (x + 1e3)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((ROWS, n)) * rng.choice([1e-30, 1e-6, 1e-3, 1.0, 1e4], size=(ROWS, 1))
    zero = rng.random(ROWS) < 0.05
    x[zero, rng.integers(n, size=int(zero.sum()))] = 0
    x[::10] = rng.standard_normal((len(x[::10]), n)) + 1e3
    return x.astype(T)


@pytest.mark.parametrize("dbl", [0, 1])
def test_plan_dct_is_scipy_bitexact(L, dbl):
    """Every supported n (the required ones and any the library adds), 500 rows each, compared as bytes."""
    import scipy.fftpack
    T = np.float64 if dbl else np.float32
    sup = supported(L)
    assert set(REQUIRED) <= set(sup)
    bad = {}
    for n in sup:
        x = rows_for(n, T, 1000 * dbl + n)
        want = scipy.fftpack.dct(x, norm="ortho", axis=1)
        assert want.dtype == T
        got = np.zeros((ROWS, n))
        xin = x.astype(np.float64)
        for r in range(ROWS):
            assert L.fwav_debug_dct2_plan(n, dbl, xin[r].ctypes.data, got[r].ctypes.data) == 0
        got = got.astype(T)
        diff = (got.view(np.uint8).reshape(ROWS, -1) != want.view(np.uint8).reshape(ROWS, -1)).any(axis=1)
        if diff.any():
            bad[n] = int(diff.sum())
    assert not bad, f"rows that differ from scipy, by n: {bad}"


def test_plan_dct_agrees_with_the_fixed_plans(L):
    """n = 4, 8, 16 through the general plan equal fwav_dct.h's compile-time plans (fwav_debug_dct2)."""
    for n in (4, 8, 16):
        for dbl in (0, 1):
            x = rows_for(n, np.float64 if dbl else np.float32, n).astype(np.float64)
            a, b = np.zeros(n), np.zeros(n)
            for r in range(100):
                assert L.fwav_debug_dct2(n, dbl, x[r].ctypes.data, a.ctypes.data) == 0
                assert L.fwav_debug_dct2_plan(n, dbl, x[r].ctypes.data, b.ctypes.data) == 0
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_unsupported_lengths_fail_with_a_message(L):
    sup = set(supported(L))
    out = np.zeros(4096)
    x = np.zeros(256)
    for n in range(-1, 130):
        if n in sup:
            continue
        assert L.fwav_embed_tables_exact_size(n) == 0
        assert L.fwav_embed_tables_exact(n, out.ctypes.data) == -1
        msg = L.fwav_last_error().decode()
        assert "fwav_embed_tables_exact" in msg and str(n) in msg, msg
        assert L.fwav_debug_dct2_plan(n, 1, x.ctypes.data, out.ctypes.data) == -1
    assert L.fwav_embed_tables_exact(32, None) == -1


def test_tables_write_exactly_their_size(L):
    """fwav_embed_tables_exact fills fwav_embed_tables_exact_size(rs) doubles (no NaN left inside) and nothing after
    them (a NaN guard stays intact); at 4, 8 and 16 it is fwav_embed_tables."""
    guard = 64
    for rs in supported(L):
        size = L.fwav_embed_tables_exact_size(rs)
        assert size > 0
        buf = np.full(size + guard, np.nan)
        assert L.fwav_embed_tables_exact(rs, buf.ctypes.data) == 0
        assert not np.isnan(buf[:size]).any(), rs
        assert np.isnan(buf[size:]).all(), rs
        if rs in (4, 8, 16):
            assert size == L.fwav_embed_tables_size(rs)
            ref = np.zeros(size)
            assert L.fwav_embed_tables(rs, ref.ctypes.data) == 0
            assert np.array_equal(buf[:size].view(np.uint64), ref.view(np.uint64))
        else:
            assert buf[0] == rs
            w = buf[16:16 + rs]
            assert np.array_equal(w.view(np.uint64), np.linspace(1.0, 2.0, rs).view(np.uint64)), rs


def test_python_layers_take_the_mode_and_refuse_bad_ones(L):
    """embedding= exists with the default "matrix" on every public compress entry; an unknown mode, and "pocketfft" at
    a range size without a plan, are ValueErrors that name the range size (checked before any device work)."""
    import inspect

    from fwav import api, cli, dist, engine, hipctypes, stages
    for fn in (engine._compress_device, api.compress_audio, api.process_file_compress, hipctypes.compress,
               hipctypes.pool_embed, dist.compress_sharded, dist.compress_sharded_device, dist.compress_sharded_start):
        assert inspect.signature(fn).parameters["embedding"].default == "matrix", fn
    assert engine.check_embedding("pocketfft", 32) == "pocketfft"
    assert engine.check_embedding("matrix", 51) == "matrix"
    for check in (engine.check_embedding, lambda m, rs: stages.embed_tables_host(rs, m)):
        with pytest.raises(ValueError, match="range size 51"):
            check("pocketfft", 51)
        with pytest.raises(ValueError, match="'matrix' or 'pocketfft'"):
            check("scipy", 8)
    with pytest.raises(SystemExit):
        cli.main(["compress", "in.wav", "out", "--embedding", "scipy"])
    # the sharded compress validates the mode on every rank before its first collective (no process group needed to
    # get the error), and does not take one beside a compute of the caller's own, which would ignore it
    with pytest.raises(ValueError, match="range size 51"):
        dist.compress_sharded_start(None, 13056, 8, embedding="pocketfft")
    with pytest.raises(ValueError, match="'matrix' or 'pocketfft'"):
        dist.compress_sharded_start(None, 8192, 8, embedding="scipy")
    with pytest.raises(ValueError, match="default compute"):
        dist.compress_sharded_start(None, 8192, 8, compute=lambda *a: None, embedding="pocketfft")
