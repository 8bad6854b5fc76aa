"""CPU pins of the front-end edge table (no GPU): tests/golden/front_edges.npz holds the reference's own outputs
(tests/golden/make_front_edges.py) on the inputs of tests/front_edges.py — embedding rows around both 1e-8 switches,
with denormal, underflowing and overflowing squares, inf and NaN; voiced masks with long runs of frames that keep the
state, at frame counts around a thread's 4 frames, a wave and the 1024-frame block, signals shorter than a frame and
thresholds equal to a frame's energy; pool rows at block lengths on every path of the pairwise sum with denormal,
overflowing, inf and NaN stretches.

Here: the builders still make the recorded inputs; the oracle (O.embed, O.voiced_detection, O.domain_pool) reproduces
every recorded output bit for bit (a NaN matches any NaN), which makes it the reference of the wider sweeps of
tests/test_gpu_front_edges.py; the device's DCT code, instantiated on the host, equals scipy on the table's rows; and
the edges are present (asserted on the oracle's values)."""
import json
import os

import numpy as np
import pytest

import front_edges as FE
from oracle import fractal_oracle as O

F32 = np.float32


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "front_edges.npz"))


@pytest.fixture(scope="module")
def meta(fx):
    return json.loads(str(fx["params"]))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    from fwav import _lib
    return _lib.lib()


def test_fixture_lists_what_the_builders_make(fx, meta):
    assert meta["n_rows"] == FE.N_ROWS
    assert [tuple(s) for s in meta["embed_shapes"]] == list(FE.EMBED_SHAPES)
    assert [tuple(c) for c in meta["voiced"]] == FE.voiced_cases(FE.FIXTURE_FRAMES)
    assert tuple(meta["tiny"]) == FE.TINY_LENGTHS
    assert [tuple(c) for c in meta["equal"]] == list(FE.EQUAL_CASES)
    assert [tuple(c) for c in meta["pool_configs"]] == list(FE.POOL_CONFIGS)
    assert tuple(meta["pool_bl"]) == FE.POOL_BL_FIXTURE
    for rs in sorted({rs for rs, _ in FE.EMBED_SHAPES}):
        rows, names = FE.embed_rows(rs)
        assert FE.same_bits_or_nan(rows, fx[f"rows_rs{rs}"]), rs
        assert len(names) == FE.N_ROWS == len(rows)
    for frame, nf, tail, w in FE.voiced_cases(FE.FIXTURE_FRAMES):
        tag = f"f{frame}_n{nf}_t{tail}_w{w}"
        assert FE.digest(FE.voiced_signal(frame, nf, tail)) == meta["inputs"]["voiced_" + tag], tag
    for n in FE.TINY_LENGTHS:
        assert np.array_equal(FE.tiny_signal(n).view(np.uint32), fx[f"tiny_sig_{n}"].view(np.uint32))
    for rs, step in FE.POOL_CONFIGS:
        for bl in FE.POOL_BL_FIXTURE:
            sig, tile = FE.pool_signal(bl, rs, step)
            assert tile == rs * bl + bl % 2
            assert FE.digest(sig) == meta["inputs"][f"pool_rs{rs}_s{step}_bl{bl}"], (rs, step, bl)


@pytest.mark.parametrize("rs,width", FE.EMBED_SHAPES)
def test_oracle_embedding_is_the_reference(fx, meta, rs, width):
    """O.embed on all 67 rows against multi_head_embedding's recorded rows; at most 9 rows hold a NaN (the rest is
    compared bit for bit), and zero rows embed to zeros."""
    rows, names = FE.embed_rows(rs)
    want = fx[f"emb_rs{rs}_w{width}"]
    with np.errstate(all="ignore"):
        got = O.embed(rows, emb_dim=width)
    bad = FE.bad_rows(got, want)
    assert not bad, [(r, names[r], got[r], want[r]) for r in bad[:3]]
    nan = np.isnan(want).any(axis=1)
    assert nan.sum() <= 9 and [names[i] for i in np.nonzero(nan)[0]] == meta["nan_rows"][f"rs{rs}_w{width}"]
    assert not want[names.index("zero")].any()


def test_embedding_edges_are_present():
    """On the builder's own rows: denormal inputs, squares that are denormal, that underflow to 0 and that overflow;
    rows whose two heads take different sides of the 1e-8 switch (un-normalised norms in f64); −0.0 nowhere."""
    split = 0
    for rs in sorted({rs for rs, _ in FE.EMBED_SHAPES}):
        rows, names = FE.embed_rows(rs)
        fin = rows[np.isfinite(rows).all(axis=1)]
        tiny = np.finfo(F32).tiny
        assert np.any((np.abs(fin) < tiny) & (fin != 0)), rs
        with np.errstate(all="ignore"):
            sq = fin * fin
        assert np.any((sq < tiny) & (sq != 0)) and np.any((sq == 0) & (fin != 0)) and np.any(np.isinf(sq)), rs
        sw = np.array([i for i, nm in enumerate(names) if nm in [f"b*1e{e}" for e in FE.E_SWITCH]])
        assert len(sw) == len(FE.E_SWITCH)
        x = rows[sw].astype(np.float64)
        import scipy.fftpack
        w = np.linspace(1.0, 2.0, rs)
        ton = (scipy.fftpack.dct(x, norm="ortho", axis=-1) * w)[:, 1:9]
        tra = scipy.fftpack.dct(np.diff(x, axis=-1, prepend=x[:, :1]) * w, norm="ortho", axis=-1)[:, :8]
        nt, nr = np.sqrt((ton ** 2).sum(1)), np.sqrt((tra ** 2).sum(1))
        assert nt.min() < 1e-8 < nt.max() and nr.min() < 1e-8 < nr.max(), rs
        split += int(((nt > 1e-8) != (nr > 1e-8)).sum())
    assert split >= 1


@pytest.mark.parametrize("rs,width", FE.MATRIX_SHAPES)
def test_matrix_rows_are_clear_of_the_switch(rs, width):
    """The rows the matrix path is measured on (tests/test_gpu_front_edges.py leaves none of them out): finite, and
    none with an f64 un-normalised tonal norm in (0, 1e-6), where the two sides might normalise differently."""
    rows, names = FE.embed_rows(rs)
    keep = FE.matrix_rows(names)
    assert len(keep) == 6 + FE.N_ROWS - names.index("random, scale 0.001")
    e, t, nrm = FE.f64_heads(rows[keep], width)
    assert np.isfinite(e).all() and np.isfinite(t).all()
    assert not np.any((nrm > 0) & (nrm < 1e-6)), nrm
    assert nrm[0] == 0 and not e[0].any() and not t[0].any()


def dct_host(L, n, dbl, x):
    """fwav_debug_dct2 (the fixed plans, n = 4, 8, 16) and fwav_debug_dct2_plan (the general plan) row by row."""
    x = np.ascontiguousarray(x, np.float64)
    outs = []
    fns = ([L.fwav_debug_dct2] if n in (4, 8, 16) else []) + [L.fwav_debug_dct2_plan]
    for fn in fns:
        out = np.zeros_like(x)
        for r in range(len(x)):
            assert fn(n, dbl, x[r].ctypes.data, out[r].ctypes.data) == 0
        outs.append(out)
    return outs


@pytest.mark.parametrize("rs", sorted({rs for rs, _ in FE.EMBED_SHAPES}))
def test_device_dct_code_on_the_host_is_scipy(L, rs):
    """The DCT code of k_embed / k_embed_exact, compiled for the host, on the table's rows (f32: the tonal head's
    input) and on their weighted first differences (f64: the transient head's input): scipy's own result bit for bit
    — which outputs of an overflowing or non-finite row are inf and which NaN included (a NaN matches any NaN)."""
    import scipy.fftpack
    rows, names = FE.embed_rows(rs)
    with np.errstate(all="ignore"):
        want32 = scipy.fftpack.dct(rows, norm="ortho", axis=-1)
        d = np.diff(rows, axis=-1, prepend=rows[:, :1]) * np.linspace(1.0, 2.0, rs)
        want64 = scipy.fftpack.dct(d, norm="ortho", axis=-1)
        want64r = scipy.fftpack.dct(rows.astype(np.float64), norm="ortho", axis=-1)
    assert want32.dtype == F32 and want64.dtype == np.float64
    for got in dct_host(L, rs, 0, rows):
        bad = FE.bad_rows(got.astype(F32), want32)
        assert not bad, ("f32", [(r, names[r]) for r in bad])
    for x, want in ((d, want64), (rows.astype(np.float64), want64r)):
        for got in dct_host(L, rs, 1, x):
            bad = [r for r in range(len(x)) if not FE.same_or_nan(got[r], want[r])]
            assert not bad, ("f64", [(r, names[r]) for r in bad])


def test_oracle_voiced_mask_is_the_reference(fx):
    """Every recorded mask: frames 8 and 38, 1 … 2049 frames, last frames of 1 sample and of frame − 1, window 5 (and 1
    at frame 8); the signals of 1 … 9 samples; the threshold-equality cases, where hi and lo each equal a frame's
    smoothed energy."""
    n_keep_1025 = {}
    for frame, nf, tail, w in FE.voiced_cases(FE.FIXTURE_FRAMES):
        sig = FE.voiced_signal(frame, nf, tail)
        vm = O.voiced_detection(sig, frame, FE.VOICED_THR, smooth_window=w)
        assert len(vm) == len(sig)
        assert np.array_equal(vm[::frame], fx[f"vm_f{frame}_n{nf}_t{tail}_w{w}"]), (frame, nf, tail, w)
        if nf == 1025 and tail == 0 and w == 5:
            e = O.smooth5(O.frame_energies(sig, frame))
            n_keep_1025[frame] = int(((e <= F32(1e-4)) & (e >= F32(5e-5))).sum())
    assert all(v >= 150 for v in n_keep_1025.values()), n_keep_1025
    for n in FE.TINY_LENGTHS:
        vm = O.voiced_detection(fx[f"tiny_sig_{n}"], 8, FE.VOICED_THR)
        assert np.array_equal(vm[::8], fx[f"tiny_vm_{n}"]), n
    for k, (frame, nf, tail) in enumerate(FE.EQUAL_CASES):
        sig = FE.voiced_signal(frame, nf, tail)
        hi, lo = fx[f"eq_thr_{k}"]
        e = O.smooth5(O.frame_energies(sig, frame))
        assert (e == hi).any() and (e == lo).any() and lo < hi
        vm = O.voiced_detection(sig, frame, hi, low_threshold=lo)
        assert np.array_equal(vm[::frame], fx[f"eq_vm_{k}"]), k
        # equality decides: one float down (up) and the mask is another one
        for h2, l2 in ((np.nextafter(hi, F32(0)), lo), (hi, np.nextafter(lo, F32(1)))):
            assert not np.array_equal(O.voiced_detection(sig, frame, h2, low_threshold=l2)[::frame], fx[f"eq_vm_{k}"])


def test_oracle_frame_energy_is_numpy_at_the_longest_frames():
    """O.frame_energies against fractal.py:889-891 evaluated by numpy itself, at the frame lengths of
    test_gpu_front_edges.test_frame_energy_at_the_longest_frames (those at which the pairwise sum splits a fourth time
    among them); the second frame is the louder one, as that test needs."""
    for frame in FE.LONG_FRAMES:
        for seed in range(3):
            sig = FE.long_frame_signal(frame, seed)
            pad = 2 * frame - len(sig)
            fr = np.pad(sig, (0, pad), mode="reflect").reshape(2, frame)
            want = np.mean(fr * fr, axis=1)
            got = O.frame_energies(sig, frame)
            assert want.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (frame, seed)
            assert got[1] > got[0] > 0


def keep_runs(dec):
    """[(first, last)] of the maximal runs of −1 in dec."""
    k = np.concatenate([[0], (dec < 0).astype(np.int8), [0]])
    d = np.diff(k)
    return list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - 1).tolist()))


def test_oracle_voiced_mask_is_the_sequential_scan_on_the_whole_sweep():
    """O.voiced_detection (a vectorised max-scan) against the reference's loop restated as written
    (front_edges.sequential_mask) on every case of the GPU sweep; and the sweep has what it is there for: runs of
    "keep" frames that cross a thread's 4 frames, a wave's 256 and the 1024-frame block, and that start the signal
    (no decision yet: unvoiced)."""
    cross4 = cross256 = cross1024 = leading = 0
    for frame, nf, tail, w in FE.voiced_cases(FE.VOICED_FRAMES):
        sig = FE.voiced_signal(frame, nf, tail)
        e = O.frame_energies(sig, frame)
        if w > 1:
            e = O.smooth5(e, w)[:nf] if nf < w else O.smooth5(e, w)
        thr = FE.VOICED_THR
        want = FE.sequential_mask(e, thr, thr * 0.5)[:nf]
        got = O.voiced_detection(sig, frame, thr, smooth_window=w)[::frame]
        assert np.array_equal(got, want), (frame, nf, tail, w)
        e = np.asarray(e[:nf], F32)
        dec = np.where(e > F32(thr), 1, np.where(e < F32(thr * 0.5), 0, -1))
        for a, b in keep_runs(dec):
            cross4 += a // 4 != b // 4
            cross256 += a // 256 != b // 256
            cross1024 += a // 1024 != b // 1024
            leading += a == 0
    print(f"keep runs crossing 4 frames: {cross4}, 256: {cross256}, 1024: {cross1024}; leading: {leading}")
    assert cross4 >= 100 and cross256 >= 10 and cross1024 >= 3 and leading >= 3


@pytest.mark.parametrize("rs,step", FE.POOL_CONFIGS)
def test_oracle_pool_is_the_reference_and_numpy(fx, rs, step):
    """O.domain_pool against the recorded build_domains_memmap rows, and against numpy's own float32 mean at every
    block length of the GPU sweep (1 … 319: the 8-lane leaf with a tail, the unequal pairwise split, and 511 … 1024:
    the third recursion level), denormal, overflowing, inf and NaN stretches included."""
    for bl in FE.POOL_BL_SWEEP:
        sig, tile = FE.pool_signal(bl, rs, step)
        with np.errstate(all="ignore"):
            got = O.domain_pool(sig, tile, rs, step)
        assert got.shape == (FE.N_DOMAINS, rs)
        assert FE.same_bits_or_nan(got, FE.numpy_pool(sig, tile, rs, step)), bl
        assert np.isfinite(got[:FE.P_BIG]).all() and not np.isfinite(got[FE.P_INF]).all(), bl
        assert np.isnan(got[FE.P_NAN]).any(), bl
        if bl in FE.POOL_BL_FIXTURE:
            assert FE.same_bits_or_nan(got, fx[f"pool_rs{rs}_s{step}_bl{bl}"]), bl
    # a denormal mean and an overflowed one are among the recorded rows
    p = fx[f"pool_rs{rs}_s{step}_bl9"]
    assert np.any((np.abs(p) < np.finfo(F32).tiny) & (p != 0)) and np.isinf(p).any() and np.isnan(p).any()


def test_fp16_restatement_rounds_to_nearest_even_and_keeps_subnormals():
    """front_edges.emb16_tables (the numpy statement tests/test_gpu_front_edges.py holds the device to) on values
    whose fp16 parts are known by hand."""
    x = np.zeros((1, 16), F32)
    x[0, :8] = [2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65504, -2.0 ** -26, 0.1]
    t = FE.emb16_tables(x).view(np.float16)
    assert len(t) == 2 * 256 * 16
    hi, lo = t[:8].astype(np.float64), t[4096:4104].astype(np.float64)
    assert hi[:7].tolist() == [2.0 ** -24, 0.0, 2.0 ** -23, 1.0, 1 + 2.0 ** -9, 65504.0, -0.0]
    # the halves that f16(x) dropped: 2⁻²⁵ and −2⁻²⁵ are ties that round to (signed) zero again
    assert lo[:7].tolist() == [0.0, 0.0, -0.0, 2.0 ** -11, -(2.0 ** -11), 0.0, -0.0]
    assert 0 < abs(lo[7]) < 2.0 ** -14 and abs(float(F32(0.1)) - hi[7] - lo[7]) <= 2.0 ** -25   # lo is subnormal
    assert not t[8:2048].any() and not t[4104:].any()
    sp = FE.fp16_special_table(257)
    assert np.abs(sp[np.abs(sp) != 65504]).max() <= 1
    h = sp.astype(np.float16)
    assert np.any((h != 0) & (np.abs(h) < 6.2e-5)) and np.any((h == 0) & (sp != 0))
