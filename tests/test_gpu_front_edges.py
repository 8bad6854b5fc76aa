"""The stages before the search on the device — voiced detection and range formation (fwav_signal.hip), the domain
pool, the embedding and its fp16 tables (fwav_pool_embed.hip) — called through the C ABI on the edge inputs of
tests/front_edges.py, against the reference's own recorded outputs (tests/golden/front_edges.npz) and against the
oracle, which tests/test_front_edges_cpu.py pins to that fixture.

Bars.  Exact embedding (k_embed<4|8|16>, k_embed_exact), pool, voiced mask and ranges: bit-equal, except that a NaN
matches any NaN; no row and no case is left out.  Matrix embedding (k_embed<0>): the bars of
test_gpu_generic_rs.test_embedding on every finite row of the table.  fp16 tables: equal as uint16 to a numpy
restatement (every NaN made 0x7e00 on both sides)."""
import functools
import json
import os

import numpy as np
import pytest

import front_edges as FE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fwav import engine  # noqa: E402
from fwav._lib import call, size_call  # noqa: E402
from oracle import fractal_oracle as O  # noqa: E402

F32 = np.float32


def dev():
    return torch.device("cuda", 0)


def td(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def fixture():
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "front_edges.npz"))
    return fx, json.loads(str(fx["params"]))


@functools.lru_cache(maxsize=None)
def table(rs):
    rows, names = FE.embed_rows(rs)
    assert FE.same_bits_or_nan(rows, fixture()[0][f"rows_rs{rs}"])
    return rows, names


# ------------------------------------------------------------------------------------------------ embedding
def embed_rows_call(fn, rows, mode, want16=False):
    """fwav_embed_rows / fwav_embed_rows_exact on caller rows f32[n, rs] → emb f32[n, 16] (and the fp16 table)."""
    n, rs = rows.shape
    x = td(rows.reshape(-1))
    tab = engine.embed_tables(rs, dev(), mode)
    emb = torch.full((n * 16,), 7.0, dtype=torch.float32, device=dev())
    e16 = None
    if want16:
        e16 = torch.full((size_call("fwav_emb16_elems", n),), 0x7777, dtype=torch.int16, device=dev())
    call(fn, x.data_ptr(), n, rs, tab.data_ptr(), emb.data_ptr(), None if e16 is None else e16.data_ptr(), stream())
    torch.cuda.synchronize()
    out = emb.cpu().numpy().reshape(n, 16)
    return (out, e16.cpu().numpy().view(np.uint16)) if want16 else out


def check_rows(got, want, names, where, first=0):
    bad = FE.bad_rows(got, want)
    assert not bad, (where, [(first + r, names[(first + r) % FE.N_ROWS], got[r], want[r]) for r in bad[:3]])


CALLER_CASES = ([("fwav_embed_rows", rs, "matrix") for rs in FE.EMBED_FIXED]
                + [("fwav_embed_rows_exact", rs, "pocketfft") for rs in FE.EMBED_PLAN + (8,)])


@pytest.mark.parametrize("fn,rs,mode", CALLER_CASES)
def test_embedding_of_caller_rows_is_the_reference(fn, rs, mode):
    """fwav_embed_rows (k_embed<4|8|16>) and fwav_embed_rows_exact (every k_embed_exact instantiation, and 8 again: it
    routes to k_embed<8>) at width 16: every row alone, every slice of 63, 64 and 65 rows, all 67 rows, and the table
    tiled 5 times (335 rows: more than one 256-row chunk and 64-thread group) — every copy of every row equals the
    reference's multi_head_embedding bit for bit (a NaN matches any NaN)."""
    fx, _ = fixture()
    rows, names = table(rs)
    want = fx[f"emb_rs{rs}_w16"]
    n = FE.N_ROWS
    for a in range(n):
        check_rows(embed_rows_call(fn, rows[a:a + 1], mode), want[a:a + 1], names, f"{fn} rs {rs} row {a} alone", a)
    for m in (63, 64, 65, 67):
        for a in range(n - m + 1):
            check_rows(embed_rows_call(fn, rows[a:a + m], mode), want[a:a + m], names, f"{fn} rs {rs} rows [{a}, {a + m})", a)
    got = embed_rows_call(fn, np.tile(rows, (5, 1)), mode)
    check_rows(got, np.tile(want, (5, 1)), names, f"{fn} rs {rs} tiled 5x")
    assert not got[names.index("zero")].any()
    nan = np.isnan(want).any(axis=1)
    print(f"{fn} rs {rs}: 67 rows x (1 + 13 slices + 5 copies), {int(nan.sum())} rows hold a NaN")


def pool_embed_call(fn, sig, tile, rs, step, mode, width):
    """fwav_pool_embed / _exact / _dim → (pool f32[nd, rs], emb f32[nd, width])."""
    x = td(sig)
    n = x.numel()
    nd = (n - tile) // step + 1
    tab = engine.embed_tables(rs, dev(), mode, width)
    pool = torch.full((nd * rs,), 7.0, dtype=torch.float32, device=dev())
    emb = torch.full((nd * width,), 7.0, dtype=torch.float32, device=dev())
    wsn = size_call("fwav_pool_workspace_size", n, tile, rs, step)
    ws = torch.empty(max(wsn, 16), dtype=torch.uint8, device=dev())
    args = [x.data_ptr(), n, tile, rs, step] + ([width] if fn.endswith("_dim") else []) + [
        tab.data_ptr(), pool.data_ptr(), emb.data_ptr(), None, ws.data_ptr(), wsn, stream()]
    call(fn, *args)
    torch.cuda.synchronize()
    return pool.cpu().numpy().reshape(nd, rs), emb.cpu().numpy().reshape(nd, width)


POOL_ENTRY_CASES = ([("fwav_pool_embed", rs, "matrix", 16) for rs in FE.EMBED_FIXED]
                    + [("fwav_pool_embed_exact", rs, "pocketfft", 16) for rs in FE.EMBED_PLAN + (8,)]
                    + [("fwav_pool_embed_dim", rs, "matrix", 32) for rs in FE.EMBED_FIXED])


@pytest.mark.parametrize("fn,rs,mode,width", POOL_ENTRY_CASES)
def test_embedding_through_the_pool_entry_points(fn, rs, mode, width):
    """The signal is the table's rows one after the other and tile = rs (block length 1).  step = rs: k_domain_pool
    makes pool row i the table's row i (rows of rs floats).  step = 1: the block-means layout (rows read with stride
    from S) makes pool row i·rs the table's row i.  Those pool rows equal the table bit for bit and their embeddings
    equal the reference's — at width 32 (fwav_pool_embed_dim) too."""
    fx, _ = fixture()
    rows, names = table(rs)
    want = fx[f"emb_rs{rs}_w{width}"]
    sig = rows.reshape(-1)
    for step, stride in ((rs, 1), (1, rs)):
        pool, emb = pool_embed_call(fn, sig, rs, rs, step, mode, width)
        assert len(pool) == (FE.N_ROWS - 1) * stride + 1
        check_rows(pool[::stride], rows, names, f"{fn} rs {rs} step {step}: pool")
        check_rows(emb[::stride], want, names, f"{fn} rs {rs} step {step}: embedding")


@pytest.mark.parametrize("rs,width", FE.MATRIX_SHAPES)
def test_matrix_embedding_against_the_f64_embedding(rs, width):
    """k_embed<0> (the default at these range sizes) on every finite, non-overflowing row of the table — none left
    out: tests/test_front_edges_cpu.py asserts that none of them has an f64 tonal norm in (0, 1e-6).  Bars of
    test_gpu_generic_rs.test_embedding: tonal within 2⁻²² of the f64 embedding, transient within 2⁻²³ of the f64
    head; a zero row embeds to exact zeros; head norms ≤ 1 + 1e-6."""
    rows, names = FE.embed_rows(rs)
    keep = FE.matrix_rows(names)
    x = np.ascontiguousarray(rows[keep])
    e, t, nrm = FE.f64_heads(x, width)
    assert not np.any((nrm > 0) & (nrm < 1e-6))
    H = width // 2
    if width == 16:
        emb = embed_rows_call("fwav_embed_rows", x, "matrix")
        pool, emb2 = pool_embed_call("fwav_pool_embed", x.reshape(-1), rs, rs, rs, "matrix", 16)
        assert FE.same_bits_or_nan(pool, x) and FE.same_bits_or_nan(emb2, emb)
    else:
        pool, emb = pool_embed_call("fwav_pool_embed_dim", x.reshape(-1), rs, rs, rs, "matrix", width)
        assert FE.same_bits_or_nan(pool, x)
    assert np.isfinite(emb).all()
    d_ton = np.abs(emb[:, :H].astype(np.float64) - e).max()
    d_tr = np.abs(emb[:, H:].astype(np.float64) - t).max()
    print(f"matrix path rs {rs} width {width}: {len(keep)} rows, tonal max |device - f64| = {d_ton:.3e} (bar "
          f"{2.0 ** -22:.3e}), transient max |device - f64| = {d_tr:.3e} (bar {2.0 ** -23:.3e})")
    assert d_ton <= 2.0 ** -22
    assert d_tr <= 2.0 ** -23
    assert names[keep[0]] == "zero" and not emb[0].any()
    for head in (emb[:, :H].astype(np.float64), emb[:, H:].astype(np.float64)):
        assert np.sqrt((head ** 2).sum(1)).max() <= 1 + 1e-6


# ------------------------------------------------------------------------------------------------ fp16 tables
def emb16_from_emb(emb):
    nd = len(emb)
    e = td(np.ascontiguousarray(emb, F32).reshape(-1))
    e16 = torch.full((size_call("fwav_emb16_elems", nd),), 0x7777, dtype=torch.int16, device=dev())
    call("fwav_emb16_from_emb", e.data_ptr(), nd, e16.data_ptr(), stream())
    torch.cuda.synchronize()
    return e16.cpu().numpy().view(np.uint16)


def check16(got, emb, where):
    want = FE.emb16_tables(emb)
    got = FE.canonical16(got)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (where, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("nd", [1, 255, 256, 257, 335])
def test_fp16_tables_against_numpy(nd):
    """store_emb16 — hi = f16(x), lo = f16(x − hi), tiled [chunk][half][256][8], the second table n16/2 further on,
    padded rows zero — against numpy's conversions (round to nearest even, subnormals kept): the table fwav_embed_rows
    writes beside the device's embedding of the edge rows (rs 4, 8 and 16; NaN and zero rows among them), the one
    fwav_emb16_from_emb writes from that embedding, and fwav_emb16_from_emb on a table of fp16 subnormals, exact
    halfway cases of both parities, values around half the smallest subnormal and ±65504."""
    for rs in FE.EMBED_FIXED:
        rows, _ = table(rs)
        x = np.ascontiguousarray(np.tile(rows, (5, 1))[:nd])
        emb, e16 = embed_rows_call("fwav_embed_rows", x, "matrix", want16=True)
        check16(e16, emb, f"fwav_embed_rows rs {rs} nd {nd}")
        check16(emb16_from_emb(emb), emb, f"fwav_emb16_from_emb(device embedding) rs {rs} nd {nd}")
    rows, _ = table(19)
    emb, e16 = embed_rows_call("fwav_embed_rows_exact", np.ascontiguousarray(np.tile(rows, (5, 1))[:nd]), "pocketfft",
                               want16=True)
    check16(e16, emb, f"fwav_embed_rows_exact rs 19 nd {nd}")
    sp = FE.fp16_special_table(nd)
    check16(emb16_from_emb(sp), sp, f"fwav_emb16_from_emb(special values) nd {nd}")


# ------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("rs,step", FE.POOL_CONFIGS)
def test_pool_at_every_block_length(rs, step):
    """fwav_pool_embed on pool_signal for every block length 1 … 319 (what compress_audio reaches) and 511, 512, 513,
    1023, 1024 (what the C ABI accepts).  rs 4, step 1: k_block_means<0 / 128 / 256>; rs 5, step 2: k_domain_pool at
    odd block lengths (tile % rs = 1), block means read with stride bl / 2 at even ones.  Every pool row equals
    O.domain_pool (pinned to numpy's mean at each of these lengths, and to the reference) and the recorded reference
    rows, NaN ≡ NaN; the first 35 rows are finite."""
    fx, _ = fixture()
    failed = []
    for bl in FE.POOL_BL_SWEEP:
        sig, tile = FE.pool_signal(bl, rs, step)
        with np.errstate(all="ignore"):
            want = O.domain_pool(sig, tile, rs, step)
        pool, _ = pool_embed_call("fwav_pool_embed", sig, tile, rs, step, "matrix", 16)
        assert pool.shape == want.shape == (FE.N_DOMAINS, rs)
        bad = FE.bad_rows(pool, want)
        if bl in FE.POOL_BL_FIXTURE:
            bad = sorted(set(bad) | set(FE.bad_rows(pool, fx[f"pool_rs{rs}_s{step}_bl{bl}"])))
        if bad:
            failed.append((bl, len(bad), bad[:4]))
    print(f"pool rs {rs} step {step}: {len(FE.POOL_BL_SWEEP)} block lengths x {FE.N_DOMAINS} rows")
    assert not failed, f"(block length, rows that differ, first rows): {failed}"


# ------------------------------------------------------------------------------------------------ voiced + ranges
def voiced_ranges(sig, frame, window, hi, lo, want_mask=True):
    """fwav_voiced_ranges → (ranges f32[nr, rs], mask u8[n]); want_mask=False passes mask_out = NULL (→ None)."""
    n = len(sig)
    rs = frame // 2
    nr = -(-n // rs)
    x = td(sig)
    wsn = size_call("fwav_voiced_workspace_size", n, frame)
    ws = torch.empty(wsn, dtype=torch.uint8, device=dev())
    ranges = torch.full((nr * rs,), 7.0, dtype=torch.float32, device=dev())
    mask = torch.full((n,), 7, dtype=torch.uint8, device=dev())
    call("fwav_voiced_ranges", x.data_ptr(), n, rs, frame, window, float(F32(hi)), float(F32(lo)), ranges.data_ptr(),
         nr, mask.data_ptr() if want_mask else None, ws.data_ptr(), wsn, stream())
    torch.cuda.synchronize()
    return ranges.cpu().numpy().reshape(nr, rs), mask.cpu().numpy() if want_mask else None


def check_voiced(sig, frame, window, hi, lo, recorded, where, null_mask=False):
    """null_mask: the call without a mask buffer (what engine.compress_device makes) gives the same ranges too."""
    want = O.voiced_detection(sig, frame, hi, smooth_window=window, low_threshold=lo)
    ranges, mask = voiced_ranges(sig, frame, window, hi, lo)
    if null_mask:
        r2, _ = voiced_ranges(sig, frame, window, hi, lo, want_mask=False)
        assert np.array_equal(r2.view(np.uint32), ranges.view(np.uint32)), (where, "mask_out = NULL")
    if recorded is not None:
        assert np.array_equal(mask[::frame], recorded), (where, "the reference's mask")
    assert np.array_equal(mask, want), (where, np.nonzero(mask != want)[0][:8] // frame)
    wr, _ = O.form_ranges(sig, want, frame // 2)
    assert ranges.shape == wr.shape and np.array_equal(ranges.view(np.uint32), wr.view(np.uint32)), where


@pytest.mark.parametrize("frame", FE.LONG_FRAMES)
def test_frame_energy_at_the_longest_frames(frame):
    """k_frame_energy's pairwise sum at frame lengths up to the 1024 the C ABI accepts, those included at which
    numpy splits a fourth time (970, 1022, 1023).  The energy itself is not returned, so the thresholds pin it: with
    smooth_window 1, lo = 0 and hi = the oracle's energy of the second (louder, reflect-padded) frame the mask stays 0;
    with hi one float lower that frame is voiced.  The device agrees on both only if its energy is that float."""
    for seed in range(3):
        sig = FE.long_frame_signal(frame, seed)
        e = O.frame_energies(sig, frame)
        assert len(e) == 2 and e[1] > e[0] > 0
        for hi, voiced in ((e[1], 0), (np.nextafter(e[1], F32(0)), 1)):
            want = O.voiced_detection(sig, frame, hi, smooth_window=1, low_threshold=0.0)
            assert want[0] == 0 and want[-1] == voiced
            check_voiced(sig, frame, 1, hi, 0.0, None, f"frame {frame} seed {seed} hi {hi!r}")


@pytest.mark.parametrize("frame", FE.VOICED_FRAMES)
def test_voiced_mask_and_ranges(frame):
    """fwav_voiced_ranges on voiced_signal (long runs of frames that keep the state, everywhere) at 1 … 6, 64, 65,
    1023, 1024, 1025 and 2049 frames, a last frame of 1 sample, of frame − 1 and a whole one, smooth_window 5 (and 1 at
    frame 8): the mask equals the reference's where recorded (frames 8 and 38) and O.voiced_detection, the ranges
    equal O.form_ranges.  Frame 8 also runs the signals of 1 … 9 samples (n < frame: the reflect pad wraps more than
    once); frames 8 and 38 the cases whose hi and lo equal a frame's smoothed energy."""
    fx, _ = fixture()
    thr = FE.VOICED_THR
    hi, lo = F32(thr), F32(thr * 0.5)
    n_cases = 0
    for f, nf, tail, w in FE.voiced_cases((frame,)):
        key = f"vm_f{f}_n{nf}_t{tail}_w{w}"
        assert (key in fx) == (frame in FE.FIXTURE_FRAMES)
        check_voiced(FE.voiced_signal(f, nf, tail), f, w, hi, lo, fx[key] if key in fx else None, key)
        n_cases += 1
    if frame == 8:
        for n in FE.TINY_LENGTHS:
            check_voiced(fx[f"tiny_sig_{n}"], 8, 5, hi, lo, fx[f"tiny_vm_{n}"], f"{n} samples")
            n_cases += 1
    for k, (f, nf, tail) in enumerate(FE.EQUAL_CASES):
        if f == frame:
            h, l = fx[f"eq_thr_{k}"]
            check_voiced(FE.voiced_signal(f, nf, tail), f, 5, h, l, fx[f"eq_vm_{k}"], f"equality case {k}")
            n_cases += 1
    print(f"frame {frame}: {n_cases} signals")
