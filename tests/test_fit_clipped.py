"""compress_audio(fit="clipped") without a device: the option's checks, fwav_affine_fit's argument check, the numpy
restatement's own properties (tests/fit_clipped.py) on the affine edge tables, and the feature's point re-derived on
the CPU — the SNR of the stored tuple as the decoder reproduces it, under both selections.

The gains asserted here are the ones the feature was proposed with: at least 3 dB on speech_like(0.5, 44100) with
query="range" at tiles 2048 and 1024 (measured 4.98 and 22.52 dB)."""
import numpy as np
import pytest

import affine_edges as AE
import fit_clipped as FC
from oracle import fractal_oracle as O

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from fwav import _lib
    return _lib


def test_check_fit():
    from fwav import stages
    assert stages.FITS == ("reference", "clipped")
    for f in stages.FITS:
        assert stages.check_fit(f) == f
    for bad in ("clip", "", None, 1):
        with pytest.raises(ValueError, match="fit must be 'reference' or 'clipped'"):
            stages.check_fit(bad)
    # "numpy" ranks every K-th place tie under the clipped fit; the other orders and the default fit are untouched
    assert stages.tie_mode("numpy", "clipped") == stages.TIE_MODES["numpy_sets"] == 1
    assert stages.tie_mode("numpy", "reference") == stages.TIE_MODES["numpy"] == 0
    for order in ("numpy_sets", "numpy_rows", "index"):
        assert stages.tie_mode(order, "clipped") == stages.tie_mode(order) == stages.TIE_MODES[order]
    with pytest.raises(ValueError):
        stages.tie_mode("numpy", "x")
    with pytest.raises(ValueError):
        stages.tie_mode("scipy", "clipped")


def test_refusals_come_before_any_device_work(monkeypatch):
    pytest.importorskip("torch")
    from fwav import api, engine, hipctypes

    def no_device(*a, **k):
        raise AssertionError("a device was asked for before the arguments were checked")

    monkeypatch.setattr(engine, "require_device", no_device)
    with pytest.raises(ValueError, match="fit must be"):
        api.compress_audio(np.zeros(4096, F32), 44100, 2, fit="clip")
    with pytest.raises(ValueError, match="fit must be"):
        hipctypes.compress(np.zeros(4096, F32), 1024, 32, fit="clip")
    with pytest.raises(ValueError, match="fit must be"):
        hipctypes.affine_batch(np.zeros((1, 4), F32), np.zeros((1, 1), np.int32), np.zeros((1, 4), F32), fit="clip")
    assert engine.check_fit is __import__("fwav.stages", fromlist=["x"]).check_fit and engine.FITS == ("reference", "clipped")
    assert "error" in api.process_file_compress("/nonexistent/in.wav", fit="clipped")


def test_cli_hands_fit_to_the_file_level_call(monkeypatch):
    import inspect
    from fwav import api, cli
    P = cli.build_parser()
    assert P.parse_args(["compress", "in.wav", "out"]).fit == "reference"
    assert P.parse_args(["compress", "in.wav", "out", "--fit", "clipped"]).fit == "clipped"
    with pytest.raises(SystemExit):
        P.parse_args(["compress", "in.wav", "out", "--fit", "clip"])
    seen = {}
    monkeypatch.setattr(cli, "_compress_job", lambda args: seen.setdefault("c", args))
    cli.main(["compress", "in.wav", "outdir", "--fit", "clipped", "--query", "range"])
    cp = list(inspect.signature(api.process_file_compress).parameters)
    got = dict(zip(cp, seen["c"]))
    assert len(seen["c"]) == len(cp) and got["fit"] == "clipped" and got["query"] == "range"


def test_dist_passes_fit_through(lib, monkeypatch):
    """fwav.dist validates fit before its first collective, refuses it beside a compute of the caller's, and its
    default compute hands it to compress_device."""
    pytest.importorskip("torch")
    from fwav import dist, engine
    with pytest.raises(ValueError, match="fit must be"):
        dist.compress_sharded_start(None, 2048, 32, fit="clip")
    with pytest.raises(ValueError, match="apply to the default compute"):
        dist.compress_sharded_start(None, 2048, 32, compute=lambda *a: None, fit="clipped")
    seen = {}

    class R:
        empty = True

    monkeypatch.setattr(engine, "compress_device", lambda *a, **k: seen.update(k) or R())
    assert dist._device_compute(None, 2048, 32, 1e-4, (0, 1), fit="clipped") is None and seen["fit"] == "clipped"
    assert dist._device_compute(None, 2048, 32, 1e-4, (0, 1)) is None and seen["fit"] == "reference"


def test_affine_fit_error_codes_without_gpu(lib):
    """fit outside {0, 1} is FWAV_ERR_ARG before any device work (and before the pointer checks); fit 0 and 1 check
    their arguments as fwav_affine does."""
    import ctypes
    L = lib.lib()
    assert L.fwav_abi_version() == 5  # an addition only
    big = ctypes.c_void_p(16)
    for fit in (2, -1, 7):
        rc = L.fwav_affine_fit(big, 10, 8, big, 64, big, 100, 16.0, big, big, big, big, big, fit, None)
        assert rc == -1 and b"fit" in L.fwav_last_error(), fit
    for fit, name in ((0, b"fwav_affine:"), (1, b"fwav_affine_fit:")):
        rc = L.fwav_affine_fit(None, 10, 8, None, 64, None, 100, 16.0, None, None, None, None, None, fit, None)
        assert rc == -1 and b"null" in L.fwav_last_error() and name in L.fwav_last_error()
        rc = L.fwav_affine_fit(big, 10, 0, big, 64, big, 100, 16.0, big, big, big, big, big, fit, None)
        assert rc == -2
        assert L.fwav_affine_fit(big, 0, 8, big, 64, big, 100, 16.0, big, big, big, big, big, fit, None) == 0


@pytest.mark.parametrize("rs", (4, 5, 8, 16, 19))
def test_restatement_properties_on_the_edge_tables(rs):
    """With a clip that never binds the restatement's error is O.affine's bit for bit; with one that does, its error
    is at most the clipped-formula error of O.affine's slot on every row whose errors are all numbers (a NaN error is
    selected first by contract, as numpy's argmin does); the selection does not depend on the candidates' order."""
    for K in AE.K_ALL:
        ranges, cand, pool, names = AE.build(rs, K)
        with np.errstate(all="ignore"):
            ref = O.affine(ranges, cand, pool, s_clip=1e30)
            got = FC.affine_clipped(ranges, cand, pool, s_clip=1e30)
        assert AE.same_bits_or_nan(got[4], ref[4]), (rs, K)
        for sc in (16.0, 0.5, 0.0):
            with np.errstate(all="ignore"):
                s, o, err, dom = FC.slots_clipped(ranges, cand, pool, sc)
                idx, sb, ob, sym, eb = FC.affine_clipped(ranges, cand, pool, sc)
                e_ref = FC.clipped_error_of_reference_slot(ranges, cand, pool, sc)
            has_nan = np.isnan(err).any(axis=1)
            assert np.array_equal(np.isnan(eb), has_nan), (rs, K, sc)
            with np.errstate(all="ignore"):
                assert np.all(eb[~has_nan] <= e_ref[~has_nan]), (rs, K, sc)
            assert np.all(np.abs(sb[~np.isnan(sb)]) <= abs(F32(sc)))
            # the candidates in reverse order: the same tuples
            with np.errstate(all="ignore"):
                rev = FC.affine_clipped(ranges, cand[:, ::-1].copy(), pool, sc)
            for a, b in zip((idx, sb, ob, sym, eb), rev):
                assert AE.same_bits_or_nan(a, b), (rs, K, sc)
        with np.errstate(all="ignore"):
            idx0 = FC.affine_clipped(ranges, cand, pool, 0.0)[0]
        # s = 0: every valid slot has the error ‖r̄ − R‖, so the lowest valid domain wins (0 where there is none)
        low = np.where((cand >= 0).any(axis=1), np.where(cand < 0, np.iinfo(np.int32).max, cand).min(axis=1), 0)
        assert np.array_equal(idx0[~has_nan], low[~has_nan])
        assert idx0[names.index("all -1")] == 0


# -------------------------------------------------------------------------------- the eight gains, re-derived
TABLE = {  # (signal, tile, query): (SNR by stored err, stored tuple as decoded, clipped selection, matches changed)
    ("speech", 2048, "domain_row"): (18.28, 18.28, 18.28, 0),
    ("speech", 2048, "range"): (28.46, 19.20, 24.18, 128),
    ("speech", 1024, "domain_row"): (27.92, 27.19, 27.92, 115),
    ("speech", 1024, "range"): (60.92, 30.18, 52.70, 980),
    ("sweep", 1024, "domain_row"): (4.31, 0.60, 2.67, 1688),
    ("sweep", 1024, "range"): (33.93, 0.15, 3.83, 1888),
    ("noise", 2048, "domain_row"): (2.60, 2.54, 2.57, 48),
    ("noise", 2048, "range"): (8.62, 7.26, 7.90, 480),
}


@pytest.mark.parametrize("key", list(TABLE), ids=lambda k: f"{k[0]}{k[1]}-{k[2]}")
def test_gain_of_the_clipped_selection(key):
    """Over the searched ranges: the SNR the stored err promises, the SNR of the stored tuple as a decoder reproduces
    it (the reference's slot, its s clipped, its o that of the unclipped s), and the same under the clipped selection,
    whose stored err is that very error.  Printed for all eight rows beside the figures the feature was proposed
    with; the two speech rows with query="range" are asserted to gain at least 3 dB."""
    name, tile, query = key
    c = FC.restated(name, tile, query)
    over = np.isfinite(c["m"][4])
    stored = FC.snr_db(c["ranges"], c["m"][4], over)
    decoded = FC.snr_db(c["ranges"], c["e_stored"], over)
    clipped = FC.snr_db(c["ranges"], c["mc"][4], over)
    assert abs(FC.snr_db(c["ranges"], c["e_stored_c"], over) - clipped) < 1e-3  # err is the stored tuple's error
    changed = int(((c["m"][0] != c["mc"][0]) | (c["m"][3] != c["mc"][3]))[over].sum())
    print(f"{key}: stored-err SNR {stored:.2f} dB, stored tuple as decoded {decoded:.2f} dB, clipped selection "
          f"{clipped:.2f} dB, gain {clipped - decoded:.2f} dB, matches changed {changed} of {int(over.sum())}; "
          f"proposed with {TABLE[key]}")
    assert np.array_equal(np.isfinite(c["mc"][4]), over)  # the same ranges are searched
    assert clipped >= decoded - 1e-6                       # the constrained optimum over the same slots
    if key in (("speech", 2048, "range"), ("speech", 1024, "range")):
        assert clipped - decoded >= 3.0, (stored, decoded, clipped)
